"""SLRC+ in float64 numpy, written from the formulas (not from any kernel): the score, GeneralModel.loss (tests/fpmc_np.py's), the
gradients to the ten parameters and one optimizer step on the rows of the batch.

    t = relational_interval[b, c, r], mask = (t >= 0), dt = t * mask
    alpha = global_alpha + alphas[i, r], pi = pis[i, r] + 0.5, mu = mus[i, r] + 1
    beta = clamp(betas[i, r] + 1, 1e-10, 10), sigma = clamp(sigmas[i, r] + 1, 1e-10, 10)     (gradient passes on [1e-10, 10])
    e = exp(log beta - beta dt), n = exp(-(dt - mu)^2 / (2 sigma^2) - log sigma - log sqrt(2 pi))
    pred[b, c] = <U[u], I[i]> + user_bias[u] + item_bias[i] + sum_r alpha (pi e + (1 - pi) n) mask

tests/test_slrc_cpu.py pins this file to the reference's own numbers (tests/golden/slrc_*.npz); the GPU tests then hold the kernels
to it on shapes the goldens do not have."""
import numpy as np

from fpmc_np import bpr, optimizer_rows, ranks  # noqa: F401  (the loss and the optimizers are the same arithmetic)

GOLDEN_CASES = ("slrc_d16_r1_sgd_b1_k1", "slrc_d32_r3_sgd_b160_k4", "slrc_d64_r3_adam_b77_k99", "slrc_d128_r8_adagrad_b33_k9")
PARAMS = ("U", "I", "user_bias", "item_bias", "global_alpha", "alphas", "pis", "betas", "sigmas", "mus")   # the engine's order
HAWKES = PARAMS[5:]
STATE_KEYS = {"U": "u_embeddings.weight", "I": "i_embeddings.weight", "user_bias": "user_bias.weight", "item_bias": "item_bias.weight",
              "global_alpha": "global_alpha", "alphas": "alphas.weight", "pis": "pis.weight", "betas": "betas.weight",
              "sigmas": "sigmas.weight", "mus": "mus.weight"}
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def f64(P):
    return {k: np.asarray(P[k], dtype=np.float64) for k in PARAMS}


def _excitation(P, iid, iv):
    """-> (excitation [B, C], the partial derivatives d pred / d (alphas, pis, betas, sigmas, mus)[iid, r], each [B, C, R])"""
    iv = np.asarray(iv, dtype=np.float64)
    mask = (iv >= 0).astype(np.float64)
    dt = iv * mask
    alpha = float(P["global_alpha"]) + P["alphas"][iid]
    pi, mu = P["pis"][iid] + 0.5, P["mus"][iid] + 1.0
    xb, xs = P["betas"][iid] + 1.0, P["sigmas"][iid] + 1.0
    beta, sigma = np.clip(xb, 1e-10, 10.0), np.clip(xs, 1e-10, 10.0)
    pass_b = ((xb >= 1e-10) & (xb <= 10.0)).astype(np.float64)
    pass_s = ((xs >= 1e-10) & (xs <= 10.0)).astype(np.float64)
    e = np.exp(np.log(beta) - beta * dt)
    z = dt - mu
    with np.errstate(under="ignore", over="ignore"):
        n = np.exp(-(z * z) / (2.0 * sigma * sigma) - np.log(sigma) - LOG_SQRT_2PI)
        decay = pi * e + (1.0 - pi) * n
        an = alpha * (1.0 - pi) * n
        d = {"alphas": decay * mask,
             "pis": alpha * (e - n) * mask,
             "betas": alpha * pi * e * (1.0 / beta - dt) * mask * pass_b,
             "sigmas": an * ((z * z) / (sigma * sigma * sigma) - 1.0 / sigma) * mask * pass_s,
             "mus": an * (z / (sigma * sigma)) * mask}
    return (alpha * decay * mask).sum(-1), d


def scores(P, uid, iid, iv):
    P = f64(P)
    base = np.einsum("bd,bcd->bc", P["U"][uid], P["I"][iid]) + P["user_bias"].reshape(-1)[uid][:, None] + P["item_bias"].reshape(-1)[iid]
    return base + _excitation(P, iid, iv)[0]


def front_grads(P, uid, iid, iv, gpred):
    """what rc_slrc_fwd_bwd leaves beside pred / loss_vec / gpred: ugrad [B, d], ubgrad [B], hgrad [B * C, 5 R], gagrad [B]"""
    P = f64(P)
    gpred = np.asarray(gpred, dtype=np.float64)
    _, d = _excitation(P, iid, iv)
    B, Cn = iid.shape
    hgrad = np.concatenate([gpred[:, :, None] * d[k] for k in HAWKES], axis=-1).reshape(B * Cn, -1)
    return (np.einsum("bc,bcd->bd", gpred, P["I"][iid]), gpred.sum(axis=1), hgrad, (gpred * d["alphas"].sum(-1)).sum(axis=1))


def dense_grads(P, uid, iid, iv, gpred):
    """the ten dense gradients, a dict over PARAMS with the parameters' own shapes"""
    P = f64(P)
    gpred = np.asarray(gpred, dtype=np.float64)
    _, d = _excitation(P, iid, iv)
    G = {k: np.zeros_like(P[k]) for k in PARAMS}
    flat = iid.reshape(-1)
    np.add.at(G["U"], uid, np.einsum("bc,bcd->bd", gpred, P["I"][iid]))
    np.add.at(G["I"], flat, (gpred[:, :, None] * P["U"][uid][:, None, :]).reshape(flat.size, -1))
    np.add.at(G["user_bias"].reshape(-1), uid, gpred.sum(axis=1))
    np.add.at(G["item_bias"].reshape(-1), flat, gpred.reshape(-1))
    G["global_alpha"] = np.asarray((gpred * d["alphas"].sum(-1)).sum())
    for k in HAWKES:
        np.add.at(G[k], flat, (gpred[:, :, None] * d[k]).reshape(flat.size, -1))
    return G


def step(P, uid, iid, iv, opt, lr, l2, states=None, step_no=1):
    """one row-wise training step -> (loss, new parameters, new states {name: (m, v)}): rows of the batch only, the two bias tables
    without weight decay, global_alpha (a single dense float) with it"""
    loss_vec, gpred = bpr(scores(P, uid, iid, iv))
    G = dense_grads(P, uid, iid, iv, gpred)
    new, st = {}, {}
    for k in PARAMS:
        m, v = (states or {}).get(k, (None, None))
        W, Gk = np.asarray(P[k], np.float64).reshape(-1, 1) if k == "global_alpha" else P[k], G[k].reshape(-1, 1) if k == "global_alpha" else G[k]
        rows = np.array([0]) if k == "global_alpha" else (uid if k in ("U", "user_bias") else iid)
        W1, mk, vk = optimizer_rows(W, Gk, rows, opt, lr, 0.0 if "bias" in k else l2, m, v, step_no)
        new[k] = W1.reshape(np.shape(P[k]))
        st[k] = (mk, vk)
    return loss_vec.mean(), new, st
