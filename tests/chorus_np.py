"""Chorus's stage 2 in float64 numpy, written from the formulas (not from any kernel): the score in the reference's own summation
(z first, then the dot product with the user), GeneralModel.loss (tests/fpmc_np.py's), the gradients to the nine parameters and one
row-wise optimizer step with the three hyper records of Chorus.customize_parameters.

    t = relational_interval[b, c, r], on = (t >= 0), dt = on ? t : 0, k = category_id[b, c]
    beta = clamp(betas[k, r] + 1, 1e-10, 10), sigma = clamp(sigmas[k, r] + 1, 1e-10, 10), mu = mus[k, r] + 1
    n(x; m, s) = exp(-(x - m)^2 / (2 s^2) - log s - log sqrt(2 pi))
    kind 0: kappa = exp(log beta - beta dt)     kind 1: kappa = n(dt; 0, beta)     kind 2: kappa = n(dt; mu, sigma) - n(dt; 0, beta)
    decay = on * clamp(kappa, -1, 1),  S = sum_r decay_r,  z = (1 + S) I[i] + sum_r decay_r Rel[r]
    BPR: pred = <U[u], z> + user_bias[u] + item_bias[i]        GMF: pred = <w o U[u], z>
Both clamps pass the gradient on the closed interval.  Stage 1 is tests/cfkg_np.py's arithmetic on (I, Rel)."""
import numpy as np

from fpmc_np import bpr, optimizer_rows  # noqa: F401  (the loss and the optimizers are the same arithmetic)

PARAMS = ("U", "I", "Rel", "betas", "mus", "sigmas", "w", "user_bias", "item_bias")   # the engine's (= the definition) order
CAT_TABLES = ("betas", "sigmas", "mus")                                               # kgrad's column blocks
STATE_KEYS = {"U": "u_embeddings.weight", "I": "i_embeddings.weight", "Rel": "r_embeddings.weight", "betas": "betas.weight",
              "mus": "mus.weight", "sigmas": "sigmas.weight", "w": "prediction.weight", "user_bias": "user_bias.weight",
              "item_bias": "item_bias.weight"}
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def kinds_of(item_relations):
    return [0] + [1 if "complement" in c else (2 if "substitute" in c else 0) for c in item_relations]


def f64(P):
    return {k: np.asarray(P[k], dtype=np.float64) for k in PARAMS}


def kernels(P, cid, iv, kinds):
    """-> (decay [B, C, R], unclamped kappa, {table: d decay / d table[cid, r]} with the mask and both gates applied)"""
    iv = np.asarray(iv, dtype=np.float64)
    on = iv >= 0
    dt = np.where(on, iv, 0.0)
    xb, xs, mu = P["betas"][cid] + 1.0, P["sigmas"][cid] + 1.0, P["mus"][cid] + 1.0
    beta, sigma = np.clip(xb, 1e-10, 10.0), np.clip(xs, 1e-10, 10.0)
    pass_b, pass_s = (xb >= 1e-10) & (xb <= 10.0), (xs >= 1e-10) & (xs <= 10.0)
    kind = np.broadcast_to(np.asarray(kinds), iv.shape)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(np.log(beta) - beta * dt)
        n0 = np.exp(-(dt * dt) / (2.0 * beta * beta) - np.log(beta) - LOG_SQRT_2PI)
        z = dt - mu
        n1 = np.exp(-(z * z) / (2.0 * sigma * sigma) - np.log(sigma) - LOG_SQRT_2PI)
        dn0 = n0 * ((dt * dt) / beta ** 3 - 1.0 / beta)
        kappa = np.where(kind == 0, e, np.where(kind == 1, n0, n1 - n0))
        db = np.where(kind == 0, e * (1.0 / beta - dt), np.where(kind == 1, dn0, -dn0))
        ds = np.where(kind == 2, n1 * ((z * z) / sigma ** 3 - 1.0 / sigma), 0.0)
        dm = np.where(kind == 2, n1 * (z / (sigma * sigma)), 0.0)
    gate = on & (kappa >= -1.0) & (kappa <= 1.0)
    decay = np.where(on, np.clip(kappa, -1.0, 1.0), 0.0)
    d = {"betas": np.where(gate & pass_b, db, 0.0), "sigmas": np.where(gate & pass_s, ds, 0.0), "mus": np.where(gate, dm, 0.0)}
    return decay, kappa, d


def _uprime(P, uid, gmf):
    return P["U"][uid] * P["w"].reshape(-1) if gmf else P["U"][uid]


def scores(P, uid, iid, cid, iv, kinds, gmf=False):
    P = f64(P)
    decay, _, _ = kernels(P, cid, iv, kinds)
    z = (1.0 + decay.sum(-1))[:, :, None] * P["I"][iid] + np.einsum("bcr,rd->bcd", decay, P["Rel"])
    pred = np.einsum("bd,bcd->bc", _uprime(P, uid, gmf), z)
    if not gmf:
        pred = pred + P["user_bias"].reshape(-1)[uid][:, None] + P["item_bias"].reshape(-1)[iid]
    return pred


def front_grads(P, uid, iid, cid, iv, kinds, gpred, gmf=False):
    """what rc_chorus_fwd_bwd leaves beside pred / loss_vec / gpred: a dict of coef [B, C], ugrad [B, d], ubgrad [B], kgrad
    [B * C, 3 R], GRel [R, d], gw [d], uprime [B, d]"""
    P = f64(P)
    g = np.asarray(gpred, dtype=np.float64)
    B, Cn = iid.shape
    decay, _, d = kernels(P, cid, iv, kinds)
    up = _uprime(P, uid, gmf)
    S = decay.sum(-1)
    z = (1.0 + S)[:, :, None] * P["I"][iid] + np.einsum("bcr,rd->bcd", decay, P["Rel"])
    gz = np.einsum("bc,bcd->bd", g, z)
    ddecay = g[:, :, None] * (np.einsum("bd,bcd->bc", up, P["I"][iid])[:, :, None] + np.einsum("bd,rd->br", up, P["Rel"])[:, None, :])
    return {"coef": g * (1.0 + S), "ugrad": gz * P["w"].reshape(-1) if gmf else gz, "ubgrad": g.sum(axis=1),
            "kgrad": np.concatenate([ddecay * d[k] for k in CAT_TABLES], axis=-1).reshape(B * Cn, -1),
            "GRel": np.einsum("bcr,bd->rd", g[:, :, None] * decay, up), "gw": (P["U"][uid] * gz).sum(axis=0), "uprime": up}


def dense_grads(P, uid, iid, cid, iv, kinds, gpred, gmf=False):
    """the nine dense gradients, a dict over PARAMS with the parameters' own shapes; None where the head does not read the
    parameter (w under BPR, the biases under GMF, sigmas and mus without a kind-2 relation)"""
    P = f64(P)
    g = np.asarray(gpred, dtype=np.float64)
    F = front_grads(P, uid, iid, cid, iv, kinds, g, gmf)
    G = {k: np.zeros_like(P[k]) for k in PARAMS}
    flat = iid.reshape(-1)
    np.add.at(G["U"], uid, F["ugrad"])
    np.add.at(G["I"], flat, (F["coef"][:, :, None] * F["uprime"][:, None, :]).reshape(flat.size, -1))
    G["Rel"] = F["GRel"]
    R = P["Rel"].shape[0]
    for j, k in enumerate(CAT_TABLES):
        np.add.at(G[k], cid.reshape(-1), F["kgrad"][:, j * R:(j + 1) * R])
    if 2 not in list(kinds):      # sigmas and mus are read by the 'substitute' kernel alone
        G["sigmas"] = G["mus"] = None
    if gmf:
        G["w"] = F["gw"].reshape(P["w"].shape)
        G["user_bias"] = G["item_bias"] = None
    else:
        G["w"] = None
        np.add.at(G["user_bias"].reshape(-1), uid, F["ubgrad"])
        np.add.at(G["item_bias"].reshape(-1), flat, g.reshape(-1))
    return G


def step(P, uid, iid, cid, iv, kinds, opt, lr, l2, lr_scale, gmf=False, states=None, step_no=1, dense=False):
    """one row-wise training step -> (loss, new parameters, new states {name: (m, v)}): rows of the batch only for U, I, the category
    tables and the biases; Rel and w dense.  (lr, l2) for U, betas, mus, sigmas, w; (lr_scale lr, l2) for I, Rel; (lr, 0) for the
    biases; a parameter without a gradient is left alone.  dense: torch.optim's semantics instead -- every row of every table with a
    gradient takes the step (weight decay and the moments reach rows outside the batch)."""
    loss_vec, gpred = bpr(scores(P, uid, iid, cid, iv, kinds, gmf))
    G = dense_grads(P, uid, iid, cid, iv, kinds, gpred, gmf)
    rows = {"U": uid, "I": iid, "betas": cid, "mus": cid, "sigmas": cid, "user_bias": uid, "item_bias": iid}
    new, st = {}, {}
    for k in PARAMS:
        m, v = (states or {}).get(k, (None, None))
        if G[k] is None:
            new[k], st[k] = np.asarray(P[k], np.float64), (m, v)
            continue
        W = np.asarray(P[k], np.float64)
        r = np.arange(W.shape[0]) if dense else rows.get(k, np.arange(W.shape[0]))
        klr, kl2 = (lr_scale * lr if k in ("I", "Rel") else lr), (0.0 if "bias" in k else l2)
        new[k], mk, vk = optimizer_rows(W, G[k], r, opt, klr, kl2, m, v, step_no)
        st[k] = (mk, vk)
    return loss_vec.mean(), new, st
