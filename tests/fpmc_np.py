"""FPMC in float64 numpy, written from the formulas (not from any kernel): the two-term score, GeneralModel.loss, the gradients
to the scores, to the per-tuple query rows and to the four tables, and one optimizer step on the rows of the batch.

    pred[b, c] = <UI[uid[b]], IU[iid[b, c]]> + <LI[lid[b]], IL[iid[b, c]]>
    P[b]       = sum_{k >= 1} softmax(pred[b, 1:])_k * sigmoid(pred[b, 0] - pred[b, k]),   loss = mean_b -log(clamp(P[b]))

tests/test_fpmc_cpu.py pins this file to the reference's own numbers (tests/golden/fpmc_*.npz); the GPU tests then hold the
kernels to it on shapes the goldens do not have."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_CASES = ("fpmc_d16_sgd_b1_k1", "fpmc_d32_sgd_b160_k4", "fpmc_d64_adam_b77_k99", "fpmc_d128_adagrad_b33_k9")
TABLES = ("UI", "LI", "IU", "IL")      # the engine's argument order


def golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


def f64(*xs):
    return [np.asarray(x, dtype=np.float64) for x in xs]


def scores(UI, LI, IU, IL, uid, lid, iid):
    UI, LI, IU, IL = f64(UI, LI, IU, IL)
    return np.einsum("bd,bcd->bc", UI[uid], IU[iid]) + np.einsum("bd,bcd->bc", LI[lid], IL[iid])


def bpr(pred, inv_b=None):
    """-> (loss_vec [B], gpred [B, C] = d(inv_b * sum loss_vec) / d pred); the clamp bounds are the fp32 ones (1 - 1e-8 rounds to 1)"""
    pred = np.asarray(pred, dtype=np.float64)
    B = pred.shape[0]
    inv_b = 1.0 / B if inv_b is None else inv_b
    pos, neg = pred[:, :1], pred[:, 1:]
    e = np.exp(neg - neg.max(axis=1, keepdims=True))
    w = e / e.sum(axis=1, keepdims=True)
    s = 1.0 / (1.0 + np.exp(-(pos - neg)))
    P = (w * s).sum(axis=1)
    Pc = np.clip(P, 1e-8, 1.0)
    loss_vec = -np.log(Pc)
    dLdP = np.where((P >= 1e-8) & (P <= 1.0), -inv_b / Pc, 0.0)
    gpred = np.empty_like(pred)
    gpred[:, 0] = dLdP * (w * s * (1.0 - s)).sum(axis=1)
    gpred[:, 1:] = dLdP[:, None] * w * ((s - P[:, None]) - s * (1.0 - s))
    return loss_vec, gpred


def query_grads(IU, IL, iid, gpred):
    """ugrad[b] = sum_c g[b, c] IU[iid[b, c]], lgrad[b] = sum_c g[b, c] IL[iid[b, c]]"""
    IU, IL, gpred = f64(IU, IL, gpred)
    return np.einsum("bc,bcd->bd", gpred, IU[iid]), np.einsum("bc,bcd->bd", gpred, IL[iid])


def dense_grads(UI, LI, IU, IL, uid, lid, iid, gpred):
    """the four dense table gradients, in TABLES order"""
    UI, LI, IU, IL, gpred = f64(UI, LI, IU, IL, gpred)
    ugrad, lgrad = query_grads(IU, IL, iid, gpred)
    GUI, GLI, GIU, GIL = (np.zeros_like(t) for t in (UI, LI, IU, IL))
    np.add.at(GUI, uid, ugrad)
    np.add.at(GLI, lid, lgrad)
    np.add.at(GIU, iid.reshape(-1), (gpred[:, :, None] * UI[uid][:, None, :]).reshape(-1, UI.shape[1]))
    np.add.at(GIL, iid.reshape(-1), (gpred[:, :, None] * LI[lid][:, None, :]).reshape(-1, LI.shape[1]))
    return GUI, GLI, GIU, GIL


def optimizer_rows(W, G, rows, opt, lr, l2, m=None, v=None, step=1, beta1=0.9, beta2=0.999, eps=None):
    """one torch.optim step (sgd / adam / adagrad, single-tensor formulas) on `rows` of W only -> (W, m, v) as new float64 arrays"""
    W, G = f64(W, G)
    W = W.copy()
    m = np.zeros_like(W) if m is None else np.asarray(m, np.float64).copy()
    v = np.zeros_like(W) if v is None else np.asarray(v, np.float64).copy()
    r = np.unique(np.asarray(rows).reshape(-1))
    g = G[r] + l2 * W[r]
    if opt == "SGD":
        W[r] -= lr * g
    elif opt == "Adam":
        eps = 1e-8 if eps is None else eps
        m[r] += (1 - beta1) * (g - m[r])
        v[r] = beta2 * v[r] + (1 - beta2) * g * g
        denom = np.sqrt(v[r]) / np.sqrt(1 - beta2 ** step) + eps
        W[r] -= lr / (1 - beta1 ** step) * m[r] / denom
    elif opt == "Adagrad":
        eps = 1e-10 if eps is None else eps
        m[r] += g * g
        W[r] -= lr * g / (np.sqrt(m[r]) + eps)
    else:
        raise ValueError(opt)
    return W, m, v


def step(tables, uid, lid, iid, opt, lr, l2, states=None, step_no=1):
    """one row-wise training step from `tables` (dict over TABLES) -> (loss, new tables, new states {name: (m, v)})"""
    T = [tables[k] for k in TABLES]
    loss_vec, gpred = bpr(scores(*T, uid, lid, iid))
    G = dict(zip(TABLES, dense_grads(*T, uid, lid, iid, gpred)))
    rows = {"UI": uid, "LI": lid, "IU": iid, "IL": iid}
    new, st = {}, {}
    for k in TABLES:
        m, v = (states or {}).get(k, (None, None))
        new[k], mk, vk = optimizer_rows(tables[k], G[k], rows[k], opt, lr, l2, m, v, step_no)
        st[k] = (mk, vk)
    return loss_vec.mean(), new, st


def ranks(pred):
    """rank of column 0 among the candidates, as BaseRunner.evaluate_method counts it: the number of scores >= the target's (itself
    included, ties against it)"""
    pred = np.asarray(pred)
    return (pred >= pred[:, :1]).sum(axis=1)
