"""CFKG in float64 numpy, written from the formulas (not from any kernel): the translation-distance score, MarginRankingLoss on the
quadruple feed, the gradients to the two tables and one optimizer step (entity rows of the batch only, the relation table densely).

    pred[b, c] = -|E[head[b, c]] + R[rel[b, c]] - E[tail[b, c]]|^2
    training feed, C = 4: head = (h, h, h, h'), tail = (t, t, t', t), one relation r per row
    a = h + r - t, b = h + r - t', c = h' + r - t, x1 = margin + |a|^2 - |b|^2, x2 = margin + |a|^2 - |c|^2, s = [x >= 0]
    loss = (1 / 2B) sum_b (s1 x1 + s2 x2)                 (at a tie the gradient passes: clamp_min(0)'s backward mask is >=)
    with w = 1 / B:  g_h = w ((s1 + s2) a - s1 b), g_t = w (-(s1 + s2) a + s2 c), g_t' = w s1 b, g_h' = -w s2 c,
                     g_r = w ((s1 + s2) a - s1 b - s2 c)

tests/test_cfkg_cpu.py pins this file to the reference's own numbers (tests/golden/cfkg_*.npz); the GPU tests then hold the kernels
to it on shapes the goldens do not have."""
import numpy as np

from fpmc_np import optimizer_rows, ranks  # noqa: F401  (the optimizers are the same arithmetic)

GOLDEN_CASES = ("cfkg_d128_adagrad_b33_r8_m05", "cfkg_d16_sgd_b1_r1_m0", "cfkg_d32_sgd_b160_r4_m1", "cfkg_d64_adam_b77_r4_m0")
STATE_KEYS = {"E": "e_embeddings.weight", "R": "r_embeddings.weight"}


def scores(E, R, head, tail, rel):
    E, R = np.asarray(E, np.float64), np.asarray(R, np.float64)
    v = E[head] + R[rel] - E[tail]
    return -(v * v).sum(-1)


def quad(head, tail, rel):
    """the five id columns (h, t, hn, tn, r) of a [B, 4] training feed"""
    return head[:, 0], tail[:, 0], head[:, 3], tail[:, 2], rel[:, 0]


def hinge(pred, margin):
    """MarginRankingLoss(margin) over the pairs (column 0, column 2), (column 1, column 3) of pred [B, 4]
    -> (loss, loss_vec [B] with loss = mean(loss_vec), x [B, 2], gpred [B, 4] = d loss / d pred)"""
    pred = np.asarray(pred, np.float64)
    B = pred.shape[0]
    x = margin - pred[:, :2] + pred[:, 2:]
    s = (x >= 0).astype(np.float64)
    loss_vec = 0.5 * (s * x).sum(axis=1)
    gpred = np.concatenate([-s, s], axis=1) / (2.0 * B)
    return loss_vec.mean(), loss_vec, x, gpred


def front(E, R, head, tail, rel, margin, inv_b=None):
    """what rc_cfkg_fwd_bwd leaves: (pred [B, 4], loss_vec [B], grows [B, 4, d] for (h, t, hn, tn), GR [n_rel, d])"""
    E, R = np.asarray(E, np.float64), np.asarray(R, np.float64)
    h, t, hn, tn, r = quad(head, tail, rel)
    w = 1.0 / len(h) if inv_b is None else inv_b
    a, b, c = E[h] + R[r] - E[t], E[h] + R[r] - E[tn], E[hn] + R[r] - E[t]
    na, nb, nc = (a * a).sum(-1), (b * b).sum(-1), (c * c).sum(-1)
    x1, x2 = margin + na - nb, margin + na - nc
    s1, s2 = (x1 >= 0).astype(np.float64)[:, None], (x2 >= 0).astype(np.float64)[:, None]
    gh, gt = w * ((s1 + s2) * a - s1 * b), w * (-(s1 + s2) * a + s2 * c)
    gtn, ghn = w * s1 * b, -w * s2 * c
    gr = w * ((s1 + s2) * a - s1 * b - s2 * c)
    GR = np.zeros_like(R)
    np.add.at(GR, r, gr)
    pred = np.stack([-na, -na, -nb, -nc], axis=1)
    loss_vec = 0.5 * (s1[:, 0] * x1 + s2[:, 0] * x2)
    return pred, loss_vec, np.stack([gh, gt, ghn, gtn], axis=1), GR


def dense_grads(E, R, head, tail, rel, gpred):
    """(GE, GR) of an arbitrary loss with d loss / d pred = gpred, any [B, C]"""
    E, R = np.asarray(E, np.float64), np.asarray(R, np.float64)
    g = -2.0 * np.asarray(gpred, np.float64)[..., None] * (E[head] + R[rel] - E[tail])
    g = g.reshape(-1, E.shape[1])
    GE, GR = np.zeros_like(E), np.zeros_like(R)
    np.add.at(GE, head.reshape(-1), g)
    np.add.at(GE, tail.reshape(-1), -g)
    np.add.at(GR, rel.reshape(-1), g)
    return GE, GR


def step(E, R, head, tail, rel, margin, opt, lr, l2, states=None, step_no=1):
    """one training step of engine.CfkgTrainer's semantics -> (loss, E1, R1, states {name: (m, v)}): E on the rows of the batch only,
    R on every row (torch.optim's dense step)"""
    pred, loss_vec, grows, GR = front(E, R, head, tail, rel, margin)
    h, t, hn, tn, _ = quad(head, tail, rel)
    ids = np.stack([h, t, hn, tn], axis=1).reshape(-1)
    GE = np.zeros((np.shape(E)[0], np.shape(E)[1]))
    np.add.at(GE, ids, grows.reshape(len(ids), -1))
    st = states or {}
    E1, mE, vE = optimizer_rows(E, GE, ids, opt, lr, l2, *st.get("E", (None, None)), step_no)
    R1, mR, vR = optimizer_rows(R, GR, np.arange(np.shape(R)[0]), opt, lr, l2, *st.get("R", (None, None)), step_no)
    return loss_vec.mean(), E1, R1, {"E": (mE, vE), "R": (mR, vR)}
