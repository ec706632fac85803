"""DirectAU's loss restated in float64 numpy with the closed-form gradient (models/general/DirectAU.py:54-88), the 1/S factor
applied after the pair sums as in csrc/directau.hip.  Shared by tests/test_directau_cpu.py and tests/test_gpu_directau.py."""
import numpy as np

EPS = 1e-12


def normalize(x):
    n = np.sqrt((x * x).sum(1))
    den = np.maximum(n, EPS)
    return x / den[:, None], den, n


def pair_sums(xh, block=4096):
    """S = sum_{i<j} e_ij, s_i = sum_{j != i} e_ij, M_i = sum_{j != i} e_ij x^_j, e_ij = exp(-2 |x^_i - x^_j|^2), row blocks of
    `block` so that large batches never hold B x B"""
    B = xh.shape[0]
    n = (xh * xh).sum(1)
    s = np.zeros(B)
    M = np.zeros_like(xh)
    for a in range(0, B, block):
        sl = slice(a, min(B, a + block))
        D = np.maximum(n[sl, None] + n[None, :] - 2.0 * xh[sl] @ xh.T, 0.0)
        E = np.exp(-2.0 * D)
        idx = np.arange(sl.start, sl.stop)
        E[idx - a, idx] = 0.0
        s[sl] = E.sum(1)
        M[sl] = E @ xh
    return 0.5 * s.sum(), s, M


def unnormalize(g, xh, den, n):
    """F.normalize's backward"""
    out = g / EPS
    big = n > EPS
    p = (xh * g).sum(1)
    out[big] = (g[big] - xh[big] * p[big, None]) / den[big, None]
    return out


def loss_and_row_grads(u, v, gamma):
    """u, v [B, d] rows -> (loss, align, unif_u, unif_i, grad_u [B, d], grad_v [B, d]) in float64"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    B = u.shape[0]
    uh, du, nu = normalize(u)
    vh, dv, nv = normalize(v)
    diff = uh - vh
    align = (diff * diff).sum(1).mean()
    gu_h, gv_h = 2.0 * diff / B, -2.0 * diff / B
    unif = []
    for xh, g in ((uh, gu_h), (vh, gv_h)):
        if B < 2:
            unif.append(np.nan)
            continue
        S, s, M = pair_sums(xh)
        unif.append(np.log(S / (B * (B - 1) / 2.0)))
        g -= (2.0 * gamma / S) * (s[:, None] * xh - M)
    loss = align + gamma * (unif[0] + unif[1]) / 2.0
    return loss, align, unif[0], unif[1], unnormalize(gu_h, uh, du, nu), unnormalize(gv_h, vh, dv, nv)


def table_grads(U, I, uid, iid, gamma):
    """(loss, GU, GI, prediction [B, 1]) for ids into the two tables"""
    uid, iid = np.asarray(uid).reshape(-1), np.asarray(iid).reshape(-1)
    u, v = np.asarray(U, np.float64)[uid], np.asarray(I, np.float64)[iid]
    loss, _, _, _, gu, gv = loss_and_row_grads(u, v, gamma)
    GU, GI = np.zeros(U.shape), np.zeros(I.shape)
    np.add.at(GU, uid, gu)
    np.add.at(GI, iid, gv)
    return loss, GU, GI, (u * v).sum(1)[:, None]
