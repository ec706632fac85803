"""float64 numpy restatement of BUIR (models/general/BUIR.py:66-110) for the tests: loss, the four gradients, the scoring identity
and the target update.  Closed forms only, no autograd.

  n(x) = x / max(|x|, eps);  pu = W uo + b, pi = W io + b;  loss = mean_b [4 - 2 <n(pu), n(it)> - 2 <n(pi), n(ut)>]
  d loss / d n(pu) = -2 g0 / B n(it), through the normalisation (g - x^ (x^ . g)) / |x| past eps, g / eps below;
  d uo = W^T g_pu, d io = W^T g_pi, dW = sum_b (g_pu uo^T + g_pi io^T), db = sum_b (g_pu + g_pi)
"""
import numpy as np

EPS = 1e-12


def normalize(x):
    """-> (x / max(|x|, eps), max(|x|, eps), |x|) per row"""
    n = np.sqrt((x * x).sum(-1, keepdims=True))
    den = np.maximum(n, EPS)
    return x / den, den, n


def unnormalize(g, xh, den, n):
    """F.normalize's backward: the gradient g w.r.t. x / max(|x|, eps) mapped to x"""
    past = n > EPS
    return np.where(past, (g - xh * (xh * g).sum(-1, keepdims=True)) / den, g / EPS)


def row_grads(uo, ut, io, it, W, b, g0=1.0):
    """rows [B, d] (float64) -> (loss, prediction [B, 1], d uo, d io, dW, db)"""
    B = uo.shape[0]
    pu, pi = uo @ W.T + b, io @ W.T + b
    pred = ((pi * uo).sum(-1) + (pu * io).sum(-1))[:, None]
    xu, du, nu = normalize(pu)
    xi, di, ni = normalize(pi)
    tu, ti = normalize(ut)[0], normalize(it)[0]
    loss = (4.0 - 2.0 * (xu * ti).sum(-1) - 2.0 * (xi * tu).sum(-1)).mean()
    c = -2.0 * g0 / B
    g_pu = unnormalize(c * ti, xu, du, nu)
    g_pi = unnormalize(c * tu, xi, di, ni)
    return loss, pred, g_pu @ W, g_pi @ W, g_pu.T @ uo + g_pi.T @ io, (g_pu + g_pi).sum(0)


def table_grads(UO, UT, IO, IT, W, b, uid, iid, g0=1.0):
    """tables (any float dtype), uid [B], iid [B] or [B, 1] -> (loss, prediction [B, 1], G_user_online, G_item_online, dW, db)"""
    f = lambda a: np.asarray(a, np.float64)
    uid, iid = np.asarray(uid).reshape(-1), np.asarray(iid).reshape(-1)
    UO, UT, IO, IT, W, b = (f(a) for a in (UO, UT, IO, IT, W, b))
    loss, pred, duo, dio, dW, db = row_grads(UO[uid], UT[uid], IO[iid], IT[iid], W, b, g0)
    GU, GI = np.zeros_like(UO), np.zeros_like(IO)
    np.add.at(GU, uid, duo)
    np.add.at(GI, iid, dio)
    return loss, pred, GU, GI, dW, db


def scores_reference_order(UO, IO, W, b, uid, iid):
    """prediction [B, C] as BUIR.py:78-79 writes it: <P(i_c), u> + <P(u), i_c>"""
    UO, IO, W, b = (np.asarray(a, np.float64) for a in (UO, IO, W, b))
    u, i = UO[uid], IO[iid]                                  # [B, d], [B, C, d]
    return ((i @ W.T + b) * u[:, None, :]).sum(-1) + ((u @ W.T + b)[:, None, :] * i).sum(-1)


def query(UO, W, b, uid):
    """q [B, d] = (W + W^T) u + b, c [B] = <b, u>: prediction[b, c] = <q_b, i_c> + c_b"""
    UO, W, b = (np.asarray(a, np.float64) for a in (UO, W, b))
    u = UO[uid]
    return u @ (W + W.T).T + b, u @ b


def scores(UO, IO, W, b, uid, iid):
    q, c = query(UO, W, b, uid)
    return (q[:, None, :] * np.asarray(IO, np.float64)[iid]).sum(-1) + c[:, None]


def ema(target, online, momentum):
    """target * m + online * (1 - m) as torch evaluates it on fp32 tensors with Python scalars: m and (1 - m, formed in double)
    rounded to fp32, the two products and the sum each rounded to fp32"""
    t, o = np.asarray(target, np.float32), np.asarray(online, np.float32)
    m, om = np.float32(momentum), np.float32(1.0 - momentum)
    return (t * m).astype(np.float32) + (o * om).astype(np.float32)
