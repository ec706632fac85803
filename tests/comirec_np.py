"""ComiRec's forward, hard selection and hand-derived backward restated in float64 numpy (models/sequential/ComiRec.py:57-93),
literally: the softmax subtracts the batch-wide maximum and NaN rows become 0, as the reference writes it.  Shared by
tests/test_comirec_cpu.py and tests/test_gpu_comirec.py.

P is a dict of float64 arrays: I [n_items, d], Pos [n_pos, d] or None (--add_pos 0), W1 [A, d], b1 [A], W2 [K, A], b2 [K]."""
import numpy as np

KEYS = ("I", "Pos", "W1", "b1", "W2", "b2")


def params64(P):
    return {k: (None if P.get(k) is None else np.asarray(P[k], np.float64)) for k in KEYS}


def forward(P, hist, lengths):
    """-> dict(valid [B, L], h, x [B, L, d], t [B, L, A], a [B, K, L], interests [B, K, d])"""
    P = params64(P)
    hist, lengths = np.asarray(hist), np.asarray(lengths)
    B, L = hist.shape
    valid = hist > 0
    h = P["I"][hist]
    x = h
    if P["Pos"] is not None:
        position = (lengths[:, None] - np.arange(L)[None, :]) * valid
        x = h + P["Pos"][position]
    t = np.tanh(x @ P["W1"].T + P["b1"])
    s = t @ P["W2"].T + P["b2"]                                   # [B, L, K]
    s = np.where(valid[:, :, None], s, -np.inf).transpose(0, 2, 1)   # [B, K, L]
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.exp(s - s.max())
        a = e / e.sum(-1, keepdims=True)
    a = np.where(np.isnan(a), 0.0, a)
    interests = np.einsum("bkl,bld->bkd", a, h)
    return dict(valid=valid, h=h, x=x, t=t, a=a, interests=interests)


def target_pred(interests, I, target):
    """[B, K]: every interest against the item of candidate column 0"""
    return np.einsum("bkd,bd->bk", interests, np.asarray(I, np.float64)[np.asarray(target)])


def top2_gap(tp):
    """best minus second-best target_pred per row (0 with a single interest)"""
    if tp.shape[1] < 2:
        return np.zeros(tp.shape[0])
    srt = np.sort(tp, axis=1)
    return srt[:, -1] - srt[:, -2]


def train_forward(P, hist, lengths, item_id, sel=None):
    """the training phase -> (fwd dict, sel [B], user [B, d], prediction [B, C]); sel given: imposed instead of the argmax"""
    f = forward(P, hist, lengths)
    I = np.asarray(P["I"], np.float64)
    item_id = np.asarray(item_id)
    if sel is None:
        sel = target_pred(f["interests"], I, item_id[:, 0]).argmax(1)    # the first maximum: the lowest index on a tie
    sel = np.asarray(sel).astype(np.int64)
    user = f["interests"][np.arange(hist.shape[0]), sel]
    pred = np.einsum("bd,bcd->bc", user, I[item_id])
    return f, sel, user, pred


def eval_forward(P, hist, lengths, item_id):
    f = forward(P, hist, lengths)
    return np.einsum("bkd,bcd->bck", f["interests"], np.asarray(P["I"], np.float64)[np.asarray(item_id)]).max(-1)


def backward_user(P, hist, lengths, f, sel, d_user):
    """from d_user [B, d] -> (g_hist [B, L, d], g_x [B, L, d], dW1, db1, dW2, db2); no gradient through the selection"""
    P = params64(P)
    B, L = np.asarray(hist).shape
    K, A = P["W2"].shape
    rows = np.arange(B)
    a_sel = f["a"][rows, sel]                                        # [B, L]
    user = f["interests"][rows, sel]
    e = np.einsum("bd,bld->bl", d_user, f["h"])
    ds = a_sel * (e - (d_user * user).sum(1)[:, None])              # softmax backward of row sel; 0 at invalid positions
    W2s = P["W2"][sel]                                               # [B, A]
    dpre = ds[:, :, None] * W2s[:, None, :] * (1.0 - f["t"] ** 2)   # [B, L, A]
    g_x = dpre @ P["W1"]
    g_hist = a_sel[:, :, None] * d_user[:, None, :] + g_x
    dW1 = np.einsum("bla,bld->ad", dpre, f["x"])
    db1 = dpre.sum((0, 1))
    dW2, db2 = np.zeros((K, A)), np.zeros(K)
    np.add.at(dW2, sel, np.einsum("bl,bla->ba", ds, f["t"]))
    np.add.at(db2, sel, ds.sum(1))
    return g_hist, g_x, dW1, db1, dW2, db2


def bpr_loss_and_grad(pred):
    """GeneralModel.loss (models/BaseModel.py:182-185) and d loss / d pred in float64 (inside the clamp range)"""
    pos, neg = pred[:, 0], pred[:, 1:]
    w = np.exp(neg - neg.max(1, keepdims=True))
    w /= w.sum(1, keepdims=True)
    sg = 1.0 / (1.0 + np.exp(-(pos[:, None] - neg)))
    q = (w * sg).sum(1)
    B = pred.shape[0]
    dq = -1.0 / (B * q)
    g = np.zeros_like(pred)
    g[:, 0] = dq * (w * sg * (1.0 - sg)).sum(1)
    g[:, 1:] = dq[:, None] * (-w * sg * (1.0 - sg) + w * (sg - q[:, None]))
    return -np.log(q).mean(), g


def train_grads(P, hist, lengths, item_id, sel=None):
    """one training batch -> dict(loss, pred, sel, interests, grads {I, Pos, W1, b1, W2, b2}) with the BPR loss"""
    P = params64(P)
    hist, lengths, item_id = np.asarray(hist), np.asarray(lengths), np.asarray(item_id)
    f, sel, user, pred = train_forward(P, hist, lengths, item_id, sel)
    loss, g = bpr_loss_and_grad(pred)
    cand = P["I"][item_id]
    d_user = np.einsum("bc,bcd->bd", g, cand)
    g_hist, g_x, dW1, db1, dW2, db2 = backward_user(P, hist, lengths, f, sel, d_user)
    GI = np.zeros_like(P["I"])
    np.add.at(GI, item_id.reshape(-1), (g[:, :, None] * user[:, None, :]).reshape(-1, user.shape[1]))
    np.add.at(GI, hist.reshape(-1), g_hist.reshape(-1, user.shape[1]))
    grads = {"I": GI, "Pos": None, "W1": dW1, "b1": db1, "W2": dW2, "b2": db2}
    if P["Pos"] is not None:
        L = hist.shape[1]
        position = (lengths[:, None] - np.arange(L)[None, :]) * f["valid"]
        GP = np.zeros_like(P["Pos"])
        np.add.at(GP, position.reshape(-1), g_x.reshape(-1, user.shape[1]))
        grads["Pos"] = GP
    return dict(loss=loss, pred=pred, sel=sel, interests=f["interests"], grads=grads, fwd=f)


# ---- shared by the two test files: golden parameter names, the error measure, the round-off floors --------------------------------
TOL = 2e-5
PARAM_KEYS = {"I": "i_embeddings__weight", "Pos": "p_embeddings__weight", "W1": "W1__weight", "b1": "W1__bias", "W2": "W2__weight",
              "b2": "W2__bias"}


def golden_params(g, prefix="P0_"):
    return {k: (g[prefix + v] if prefix + v in g else None) for k, v in PARAM_KEYS.items()}


def rel_err(got, want, floor=0.0):
    """largest |got - want| over max(largest |want|, floor)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(float(np.abs(want).max()) if want.size else 0.0, floor, 1e-30)
    return float(np.abs(got - want).max()) / scale if want.size else 0.0


def grad_floor(grads, k):
    """the scale below which a gradient tensor of the attention path is round-off.  grads: {key: reference gradient or None}.
    With one valid position per sequence (L = 1, short histories) ds = a (e - c) is exactly 0 in the reference and a few ulp of
    <d_user, h> elsewhere, so Pos / W1 / b1 / W2 / b2 are compared no finer than 1e-6 of the batch's largest gradient entry; b2
    (exactly 0 in exact arithmetic at every shape: a softmax ignores a shift of its row) no finer than 1e-5 of W2's largest
    weight gradient"""
    if k == "I":
        return 0.0
    gmax = max(float(np.abs(v).max()) for v in grads.values() if v is not None)
    floor = 1e-6 * gmax / TOL
    return max(floor, 1e-5 * float(np.abs(grads["W2"]).max()) / TOL) if k == "b2" else floor


def golden_grads(g):
    return {k: (g["G_" + v] if "G_" + v in g else None) for k, v in PARAM_KEYS.items()}
