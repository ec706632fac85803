"""ContraRec restated in float64 numpy (models/sequential/ContraRec.py): the BERT4Rec encoder (:250-276 with utils/layers.py
TransformerLayer :92-118, MultiHeadAttention :9-63), the context-target term (:99-101), the context-context term ContraLoss
(:142-193) and the gradients autograd derives from them, hand-derived.  Literal where it matters: padding rows take position row
0 and item row 0, are hidden as keys and multiplied by 0 at the end; the attention scores are shifted by their global maximum
and NaN becomes 0; ContraLoss keeps its two 1e-10 guards and the detached row maximum with the diagonal in it.  Shared by
tests/test_contrarec_cpu.py (pinned to every fixture there) and tests/test_gpu_contrarec.py (shapes beyond the fixtures).

P is a dict of arrays keyed by the state_dict names: i_embeddings.weight, encoder.p_embeddings.weight,
encoder.transformer_block.<l>.masked_attn_head.{q,k,v}_linear.{weight,bias}, ....layer_norm{1,2}.{weight,bias},
....linear{1,2}.{weight,bias}."""
import numpy as np

LN_EPS = 1e-5      # nn.LayerNorm's default
N_HEADS = 2        # BERT4RecEncoder(num_layers=2, num_heads=2), ContraRec.py:67
BLOCK = "encoder.transformer_block.%d."


def params64(P):
    return {k: np.asarray(v, np.float64) for k, v in P.items()}


def n_layers(P):
    k = 0
    while (BLOCK % k) + "linear1.weight" in P:
        k += 1
    return k


def _ln_fwd(z, g, b):
    mu = z.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((z - mu) ** 2).mean(-1, keepdims=True) + LN_EPS)
    xhat = (z - mu) * rstd
    return xhat * g + b, xhat, rstd


def _ln_bwd(dy, xhat, rstd, g):
    dxhat = dy * g
    d = xhat.shape[-1]
    dz = rstd * (dxhat - dxhat.mean(-1, keepdims=True) - xhat * (dxhat * xhat).mean(-1, keepdims=True))
    return dz, (dy * xhat).reshape(-1, d).sum(0), dy.reshape(-1, d).sum(0)


def encode(P, hist, lengths):
    """-> (hv [B, d], cache): the encoder output row at position length - 1 of every sequence"""
    P = params64(P)
    hist, lengths = np.asarray(hist), np.asarray(lengths)
    B, L = hist.shape
    d = P["i_embeddings.weight"].shape[1]
    dk = d // N_HEADS
    valid = np.arange(L)[None, :] < lengths[:, None]
    position = np.arange(L)[None, :] * valid                                   # :265
    x = P["i_embeddings.weight"][hist] + P["encoder.p_embeddings.weight"][position]
    cache = dict(valid=valid, position=position, layers=[])
    split = lambda t: t.reshape(B, L, N_HEADS, dk).transpose(0, 2, 1, 3)
    for l in range(n_layers(P)):
        pre = BLOCK % l
        a = pre + "masked_attn_head."
        q, k, v = (x @ P[a + n + "_linear.weight"].T + P[a + n + "_linear.bias"] for n in "qkv")
        qh, kh, vh = split(q), split(k), split(v)
        s = qh @ kh.transpose(0, 1, 3, 2) / dk ** 0.5
        s = np.where(valid[:, None, None, :], s, -np.inf)                       # the key-padding mask alone, :270
        with np.errstate(invalid="ignore"):
            e = np.exp(s - s.max())                                            # layers.py:60
            att = e / e.sum(-1, keepdims=True)
        att = np.where(np.isnan(att), 0.0, att)
        ctx = (att @ vh).transpose(0, 2, 1, 3).reshape(B, L, d)
        y1, xh1, rs1 = _ln_fwd(ctx + x, P[pre + "layer_norm1.weight"], P[pre + "layer_norm1.bias"])
        h = np.maximum(y1 @ P[pre + "linear1.weight"].T + P[pre + "linear1.bias"], 0)
        f = h @ P[pre + "linear2.weight"].T + P[pre + "linear2.bias"]
        x2, xh2, rs2 = _ln_fwd(f + y1, P[pre + "layer_norm2.weight"], P[pre + "layer_norm2.bias"])
        cache["layers"].append(dict(x=x, qh=qh, kh=kh, vh=vh, att=att, y1=y1, xh1=xh1, rs1=rs1, h=h, xh2=xh2, rs2=rs2))
        x = x2
    x = x * valid[:, :, None]                                                   # :273
    return x[np.arange(B), lengths - 1], cache                                  # :275


def encode_bwd(P, hist, lengths, cache, dhv, G):
    """adds the parameter gradients of sum(dhv * hv) to G (dense embedding gradients)"""
    P = params64(P)
    hist, lengths = np.asarray(hist), np.asarray(lengths)
    B, L = hist.shape
    d = P["i_embeddings.weight"].shape[1]
    dk = d // N_HEADS
    dx = np.zeros((B, L, d))
    dx[np.arange(B), lengths - 1] = dhv
    dx = dx * cache["valid"][:, :, None]
    merge = lambda t: t.transpose(0, 2, 1, 3).reshape(B, L, d)
    for l in range(n_layers(P) - 1, -1, -1):
        pre = BLOCK % l
        a = pre + "masked_attn_head."
        lc = cache["layers"][l]
        dz2, dg, db = _ln_bwd(dx, lc["xh2"], lc["rs2"], P[pre + "layer_norm2.weight"])
        G[pre + "layer_norm2.weight"] += dg
        G[pre + "layer_norm2.bias"] += db
        G[pre + "linear2.weight"] += dz2.reshape(-1, d).T @ lc["h"].reshape(-1, d)
        G[pre + "linear2.bias"] += dz2.reshape(-1, d).sum(0)
        dh = (dz2 @ P[pre + "linear2.weight"]) * (lc["h"] > 0)
        G[pre + "linear1.weight"] += dh.reshape(-1, d).T @ lc["y1"].reshape(-1, d)
        G[pre + "linear1.bias"] += dh.reshape(-1, d).sum(0)
        dy1 = dz2 + dh @ P[pre + "linear1.weight"]
        dz1, dg, db = _ln_bwd(dy1, lc["xh1"], lc["rs1"], P[pre + "layer_norm1.weight"])
        G[pre + "layer_norm1.weight"] += dg
        G[pre + "layer_norm1.bias"] += db
        dctx = dz1.reshape(B, L, N_HEADS, dk).transpose(0, 2, 1, 3)
        att, qh, kh, vh = lc["att"], lc["qh"], lc["kh"], lc["vh"]
        datt = dctx @ vh.transpose(0, 1, 3, 2)
        dvh = att.transpose(0, 1, 3, 2) @ dctx
        ds = att * (datt - (datt * att).sum(-1, keepdims=True)) / dk ** 0.5
        dq, dkk, dv = merge(ds @ kh), merge(ds.transpose(0, 1, 3, 2) @ qh), merge(dvh)
        dxn = dz1.copy()
        for nm, dt in (("q", dq), ("k", dkk), ("v", dv)):
            G[a + nm + "_linear.weight"] += dt.reshape(-1, d).T @ lc["x"].reshape(-1, d)
            G[a + nm + "_linear.bias"] += dt.reshape(-1, d).sum(0)
            dxn += dt @ P[a + nm + "_linear.weight"]
        dx = dxn
    np.add.at(G["i_embeddings.weight"], hist.reshape(-1), dx.reshape(-1, d))
    np.add.at(G["encoder.p_embeddings.weight"], cache["position"].reshape(-1), dx.reshape(-1, d))


def normalize(x):
    """F.normalize: x / max(|x|, 1e-12) per row -> (z, den)"""
    den = np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)
    return x / den, den


def normalize_bwd(dz, z, den):
    """past eps (g - z (z . g)) / |x|, else g / eps"""
    return np.where(den > 1e-12, (dz - z * (z * dz).sum(-1, keepdims=True)) / den, dz / 1e-12)


def contra_loss(va, vb, labels, t):
    """ContraLoss(F.normalize(stack([va, vb], 1)), labels) (:92,148-193) -> (loss, dva, dvb), all float64; labels None: InfoNCE"""
    va, vb = np.asarray(va, np.float64), np.asarray(vb, np.float64)
    B = va.shape[0]
    N = 2 * B
    z, den = normalize(np.concatenate([va, vb], 0))                             # view-major, :167
    lab = np.arange(B) if labels is None else np.asarray(labels)
    lab = np.concatenate([lab, lab])
    off = ~np.eye(N, dtype=bool)
    pos = (lab[:, None] == lab[None, :]) & off
    l = z @ z.T / t
    m = l.max(1, keepdims=True)                                                 # detached, diagonal included (:172-173)
    e = np.exp(l - m) * off
    D = e.sum(1, keepdims=True) + 1e-10
    Pn = pos.sum(1, keepdims=True).astype(np.float64)
    log_prob = l - m - np.log(D)
    loss = float((-t * (pos * log_prob).sum(1) / (Pn[:, 0] + 1e-10)).mean())
    dl = -(t / N) * (pos / (Pn + 1e-10) - (Pn / (Pn + 1e-10)) * (e / D))         # d loss / d l_rc
    dz = (dl + dl.T) @ z / t
    dx = normalize_bwd(dz, z, den)
    return loss, dx[:B], dx[B:]


def ctc_loss(pred, t):
    """:99-101 -> (loss, d loss / d pred); the global maximum is a shift of every row"""
    p = np.asarray(pred, np.float64) / t
    p = p - p.max()
    e = np.exp(p - p.max(1, keepdims=True))
    sm = e / e.sum(1, keepdims=True)
    B = p.shape[0]
    g = sm.copy()
    g[:, 0] -= 1.0
    return float(-t * np.log(sm[:, 0]).mean()), g / B


def train_step(P, hist, hist_a, hist_b, lengths, item_id, ctc_temp, ccc_temp, gamma):
    """the training forward, both losses and every parameter gradient ->
    dict(pred [B, C], features [B, 2, d] normalised, ctc, ccc, loss, G {key: gradient})"""
    P = params64(P)
    item_id = np.asarray(item_id)
    B = item_id.shape[0]
    I = P["i_embeddings.weight"]
    d = I.shape[1]
    stacked = np.concatenate([hist, hist_a, hist_b], 0)
    len3 = np.concatenate([lengths] * 3)
    hv, cache = encode(P, stacked, len3)
    his, va, vb = hv[:B], hv[B:2 * B], hv[2 * B:]
    iv = I[item_id]
    pred = (his[:, None, :] * iv).sum(-1)
    ctc, gpred = ctc_loss(pred, ctc_temp)
    ccc, dva, dvb = contra_loss(va, vb, item_id[:, 0], ccc_temp)
    G = {k: np.zeros(v.shape) for k, v in P.items()}
    np.add.at(G["i_embeddings.weight"], item_id.reshape(-1), (gpred[:, :, None] * his[:, None, :]).reshape(-1, d))
    dhv = np.concatenate([(gpred[:, :, None] * iv).sum(1), gamma * dva, gamma * dvb], 0)
    encode_bwd(P, stacked, len3, cache, dhv, G)
    feats = np.stack([normalize(va)[0], normalize(vb)[0]], 1)
    return dict(pred=pred, features=feats, ctc=ctc, ccc=ccc, loss=ctc + gamma * ccc, G=G)


def predict(P, hist, lengths, item_id):
    """the evaluation forward: prediction [B, C]"""
    P = params64(P)
    hv, _ = encode(P, hist, lengths)
    return (hv[:, None, :] * P["i_embeddings.weight"][np.asarray(item_id)]).sum(-1)


# ---- the forward-indexed position embedding and its table gradient (what rc_seq_embed_fwdpos_fwd / rc_seq_pos_grad_fwdpos compute) --

def embed_fwdpos(item_emb, pos_emb, hist, lengths):
    """X [B, L, d] = item rows + position rows (position id = index) on valid rows, 0 on the padding"""
    hist, lengths = np.asarray(hist), np.asarray(lengths)
    L = hist.shape[1]
    valid = np.arange(L)[None, :] < lengths[:, None]
    X = np.asarray(item_emb, np.float64)[hist] + np.asarray(pos_emb, np.float64)[np.arange(L)][None]
    return X * valid[:, :, None]


def pos_grad_fwdpos(dX, lengths, n_pos):
    """[n_pos, d]: row p = sum_b dX[b, p] over the sequences with len_b > p"""
    dX, lengths = np.asarray(dX, np.float64), np.asarray(lengths)
    B, L, d = dX.shape
    valid = np.arange(L)[None, :] < lengths[:, None]
    out = np.zeros((n_pos, d))
    out[:L] = (dX * valid[:, :, None]).sum(0)
    return out


def load_case(path):
    """a contrarec_*.npz case with its _grads / _after parts merged into one dict"""
    out = {}
    for part in ("", "_grads", "_after"):
        with np.load(path[:-4] + part + ".npz", allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    return out
