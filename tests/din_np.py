"""Float64 numpy restatement of DIN's attention unit (reference models/context_seq/DIN.py:63-95 with utils/layers.py MLP_Block:
Linear -> Sigmoid -> Dropout per hidden layer, then Linear(., 1)), forward and hand-derived backward, in the UNFOLDED form of the
reference: the first layer is a product with the concatenation [q, k, q - k, q * k].  Test infrastructure, not product code.

Shapes: q [N, H] with N = B * C (instance n uses batch row n // C), keys [B, L, H], lengths [B];
params = [(W_1 [A_1, 4H], b_1), ..., (W_k, b_k), (w_out [1, A_k] or [A_k], b_out [1])];
keeps = None or one keep-and-scale array [N * L, A_j] per hidden layer (oracle.mlp_oracle.dropout_keep with M = N * L)."""
import numpy as np

F64 = np.float64


def flat_params(params):
    """the one buffer rc_din_attention_fwd / bwd take: every layer's weight then bias, in definition order"""
    return np.concatenate([np.asarray(t, dtype=np.float32).reshape(-1) for pair in params for t in pair])


def split_flat(flat, H, widths):
    """inverse of flat_params -> [(W, b), ..., (w_out, b_out)]"""
    out, o, K = [], 0, 4 * H
    for A in list(widths) + [1]:
        W = flat[o:o + A * K].reshape(A, K)
        o += A * K
        out.append((W, flat[o:o + A]))
        o += A
        K = A
    assert o == flat.size
    return out


def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def concat_input(q, keys, n_cand):
    """[N, L, 4H]: what the reference materialises"""
    q = np.asarray(q, F64)
    k = np.repeat(np.asarray(keys, F64), n_cand, axis=0)          # [N, L, H]
    qq = np.broadcast_to(q[:, None, :], k.shape)
    return np.concatenate([qq, k, qq - k, qq * k], axis=-1), k


def first_layer_unfolded(q, keys, n_cand, W1, b1):
    x, _ = concat_input(q, keys, n_cand)
    return x @ np.asarray(W1, F64).T + np.asarray(b1, F64)


def first_layer_folded(q, keys, n_cand, W1, b1):
    """z_1 = (Wq + Wd) q + (Wk - Wd) k + Wp (q * k) + b_1 with W_1 = [Wq | Wk | Wd | Wp]: the q term per instance, the k term per
    (b, l), only the Wp term per (n, l) -- the form csrc/din.hip evaluates"""
    q, keys, W1 = np.asarray(q, F64), np.asarray(keys, F64), np.asarray(W1, F64)
    H = q.shape[1]
    Wq, Wk, Wd, Wp = (W1[:, i * H:(i + 1) * H] for i in range(4))
    zq = q @ (Wq + Wd).T + np.asarray(b1, F64)                     # [N, A]
    zk = keys @ (Wk - Wd).T                                       # [B, L, A]
    k = np.repeat(keys, n_cand, axis=0)
    zp = (q[:, None, :] * k) @ Wp.T                               # [N, L, A]
    return zp + np.repeat(zk, n_cand, axis=0) + zq[:, None, :]


def forward(q, keys, lengths, n_cand, params, keeps=None):
    """-> (out [N, H], att [N, L], cache)"""
    N, H = q.shape
    B, L, _ = keys.shape
    x, k = concat_input(q, keys, n_cand)
    valid = (np.arange(L)[None, :] < np.minimum(np.asarray(lengths), L)[:, None])      # [B, L]
    valid = np.repeat(valid, n_cand, axis=0)                                              # [N, L]
    k = np.where(valid[..., None], k, 0.0)           # padded positions are never read as valid
    x = np.where(valid[..., None], x, 0.0)
    hs, ss, h = [x], [], x
    for j, (W, b) in enumerate(params[:-1]):
        s = _sigmoid(h @ np.asarray(W, F64).T + np.asarray(b, F64))
        keep = np.ones_like(s) if keeps is None else np.asarray(keeps[j], F64).reshape(N, L, -1)
        h = s * keep
        ss.append((s, keep))
        hs.append(h)
    w_out, b_out = params[-1]
    score = h @ np.asarray(w_out, F64).reshape(-1) + float(np.asarray(b_out).reshape(-1)[0])
    att = np.where(valid, score, 0.0) / np.sqrt(H)
    out = np.einsum("nl,nlh->nh", att, k)
    return out, att, {"x": x, "k": k, "valid": valid, "hs": hs, "ss": ss, "att": att}


def backward(q, keys, lengths, n_cand, params, d_out, keeps=None):
    """-> (dq [N, H], dkeys [B, L, H], [(dW, db), ..., (dw_out, db_out)]) of sum(out * d_out)"""
    N, H = q.shape
    B, L, _ = keys.shape
    q = np.asarray(q, F64)
    d_out = np.asarray(d_out, F64)
    _, _, c = forward(q, keys, lengths, n_cand, params, keeps)
    k, valid = c["k"], c["valid"]
    dk = c["att"][..., None] * d_out[:, None, :]                                  # out = sum_l att k
    datt = np.einsum("nh,nlh->nl", d_out, k)
    dscore = np.where(valid, datt, 0.0) / np.sqrt(H)
    w_out = np.asarray(params[-1][0], F64).reshape(-1)
    grads = [(np.einsum("nl,nla->a", dscore, c["hs"][-1]).reshape(np.asarray(params[-1][0]).shape), np.array([dscore.sum()]))]
    dh = dscore[..., None] * w_out
    for j in range(len(params) - 2, -1, -1):
        s, keep = c["ss"][j]
        dz = dh * keep * s * (1.0 - s)
        W = np.asarray(params[j][0], F64)
        grads.append((np.einsum("nla,nlk->ak", dz, c["hs"][j]), dz.sum(axis=(0, 1))))
        dh = dz @ W
    grads.reverse()
    dx = np.where(valid[..., None], dh, 0.0)                                       # x was masked before the first layer
    dxq, dxk, dxd, dxp = (dx[..., i * H:(i + 1) * H] for i in range(4))
    dq = (dxq + dxd + dxp * k).sum(axis=1)
    dk = dk + dxk - dxd + dxp * q[:, None, :]
    dk = np.where(valid[..., None], dk, 0.0)
    dkeys = dk.reshape(B, n_cand, L, H).sum(axis=1)
    return dq, dkeys, grads


def flat_grads(grads):
    return np.concatenate([np.asarray(t, F64).reshape(-1) for pair in grads for t in pair])


def torch_reference(q, keys, lengths, n_cand, params, keeps=None):
    """DIN.attention / DIN.att_dnn's feed (models/context_seq/DIN.py:63-95, 148-156) in float64 torch ops, with explicit keep masks"""
    import torch
    N, H = q.shape
    L = keys.shape[1]
    k = keys.unsqueeze(1).repeat(1, n_cand, 1, 1).view(N, L, H)
    qq = q.repeat(1, L).view(N, L, H)
    h = torch.cat([qq, k, qq - k, qq * k], dim=-1)
    for j, (W, b) in enumerate(params[:-1]):
        h = torch.sigmoid(h @ W.T + b)
        if keeps is not None:
            h = h * keeps[j].view(N, L, -1)
    score = (h @ params[-1][0].reshape(-1, 1) + params[-1][1]).squeeze(-1)
    mask = torch.arange(L).view(1, -1) >= lengths.repeat_interleave(n_cand).unsqueeze(1)
    att = score.masked_fill(mask, 0.0) / (H ** 0.5)
    return torch.matmul(att.unsqueeze(1), k).squeeze(1), att
