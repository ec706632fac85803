"""float64 numpy restatement of the list encoder block (reference models/reranker/PRM.py:64,90-92: nn.TransformerEncoderLayer(d, H,
d_ff, dropout=0), post-norm, ReLU, eps 1e-5, under a key-padding mask), forward and backward, and the random block problems the GPU
tests regenerate from their seeds.  Held to torch's own module in tests/test_prm_cpu.py; the fp32 deviations of the problems are stored
in tests/golden/prm_layer_dev.npz by tests/golden/make_golden_prm.py."""
import numpy as np

TOL = 2e-5
EPS = 1e-5
WEIGHTS = ("Win", "bin", "Wo", "bo", "g1", "be1", "W1", "b1", "W2", "b2", "g2", "be2")      # engine.LISTENC_WEIGHTS
GRAD_NAMES = ("dX",) + tuple("d" + k for k in WEIGHTS)
TORCH_KEYS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
              "norm1.weight", "norm1.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm2.weight",
              "norm2.bias")                                                                 # the same twelve, by state_dict key
MASKS = ("random", "one", "all", "two")

SHAPES = [(16, 1, 16), (32, 2, 128), (64, 4, 128), (128, 4, 256), (64, 16, 128)]           # (d, H, d_ff)
LENGTHS = [1, 2, 15, 16, 17, 40, 64]
# (B, n, d, H, d_ff, seed): every n at (64, 4, 128) with 65 lists; every shape at n = 17 with 3 and 257 lists (the backward launches at
# most 256 workgroups of one list per pass: 257 lists make one workgroup walk a second list); one list alone
LAYER_PROBLEMS = ([(65, n, 64, 4, 128, 100 + n) for n in LENGTHS]
                  + [(B, 17, d, H, f, 200 + B + d + H) for (d, H, f) in SHAPES for B in (3, 257)]
                  + [(1, 40, 64, 4, 128, 300)])


def layer_key(B, n, d, H, dff, seed):
    return "%d_%d_%d_%d_%d_%d" % (B, n, d, H, dff, seed)


def rel_err(got, want, floor=0.0):
    """largest |difference| / largest |reference entry| (the project's measure)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(float(np.abs(want).max()), floor, 1e-300))


def stored_bound(devs, key):
    """(bound, why) from a stored fp32 deviation: the larger of 2e-5 and 4 x the reference's own deviation for that tensor"""
    dev = float(devs[key])
    return (TOL, "the cap") if 4 * dev <= TOL else (4 * dev, "4 x the stored fp32 deviation %.2e" % dev)


def bound_for(g, key):
    return stored_bound(g, "dev/" + key)


def make_mask(rng, kind, n):
    """uint8 [n], 1 = padded slot, at least one valid slot"""
    pad = np.zeros(n, np.uint8)
    if kind == "random":
        pad = (rng.random(n) < 0.3).astype(np.uint8)
        pad[rng.integers(0, n)] = 0
    elif kind == "one":
        pad[:] = 1
        pad[rng.integers(0, n)] = 0
    elif kind == "two" and n >= 2:      # [valid positives | pad | valid negatives | pad]
        npos = (n + 1) // 2
        vp, vn = rng.integers(1, npos + 1), rng.integers(0, n - npos + 1)
        pad[vp:npos] = 1
        pad[npos + vn:] = 1
    return pad


def random_block(B, n, d, H, dff, seed):
    """(X [B, n, d], pad [B, n], the twelve weights, dY [B, n, d]) in float32; the four mask kinds in turn over the lists; dY is
    non-zero on padded slots too.  in_proj is wide enough that the softmax rows are far from uniform."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s)
    X = f(B, n, d)
    pad = np.stack([make_mask(rng, MASKS[(b + seed) % 4], n) for b in range(B)])
    W = [1.5 * f(3 * d, d) / np.sqrt(d), 0.1 * f(3 * d), f(d, d) / np.sqrt(d), 0.1 * f(d), 1 + 0.3 * f(d), 0.1 * f(d),
         f(dff, d) / np.sqrt(d), 0.1 * f(dff), f(d, dff) / np.sqrt(dff), 0.1 * f(d), 1 + 0.3 * f(d), 0.1 * f(d)]
    dY = f(B, n, d)
    return (X.astype(np.float32), pad, [w.astype(np.float32) for w in W], dY.astype(np.float32))


def _ln(z, g, b):
    mu = z.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((z - mu) ** 2).mean(-1, keepdims=True) + EPS)
    xh = (z - mu) * rstd
    return xh * g + b, xh, rstd


def _ln_bwd(dy, xh, rstd, g):
    gdy = dy * g
    return rstd * (gdy - gdy.mean(-1, keepdims=True) - xh * (gdy * xh).mean(-1, keepdims=True))


def block_forward(X, pad, W, H, cache=False):
    X = np.asarray(X, np.float64)
    Win, bin_, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2 = [np.asarray(w, np.float64) for w in W]
    B, n, d = X.shape
    dk = d // H
    qkv = X @ Win.T + bin_
    q, k, v = (qkv[..., j * d:(j + 1) * d].reshape(B, n, H, dk).transpose(0, 2, 1, 3) for j in range(3))
    S = q @ k.transpose(0, 1, 3, 2) / np.sqrt(dk)
    S = np.where(np.asarray(pad).astype(bool)[:, None, None, :], -np.inf, S)
    S = S - S.max(-1, keepdims=True)
    P = np.exp(S)
    P = P / P.sum(-1, keepdims=True)
    O = (P @ v).transpose(0, 2, 1, 3).reshape(B, n, d)
    X1, xh1, r1 = _ln(X + O @ Wo.T + bo, g1, be1)
    Hd = np.maximum(X1 @ W1.T + b1, 0.0)
    Y, xh2, r2 = _ln(X1 + Hd @ W2.T + b2, g2, be2)
    if cache:
        return Y, dict(q=q, k=k, v=v, P=P, O=O, X1=X1, xh1=xh1, r1=r1, Hd=Hd, xh2=xh2, r2=r2)
    return Y


def block_backward(dY, X, pad, W, H):
    """{dX, dWin, ..., dbe2} in float64"""
    X, dY = np.asarray(X, np.float64), np.asarray(dY, np.float64)
    Win, bin_, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2 = [np.asarray(w, np.float64) for w in W]
    B, n, d = X.shape
    dk = d // H
    _, c = block_forward(X, pad, W, H, cache=True)
    s2 = lambda a, b: np.einsum("bni,bnj->ij", a, b)
    out = {"dg2": (dY * c["xh2"]).sum((0, 1)), "dbe2": dY.sum((0, 1))}
    dz2 = _ln_bwd(dY, c["xh2"], c["r2"], g2)
    out["dW2"], out["db2"] = s2(dz2, c["Hd"]), dz2.sum((0, 1))
    dH = (dz2 @ W2) * (c["Hd"] > 0)
    out["dW1"], out["db1"] = s2(dH, c["X1"]), dH.sum((0, 1))
    dX1 = dz2 + dH @ W1
    out["dg1"], out["dbe1"] = (dX1 * c["xh1"]).sum((0, 1)), dX1.sum((0, 1))
    dz1 = _ln_bwd(dX1, c["xh1"], c["r1"], g1)
    out["dWo"], out["dbo"] = s2(dz1, c["O"]), dz1.sum((0, 1))
    dO = (dz1 @ Wo).reshape(B, n, H, dk).transpose(0, 2, 1, 3)
    P = c["P"]
    dV = P.transpose(0, 1, 3, 2) @ dO
    dP = dO @ c["v"].transpose(0, 1, 3, 2)
    dS = P * (dP - (P * dP).sum(-1, keepdims=True)) / np.sqrt(dk)
    dQ, dK = dS @ c["k"], dS.transpose(0, 1, 3, 2) @ c["q"]
    dqkv = np.concatenate([t.transpose(0, 2, 1, 3).reshape(B, n, d) for t in (dQ, dK, dV)], axis=-1)
    out["dWin"], out["dbin"] = s2(dqkv, X), dqkv.sum((0, 1))
    out["dX"] = dz1 + dqkv @ Win
    return out


def torch_layer(W, H, dtype):
    """torch's own nn.TransformerEncoderLayer (what PRM.py:64 stacks) carrying the twelve weights, batch-first, in training mode"""
    import torch
    d, dff = W[2].shape[0], W[6].shape[0]
    layer = torch.nn.TransformerEncoderLayer(d_model=d, nhead=H, dim_feedforward=dff, dropout=0.0, batch_first=True)
    layer.load_state_dict({k: torch.from_numpy(np.asarray(w)) for k, w in zip(TORCH_KEYS, W)})
    return layer.to(dtype).train()


def torch_block(X, pad, W, H, dY, dtype):
    """(Y, {gradients}) of torch's module in `dtype`, as numpy"""
    import torch
    layer = torch_layer(W, H, dtype)
    x = torch.from_numpy(np.asarray(X)).to(dtype).requires_grad_(True)
    y = layer(x, src_key_padding_mask=torch.from_numpy(np.asarray(pad).astype(bool)))
    y.backward(torch.from_numpy(np.asarray(dY)).to(dtype))
    params = dict(layer.named_parameters())
    grads = {"dX": x.grad.numpy()}
    grads.update({"d" + k: params[t].grad.numpy() for k, t in zip(WEIGHTS, TORCH_KEYS)})
    return y.detach().numpy(), grads


def fp32_deviation(prob, H):
    """{tensor: deviation of torch's fp32 module from this file's float64} for one random block problem"""
    X, pad, W, dY = prob
    Y32, G32 = torch_block(X, pad, W, H, dY, __import__("torch").float32)
    want = block_backward(dY, X, pad, W, H)
    out = {"Y": rel_err(Y32, block_forward(X, pad, W, H))}
    for k in GRAD_NAMES:
        out[k] = rel_err(G32[k], want[k])
    return out


def largest_probability(X, pad, W, H):
    """(largest attention probability, 1 / valid keys of that list) over the lists with more than two valid keys, or None"""
    _, c = block_forward(X, pad, W, H, cache=True)
    valid = (np.asarray(pad) == 0).sum(1)
    pick = valid > 2
    if not pick.any():
        return None
    rows = (np.asarray(pad) == 0)[pick]
    best = (c["P"][pick] * rows[:, None, :, None]).max((1, 2, 3))        # over the valid queries
    return float((best * valid[pick]).min())                            # the least non-uniform list, as a multiple of uniform


# ---- the model goldens (tests/golden/prm_<case>.npz, from the reference's own PRM) --------------------------------------------------
def scale_state(state, g):
    """the parameters every golden computation starts from: the init stream (I0) with every block's in_proj_weight x in_scale[l] and
    out_proj.weight x out_scale[l], in float32 as the generator applied them (repeated x 1.5 steps are one exact product each)"""
    out = {k: np.array(v, copy=True) for k, v in state.items()}
    for k in ("rFF0.weight", "rFF1.weight"):
        out[k] = (out[k] * np.float32(g["ff_scale"])).astype(np.float32)
    for l, (si, so) in enumerate(zip(g["in_scale"], g["out_scale"])):
        w = out["encoder.%d.self_attn.in_proj_weight" % l]
        s = np.float32(1.0)
        while s < si:
            w = (w * np.float32(1.5)).astype(np.float32)
            s *= np.float32(1.5)
        out["encoder.%d.self_attn.in_proj_weight" % l] = w
        out["encoder.%d.self_attn.out_proj.weight" % l] = (out["encoder.%d.self_attn.out_proj.weight" % l] * np.float32(so)).astype(np.float32)
    return out


def meta(g):
    keys = ("n_users", "n_items", "emb", "hidden", "H", "blocks", "P", "N", "B", "seed", "seq", "history")
    return dict(zip(keys, (int(x) for x in g["meta"])))


BIG, SUB = 2048, 5      # gradients and updated parameters above BIG elements are stored as every SUB-th element (flat): the size limit


def keep(v):
    v = np.asarray(v)
    return v.reshape(-1)[::SUB].copy() if v.size > BIG else v.copy()


def stored(g, prefix, k, got):
    """(the golden's tensor, `got` cut down the same way)"""
    want, got = g[prefix + k], np.asarray(got)
    if got.size != want.size:
        got = got.reshape(-1)[::SUB]
    return want, got.reshape(want.shape)


def grad_floor(g):
    """1e-6 of the batch's largest gradient entry: gradients are compared no finer than that"""
    return 1e-6 * max(float(np.abs(g[k]).max()) for k in g if k.startswith("G/"))


def golden_args(g, device):
    from types import SimpleNamespace
    m, ranker = meta(g), str(g["ranker"])
    return SimpleNamespace(device=device, model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, loss_n="BPR", emb_size=m["emb"],
                           train_max_pos_item=m["P"], train_max_neg_item=m["N"], test_max_pos_item=m["P"], test_max_neg_item=m["N"],
                           ranker_name=ranker, ranker_config_file=ranker + ".yaml", ranker_model_file="ranker.pt", tuneranker=0,
                           n_blocks=m["blocks"], num_heads=m["H"], num_hidden_unit=m["hidden"], history_max=m["history"])


def golden_model(g, device, folder):
    """(the port's class built in `folder` -- the caller has made it the working directory -- over the golden's ranker fixture, on
    `device`, carrying the golden's scaled parameters; P0 as numpy).  Asserts the init stream on the way."""
    import os
    from types import SimpleNamespace
    import torch
    from models.reranker import PRM
    m, ranker = meta(g), str(g["ranker"])
    d = os.path.join(str(folder), "model", ranker + "Impression")
    os.makedirs(d, exist_ok=True)
    torch.save({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("R/")}, os.path.join(d, "ranker.pt"))
    with open(os.path.join(d, ranker + ".yaml"), "w") as f:
        f.write(str(g["ranker_yaml"]))
    torch.manual_seed(m["seed"])
    # built on the CPU, as the golden was: the head's init re-draws the ranker's tables too, from the generator of the device they
    # are on, and only on the CPU is that the stream the head's own parameters come from
    model = (PRM.PRMSequential if m["seq"] else PRM.PRMGeneral)(golden_args(g, torch.device("cpu")),
                                                                 SimpleNamespace(n_users=m["n_users"], n_items=m["n_items"]))
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_keys"]]
    for k, v in sd.items():      # the init stream of the head, the checkpoint in the ranker
        want = g["R/" + k[len("ranker."):]] if k.startswith("ranker.") else g["I0/" + k]
        assert v.cpu().numpy().tobytes() == want.tobytes(), k
    P0 = scale_state({k: v.cpu().numpy() for k, v in sd.items()}, g)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in P0.items()})
    model.device = model.ranker.device = device
    return model.to(device), P0


def raw_batch(g, i, device):
    """batch i as the base Datasets collate it, before the ranker runs"""
    import torch
    keys = ("user_id", "item_id", "pos_num", "neg_num", "history_items", "lengths")
    return {k: torch.from_numpy(g["b%d/%s" % (i, k)]).to(device) for k in keys if "b%d/%s" % (i, k) in g}


def ranker_vectors(g, i):
    """(u_v, i_v) [B, n, ranker emb] of batch i: BPRMF's are two gathers from the fixture's tables; SASRec's come stored (small cases)"""
    if not meta(g)["seq"]:
        items = g["b%d/item_id" % i]
        u = g["R/u_embeddings.weight"][g["b%d/user_id" % i]]
        return np.repeat(u[:, None, :], items.shape[1], axis=1), g["R/i_embeddings.weight"][items]
    u, v = g["b%d/u_v" % i], g["b%d/i_v" % i]
    assert u.ndim == 3, "stored cut down: not a small case"
    return u, v


def model_forward(g, i, P):
    """PRM's forward (PRM.py:69-97) on batch i in float64 from the parameters P -> ([every block's output [B, n, hidden]], prediction)"""
    m = meta(g)
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    u_v, i_v = ranker_vectors(g, i)
    di = np.concatenate([P["i_embeddings.weight"][g["b%d/item_id" % i]], u_v, i_v], axis=2)
    x = (di + P["ordinal_position_embedding.weight"][g["b%d/position" % i]]) @ P["rFF0.weight"].T + P["rFF0.bias"]
    xs, pad = [], g["b%d/padding_mask" % i].astype(np.uint8)
    for l in range(m["blocks"]):
        x = block_forward(x, pad, [P["encoder.%d.%s" % (l, k)] for k in TORCH_KEYS], m["H"])
        xs.append(x)
    return xs, (x @ P["rFF1.weight"].T + P["rFF1.bias"])[..., 0]
