"""float64 numpy restatement of SetRank's multihead attention block (reference models/reranker/SetRank.py:29-56 `MAB`: post-norm,
ReLU, eps 1e-5, nn.MultiheadAttention over query rows that are not the key rows, under a key-padding mask), forward and backward, the
induced block built from two of them (:67-80 `IMSAB`), and the random problems the GPU tests regenerate from their seeds.  Held to
torch's own modules in tests/test_setrank_cpu.py; the fp32 deviations of the reference's own `MAB` on the problems are stored in
tests/golden/setrank_mab_dev.npz by tests/golden/make_golden_setrank.py."""
import numpy as np

import prm_np
from prm_np import EPS, MASKS, TOL, WEIGHTS, _ln, _ln_bwd, make_mask, rel_err, stored_bound  # noqa: F401

GRAD_NAMES = ("dQs", "dKs") + tuple("d" + k for k in WEIGHTS)
TORCH_KEYS = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "norm1.weight", "norm1.bias",
              "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm2.weight", "norm2.bias")
M = 20                                                          # SetRank.py:68 m_clusters: the inducing points of every IMSAB block
LENGTHS = [1, 2, 15, 16, 17, 40, 48]


def admitted(nq, nk, d, dff):
    """the envelope's LDS rule (include/rechorus_hip.h, rc_setmab_check_shape), restated: bytes of the backward <= 160 KB"""
    NQ, NK = (nq + 15) // 16 * 16, (nk + 15) // 16 * 16
    floats = 3 * NQ * (d + 4) + NK * (d + 4) + max(NQ * (d + 4) + 2 * NK * (2 * d + 4), NQ * (2 * d + dff + 12)) + 64 * (NK + 4) + NK + NQ
    return 4 * floats <= 160 * 1024


# (B, nq, nk, d, H, d_ff, shared, masked, seed).  shared: ONE [nq, d] query source (MAB1 of an induced block: I against the list under
# the mask); otherwise per-list queries (MAB2: the list against h, no mask).  65 lists at (64, 4, 128) for every n; per-list queries
# under a mask at uneven tile counts and at one row each; every shape the envelope admits at 17 rows with 3 and 257 lists (the backward
# launches at most 256 workgroups: 257 lists make one workgroup walk a second list); one list alone.
SHAPES = [s for s in prm_np.SHAPES if admitted(M, 17, s[0], s[2]) and admitted(17, M, s[0], s[2])]
MAB_PROBLEMS = ([(65, M, n, 64, 4, 128, 1, 1, 400 + n) for n in LENGTHS]
                + [(65, n, M, 64, 4, 128, 0, 0, 500 + n) for n in LENGTHS]
                + [(65, nq, nk, 64, 4, 128, 0, 1, 600 + nq) for nq, nk in ((17, 33), (33, 17), (1, 1))]
                + [(B, M, 17, d, H, f, 1, 1, 700 + B + d + H) for (d, H, f) in SHAPES for B in (3, 257)]
                + [(B, 17, M, d, H, f, 0, 0, 800 + B + d + H) for (d, H, f) in SHAPES for B in (3, 257)]
                + [(1, M, 40, 64, 4, 128, 1, 1, 900), (1, 40, M, 64, 4, 128, 0, 0, 901)])
# per-list queries that ARE the keys, under the mask: the problems the self-attention kernels (engine.listenc_block_*) are run on too
SELF_PROBLEMS = [(65, 17, 17, 64, 4, 128, 0, 1, 950), (3, 40, 40, 32, 2, 128, 0, 1, 951)]


def mab_key(B, nq, nk, d, H, dff, shared, masked, seed):
    return "%d_%d_%d_%d_%d_%d_%d_%d_%d" % (B, nq, nk, d, H, dff, shared, masked, seed)


def random_mab(B, nq, nk, d, H, dff, shared, masked, seed, self_keys=False):
    """(Qs [B, nq, d] or [nq, d], Ks [B, nk, d], pad uint8 [B, nk] or None, the twelve weights, dY [B, nq, d]) in float32; the four
    mask kinds in turn over the lists; dY is non-zero everywhere.  in_proj is wide enough that the softmax rows are far from uniform."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s)
    Ks = f(B, nk, d)
    Qs = Ks.copy() if self_keys else (f(nq, d) if shared else f(B, nq, d))
    pad = np.stack([make_mask(rng, MASKS[(b + seed) % 4], nk) for b in range(B)]) if masked else None
    W = [1.5 * f(3 * d, d) / np.sqrt(d), 0.1 * f(3 * d), f(d, d) / np.sqrt(d), 0.1 * f(d), 1 + 0.3 * f(d), 0.1 * f(d),
         f(dff, d) / np.sqrt(d), 0.1 * f(dff), f(d, dff) / np.sqrt(dff), 0.1 * f(d), 1 + 0.3 * f(d), 0.1 * f(d)]
    dY = f(B, nq, d)
    return (Qs.astype(np.float32), Ks.astype(np.float32), pad, [w.astype(np.float32) for w in W], dY.astype(np.float32))


def problem(prob_id):
    return random_mab(*prob_id, self_keys=prob_id in SELF_PROBLEMS)


def mab_forward(Qs, Ks, pad, W, H, cache=False):
    """Y [B, nq, d]; Qs [B, nq, d], or [nq, d] for one source shared by every list"""
    Ks = np.asarray(Ks, np.float64)
    B, nk, d = Ks.shape
    Q = np.broadcast_to(np.asarray(Qs, np.float64), (B,) + np.shape(Qs)[-2:])
    nq = Q.shape[1]
    Win, bin_, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2 = [np.asarray(w, np.float64) for w in W]
    dk = d // H
    heads = lambda t, n: t.reshape(B, n, H, dk).transpose(0, 2, 1, 3)
    q = heads(Q @ Win[:d].T + bin_[:d], nq)
    k = heads(Ks @ Win[d:2 * d].T + bin_[d:2 * d], nk)
    v = heads(Ks @ Win[2 * d:].T + bin_[2 * d:], nk)
    S = q @ k.transpose(0, 1, 3, 2) / np.sqrt(dk)
    if pad is not None:
        S = np.where(np.asarray(pad).astype(bool)[:, None, None, :], -np.inf, S)
    S = S - S.max(-1, keepdims=True)
    P = np.exp(S)
    P = P / P.sum(-1, keepdims=True)
    O = (P @ v).transpose(0, 2, 1, 3).reshape(B, nq, d)
    X1, xh1, r1 = _ln(Q + O @ Wo.T + bo, g1, be1)
    Hd = np.maximum(X1 @ W1.T + b1, 0.0)
    Y, xh2, r2 = _ln(X1 + Hd @ W2.T + b2, g2, be2)
    if cache:
        return Y, dict(Q=Q, q=q, k=k, v=v, P=P, O=O, X1=X1, xh1=xh1, r1=r1, Hd=Hd, xh2=xh2, r2=r2)
    return Y


def mab_backward(dY, Qs, Ks, pad, W, H):
    """{dQs (Qs's shape: a shared source's is summed over the lists), dKs, dWin, ..., dbe2} in float64"""
    Ks, dY = np.asarray(Ks, np.float64), np.asarray(dY, np.float64)
    Win, bin_, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2 = [np.asarray(w, np.float64) for w in W]
    B, nk, d = Ks.shape
    nq, dk = dY.shape[1], d // H
    _, c = mab_forward(Qs, Ks, pad, W, H, cache=True)
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
    dO = (dz1 @ Wo).reshape(B, nq, H, dk).transpose(0, 2, 1, 3)
    P = c["P"]
    dV = P.transpose(0, 1, 3, 2) @ dO
    dP = dO @ c["v"].transpose(0, 1, 3, 2)
    dS = P * (dP - (P * dP).sum(-1, keepdims=True)) / np.sqrt(dk)
    flat = lambda t, n: t.transpose(0, 2, 1, 3).reshape(B, n, d)
    dq, dkv = flat(dS @ c["k"], nq), np.concatenate([flat(dS.transpose(0, 1, 3, 2) @ c["q"], nk), flat(dV, nk)], axis=-1)
    out["dWin"] = np.concatenate([s2(dq, c["Q"]), s2(dkv, Ks)])
    out["dbin"] = np.concatenate([dq.sum((0, 1)), dkv.sum((0, 1))])
    dQs = dz1 + dq @ Win[:d]
    out["dQs"] = dQs.sum(0) if np.ndim(Qs) == 2 else dQs
    out["dKs"] = dkv @ Win[d:]
    return out


def largest_probability(Qs, Ks, pad, W, H):
    """the largest attention probability of the least peaked list as a multiple of the uniform value 1 / valid keys, over the lists
    with more than two valid keys (every query row counts: queries are not masked), or None"""
    _, c = mab_forward(Qs, Ks, pad, W, H, cache=True)
    B, nk = np.shape(Ks)[:2]
    valid = np.full(B, nk) if pad is None else (np.asarray(pad) == 0).sum(1)
    pick = valid > 2
    if not pick.any():
        return None
    return float((c["P"][pick].max((1, 2, 3)) * valid[pick]).min())


def mask_matters(Qs, Ks, pad, W, H):
    """largest |Y without the mask - Y| / largest |Y|: what a kernel that ignored the mask would be off by"""
    return rel_err(mab_forward(Qs, Ks, None, W, H), mab_forward(Qs, Ks, pad, W, H))


class TorchMAB:
    """the block composed from torch's own modules (nn.MultiheadAttention, nn.LayerNorm, nn.Linear), batch-first, carrying the
    twelve weights: what the restatement is held to on the CPU and what tools/bench_setrank.py times the kernels against"""

    def __init__(self, W, H, dtype, device="cpu"):
        import torch
        nn = torch.nn
        d, dff = W[2].shape[0], W[6].shape[0]
        self.attn = nn.MultiheadAttention(d, H, dropout=0.0, batch_first=True)
        self.norm1, self.norm2 = nn.LayerNorm(d, eps=EPS), nn.LayerNorm(d, eps=EPS)
        self.linear1, self.linear2 = nn.Linear(d, dff), nn.Linear(dff, d)
        mods = {"attn": self.attn, "norm1": self.norm1, "norm2": self.norm2, "linear1": self.linear1, "linear2": self.linear2}
        self.params = []
        for key, w in zip(TORCH_KEYS, W):
            head, rest = key.split(".", 1)
            p = mods[head].get_parameter(rest)
            p.data = (w.detach().clone() if torch.is_tensor(w) else torch.from_numpy(np.array(w))).to(dtype)
            self.params.append(p)
        for m in mods.values():
            m.to(device=device, dtype=dtype).train()

    def __call__(self, Q, K, pad=None):
        import torch
        a = self.attn(Q, K, K, key_padding_mask=pad, need_weights=False)[0]
        x = self.norm1(Q + a)
        return self.norm2(x + self.linear2(torch.relu(self.linear1(x))))


def run_module(forward, params, prob, dtype):
    """(Y, {gradients}) as numpy of a torch block `forward(Q [B, nq, d], K [B, nk, d], bool pad | None)` whose twelve parameters are
    `params` (WEIGHTS order), on one random problem in `dtype`; a shared source is expanded over the lists and its gradient summed"""
    import torch
    Qs, Ks, pad, _, dY = prob
    q = torch.from_numpy(Qs).to(dtype).requires_grad_(True)
    k = torch.from_numpy(Ks).to(dtype).requires_grad_(True)
    for p in params:
        p.grad = None
    y = forward(q.expand(Ks.shape[0], -1, -1) if q.dim() == 2 else q, k, None if pad is None else torch.from_numpy(pad.astype(bool)))
    y.backward(torch.from_numpy(dY).to(dtype))
    grads = {"dQs": q.grad.numpy(), "dKs": k.grad.numpy()}
    grads.update({"d" + n: p.grad.numpy() for n, p in zip(WEIGHTS, params)})
    return y.detach().numpy(), grads


def deviation(got, prob, H):
    """{tensor: largest |difference| / largest |float64 entry|} of (Y, {gradients}) from this file's float64"""
    Qs, Ks, pad, W, dY = prob
    want = mab_backward(dY, Qs, Ks, pad, W, H)
    out = {"Y": rel_err(got[0], mab_forward(Qs, Ks, pad, W, H))}
    for name in GRAD_NAMES:
        out[name] = rel_err(got[1][name], want[name])
    return out


def imsab_forward(x, pad, I, w1, w2, H):
    """the induced block (SetRank.py:75-80): h = MAB1(I, x, x; pad), x' = MAB2(x, h, h) -> (h, x')"""
    h = mab_forward(I, x, pad, w1, H)
    return h, mab_forward(x, h, None, w2, H)


# ---- the model goldens (tests/golden/setrank_<case>.npz, from the reference's own SetRank) ---------------------------------------------
from prm_np import bound_for, grad_floor, keep, meta, ranker_vectors, raw_batch, stored  # noqa: E402,F401


def scale_state(state, g):
    """the parameters every golden computation starts from: the init stream (I0) with each tensor of scale_keys x its scale_vals
    factor (rFF0 / rFF1, every out_proj, every I, every in_proj_weight), one float32 product each, as the generator applied them"""
    out = {k: np.array(v, copy=True) for k, v in state.items()}
    for k, f in zip((str(k) for k in g["scale_keys"]), g["scale_vals"]):
        out[k] = (out[k] * np.float32(f)).astype(np.float32)
    return out


def key_bias(k, shape):
    """the key-bias third of an in_proj_bias: it shifts every score of a query row alike and the softmax does not see it, so its
    gradient is exactly zero in exact arithmetic and round-off in every precision -- a mask over it, None for any other tensor"""
    if not k.endswith("in_proj_bias"):
        return None
    exclude = np.zeros(shape, dtype=bool)
    exclude[shape[0] // 3:2 * (shape[0] // 3)] = True
    return exclude


def mab_names(g):
    return ("MAB1", "MAB2") if str(g["setrank_type"]) == "IMSAB" else ("MAB1",)


def golden_args(g, device):
    args = prm_np.golden_args(g, device)
    args.setrank_type = str(g["setrank_type"])
    return args


def golden_model(g, device, folder):
    """(the port's class built in `folder` -- the caller has made it the working directory -- over the golden's ranker fixture, on
    `device`, carrying the golden's scaled parameters; P0 as numpy).  Asserts the init stream on the way."""
    import os
    from types import SimpleNamespace
    import torch
    from models.reranker import SetRank
    m, ranker = meta(g), str(g["ranker"])
    d = os.path.join(str(folder), "model", ranker + "Impression")
    os.makedirs(d, exist_ok=True)
    torch.save({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("R/")}, os.path.join(d, "ranker.pt"))
    with open(os.path.join(d, ranker + ".yaml"), "w") as f:
        f.write(str(g["ranker_yaml"]))
    torch.manual_seed(m["seed"])
    # built on the CPU, as the golden was: the head's init re-draws the ranker's tables too, from the generator of the device they
    # are on, and only on the CPU is that the stream the head's own parameters come from
    model = (SetRank.SetRankSequential if m["seq"] else SetRank.SetRankGeneral)(golden_args(g, torch.device("cpu")),
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


def model_forward(g, i, P):
    """SetRank's forward (SetRank.py:126-156) on batch i in float64 from the parameters P -> ([every block's output], prediction)"""
    m = meta(g)
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    u_v, i_v = ranker_vectors(g, i)
    di = np.concatenate([P["i_embeddings.weight"][g["b%d/item_id" % i]], u_v, i_v], axis=2)
    x = di @ P["rFF0.weight"].T + P["rFF0.bias"] + P["ordinal_position_embedding.weight"][g["b%d/position" % i]]
    xs, pad = [], g["b%d/padding_mask" % i].astype(np.uint8)
    W = lambda l, mab: [P["encoder.%d.%s.%s" % (l, mab, k)] for k in TORCH_KEYS]
    for l in range(m["blocks"]):
        if str(g["setrank_type"]) == "IMSAB":
            x = imsab_forward(x, pad, P["encoder.%d.I" % l], W(l, "MAB1"), W(l, "MAB2"), m["H"])[1]
        else:
            x = mab_forward(x, x, pad, W(l, "MAB1"), m["H"])
        xs.append(x)
    return xs, (x @ P["rFF1.weight"].T + P["rFF1.bias"])[..., 0]
