"""Float64 restatement of FinalMLP (reference: models/context/FinalMLP.py) for the tests: the gated first layers and the bilinear
fusion with their backward passes (the ReLU / dropout mask is an ARGUMENT of the backward, so a test can hand over the mask the
kernel actually used), the whole model's forward, and the model file's classes built from a golden (whose torch path, in fp32 and
in float64, is what tests/test_finalmlp_cpu.py holds the goldens' gradients to)."""
import numpy as np

TOL = 2e-5          # the project's bound: |error| <= TOL * the tensor's largest entry


def rel_err(got, want, floor=0.0):
    """largest |got - want| over max(largest |want|, floor)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(float(np.abs(want).max()) if want.size else 0.0, floor, 1e-30)
    return float(np.abs(got - want).max()) / scale if want.size else 0.0


def bound_for(g, key):
    """(bound, why): 2e-5 of the largest entry; where the golden's stored fp32-vs-float64 deviation of the reference itself exceeds
    1e-5 for this tensor, twice that deviation"""
    k = "dev/" + key
    if k in g and float(g[k]) > 1e-5:
        return 2.0 * float(g[k]), "twice the reference's own fp32 deviation %.1e" % float(g[k])
    return TOL, "the cap"


def grad_floor(g):
    """the scale below which a gradient tensor is round-off (rel_err's floor), as tests/autoint_np.py sets it: a gradient that is
    exactly zero in exact arithmetic (under BPR whatever shifts every candidate of a row alike: the fusion's two biases) is compared
    no finer than 1e-6 of the batch's largest gradient entry"""
    top = max(float(np.abs(g[k]).max()) for k in g if k.startswith("G/"))
    return 1e-6 * top / TOL


def gate_rows(n_gate_rows, N, n_cand):
    """the gate row of every instance: 0 (one row), n // n_cand (one row per batch row) or n"""
    n = np.arange(N)
    if n_gate_rows == N and N > 1:
        return n
    if n_gate_rows == N // n_cand and N // n_cand > 1:
        return n // n_cand
    assert n_gate_rows == 1
    return np.zeros(N, dtype=np.int64)


def gate_values(Zin, Wg, bg, N, n_cand):
    rows = gate_rows(Zin.shape[0], N, n_cand)
    logits = Zin.astype(np.float64) @ Wg.astype(np.float64).T + bg.astype(np.float64)
    return (2.0 / (1.0 + np.exp(-logits)))[rows], rows


def gate_fwd(X, stream, n_cand):
    """-> (gate [N, D], pre-activation [N, H]) of stream = (Zin, Wg, bg, W, b), float64"""
    Zin, Wg, bg, W, b = [np.asarray(t, dtype=np.float64) for t in stream]
    X = np.asarray(X, dtype=np.float64)
    g, _ = gate_values(Zin, Wg, bg, X.shape[0], n_cand)
    return g, (X * g) @ W.T + b


def gate_bwd(X, stream, n_cand, mask, dA):
    """backward of A = mask * pre through one stream; mask [N, H] holds 0 or 1 / (1 - p) (ReLU and dropout together)
    -> (dX share, dZin, dWg, dbg, dW, db), float64"""
    Zin, Wg, bg, W, b = [np.asarray(t, dtype=np.float64) for t in stream]
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    g, rows = gate_values(Zin, Wg, bg, N, n_cand)
    dpre = np.asarray(dA, dtype=np.float64) * np.asarray(mask, dtype=np.float64)
    P = dpre @ W
    dX = P * g
    dz = P * X * g * (1.0 - 0.5 * g)
    dZin_rows = dz @ Wg
    dZin = np.zeros_like(Zin)
    np.add.at(dZin, rows, dZin_rows)
    dWg = dz.T @ Zin[rows]
    return dX, dZin, dWg, dz.sum(0), dpre.T @ (X * g), dpre.sum(0)


def fusion_fwd(x, y, w_xy, w_x, b_x, w_y, b_y, heads):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N, H1 = x.shape
    H2 = y.shape[1]
    W = np.asarray(w_xy, dtype=np.float64).reshape(heads, H1 // heads, H2 // heads)
    xh, yh = x.reshape(N, heads, H1 // heads), y.reshape(N, heads, H2 // heads)
    bil = np.einsum('nhi,hij,nhj->n', xh, W, yh)
    return x @ np.asarray(w_x, np.float64).reshape(-1) + y @ np.asarray(w_y, np.float64).reshape(-1) + float(np.asarray(b_x).reshape(-1)[0]) \
        + float(np.asarray(b_y).reshape(-1)[0]) + bil


def fusion_terms(x, y, w_xy, w_x, w_y, heads):
    """(linear terms without biases, bilinear term), float64"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N, H1 = x.shape
    H2 = y.shape[1]
    W = np.asarray(w_xy, dtype=np.float64).reshape(heads, H1 // heads, H2 // heads)
    bil = np.einsum('nhi,hij,nhj->n', x.reshape(N, heads, -1), W, y.reshape(N, heads, -1))
    return x @ np.asarray(w_x, np.float64).reshape(-1) + y @ np.asarray(w_y, np.float64).reshape(-1), bil


def fusion_bwd(x, y, w_xy, w_x, w_y, dout, heads):
    """-> (dx, dy, dw_xy (flat), dw_x, db_x, dw_y, db_y), float64"""
    x, y, dout = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(dout, dtype=np.float64)
    N, H1 = x.shape
    H2 = y.shape[1]
    W = np.asarray(w_xy, dtype=np.float64).reshape(heads, H1 // heads, H2 // heads)
    xh, yh = x.reshape(N, heads, H1 // heads), y.reshape(N, heads, H2 // heads)
    dx = dout[:, None] * (np.asarray(w_x, np.float64).reshape(1, -1) + np.einsum('hij,nhj->nhi', W, yh).reshape(N, H1))
    dy = dout[:, None] * (np.asarray(w_y, np.float64).reshape(1, -1) + np.einsum('nhi,hij->nhj', xh, W).reshape(N, H2))
    dW = np.einsum('n,nhi,nhj->hij', dout, xh, yh).reshape(-1)
    return dx, dy, dW, dout @ x, dout.sum(), dout @ y, dout.sum()


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


class Model64:
    """FinalMLP forward in float64 from a state_dict-like mapping of numpy arrays (keys as the reference's), dropout off.
    cfg: dict(context_features, fs1_context, fs2_context, use_fs, num_heads, ctr)"""

    def __init__(self, params, cfg):
        self.p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
        self.cfg = cfg

    def field_order(self):
        cf = self.cfg['context_features']
        return ['user_id'] + [f for f in cf if f == 'item_id' or f.startswith('i_')] + [f for f in cf if f.startswith('c_')]

    def _embed(self, key, f, values, n_cand):
        w = self.p[key]
        v = w[np.asarray(values)] if (f.endswith('_c') or f.endswith('_id')) else np.asarray(values, dtype=np.float64)[..., None] * w[:, 0]
        if v.ndim == 2:
            v = np.repeat(v[:, None, :], n_cand, axis=1)
        return v

    def _linears(self, prefix):
        ks = sorted({int(k.split('.')[-2]) for k in self.p if k.startswith(prefix + '.mlp.') and k.endswith('.weight')})
        return [(self.p[f'{prefix}.mlp.{k}.weight'], self.p[f'{prefix}.mlp.{k}.bias']) for k in ks]

    def flat_fields(self, feed):
        n_cand = np.asarray(feed['item_id']).shape[1]
        vs = [self._embed(f'embedding_dict.{f}.weight', f, feed[f], n_cand) for f in self.field_order()]
        return np.concatenate(vs, axis=-1)      # [B, C, F d]

    def gate_input(self, s, feed, B, n_cand):
        ctx = self.cfg[f'fs{s}_context']
        if not ctx:
            return np.repeat(self.p[f'fs_module.fs{s}_ctx_bias'][:, None, :], n_cand, axis=1).repeat(B, axis=0)
        parts = []
        for i, f in enumerate(ctx):
            key = f'fs_module.fs{s}_ctx_emb.{i}.weight'
            if f.endswith('_c'):
                v = self.p[key][np.asarray(feed[f])]
            else:
                v = np.asarray(feed[f], dtype=np.float64)[..., None] * self.p[key][:, 0] + self.p[f'fs_module.fs{s}_ctx_emb.{i}.bias']
            parts.append(np.repeat(v[:, None, :], n_cand, axis=1) if v.ndim == 2 else v)
        return np.concatenate(parts, axis=-1)

    def forward(self, feed):
        """-> dict(flat, gate1, gate2, A1, A2, x, y, prediction); the tensors [B, C, ...]"""
        flat = self.flat_fields(feed)
        B, C, D = flat.shape
        out = {'flat': flat}
        feats = []
        for s in (1, 2):
            if self.cfg['use_fs']:
                z = self.gate_input(s, feed, B, C)
                layers = self._linears(f'fs_module.fs{s}_gate')
                for W, b in layers[:-1]:
                    z = np.maximum(z @ W.T + b, 0.0)
                g = 2.0 * _sigmoid(z @ layers[-1][0].T + layers[-1][1])
                out[f'gate{s}'] = g
                feats.append(flat * g)
            else:
                feats.append(flat)
        streams = []
        for s, feat in zip((1, 2), feats):
            hcur = feat.reshape(B * C, D)
            for k, (W, b) in enumerate(self._linears(f'mlp{s}')):
                hcur = np.maximum(hcur @ W.T + b, 0.0)
                if k == 0:
                    out[f'A{s}'] = hcur.reshape(B, C, -1)
            streams.append(hcur)
        out['x'], out['y'] = streams
        pred = fusion_fwd(streams[0], streams[1], self.p['fusion_module.w_xy'], self.p['fusion_module.w_x.weight'],
                          self.p['fusion_module.w_x.bias'], self.p['fusion_module.w_y.weight'], self.p['fusion_module.w_y.bias'],
                          self.cfg['num_heads']).reshape(B, C)
        out['logit'] = pred
        out['prediction'] = _sigmoid(pred).reshape(-1) if self.cfg['ctr'] else pred
        return out


# ---- the model file around the goldens (torch is imported only here) ---------------------------------------------------------------
def config(g):
    import json
    return json.loads(str(g["config"]))


def state_keys(g):
    return [str(k) for k in g["state_keys"]]


def params(g, which="P0"):
    return {k: g[which + "/" + k] for k in state_keys(g)}


def batch(g, n):
    pre = "b%d/" % n
    return {k[len(pre):]: g[k] for k in g if k.startswith(pre)}


def model64(g, which="P0"):
    c = config(g)
    fl = c["flags"]
    return Model64(params(g, which), dict(context_features=c["context_features"], use_fs=fl["use_fs"], num_heads=fl["num_heads"], ctr=c["ctr"],
                                          fs1_context=[f for f in fl["fs1_context"].split(",") if f],
                                          fs2_context=[f for f in fl["fs2_context"].split(",") if f]))


def model_args(g, device, **override):
    from types import SimpleNamespace
    c = config(g)
    flags = dict(c["flags"], **override)
    args = SimpleNamespace(device=device, model_path="", buffer=1, num_neg=c["num_neg"], dropout=0, test_all=0, **flags)
    corpus = SimpleNamespace(n_users=c["n_users"], n_items=c["n_items"], user_feature_names=[], item_feature_names=c["item"],
                             situation_feature_names=c["sit"], feature_max=dict(c["feature_max"]))
    return args, corpus


def build_model(g, device, which="P0", seed=None):
    """the model file's class for this golden on `device`, loaded with the stored parameters `which` (None: as constructed under
    torch.manual_seed(seed))"""
    import torch
    from models.context.FinalMLP import FinalMLPCTR, FinalMLPTopK
    args, corpus = model_args(g, device)
    if seed is not None:
        torch.manual_seed(seed)
    model = (FinalMLPCTR if config(g)["ctr"] else FinalMLPTopK)(args, corpus)
    if which is not None:
        with torch.no_grad():
            for k, v in model.state_dict().items():
                v.copy_(torch.from_numpy(g[which + "/" + k]))
    return model.to(device)


def feed(g, n, device, phase="train"):
    import torch
    b = batch(g, n)
    f = {k: torch.from_numpy(v).to(device) for k, v in b.items()}
    f.update(batch_size=len(b["user_id"]), phase=phase)
    return f


def torch_loss(g, out):
    """the reference's loss on a forward's output, in torch ops: nn.BCELoss on (probability, label) for the CTR classes
    (BaseModel.py:262-274), the softmax-weighted BPR of GeneralModel.loss (:175-189) for the TopK classes"""
    import torch
    if config(g)["ctr"]:
        return torch.nn.functional.binary_cross_entropy(out["prediction"], out["label"].to(out["prediction"].dtype))
    pred = out["prediction"]
    pos, neg = pred[:, 0], pred[:, 1:]
    w = (neg - neg.max()).softmax(dim=1)
    return -(((pos[:, None] - neg).sigmoid() * w).sum(dim=1)).clamp(min=1e-8, max=1 - 1e-8).log().mean()
