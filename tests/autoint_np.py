"""Float64 numpy restatement of AutoInt's interacting layer (reference: models/context/AutoInt.py:49-80, utils/layers.py:9-63), its
hand-derived backward, the model's forward around it, and helpers that read tests/golden/autoint_*.npz.

    Q = X Wq^T, K = X Wk^T, V = X Wv^T, R = X Wr^T + br;  per instance and head: S = Q_h K_h^T / sqrt(dk), P = softmax(S), O_h = P V_h
    Y = relu(O + R)
    dZ = dY * (Y > 0), dR = dO = dZ, dP = dO_h V_h^T, dV_h = P^T dO_h, dS = P * (dP - rowsum(dP * P)),
    dQ_h = dS K_h / sqrt(dk), dK_h = dS^T Q_h / sqrt(dk), dX = dQ Wq + dK Wk + dV Wv + dR Wr, dW* = G*^T X, dbr = colsum(dR)
The reference's global-maximum shift before the softmax is a no-op for finite scores and is not restated."""
import numpy as np

TOL = 2e-5            # the project's cap: of the tensor's largest entry
SCALE0 = 20.0         # the generator's uniform parameter scaling


def row_threshold(F):
    """a softmax row over F keys counts as non-uniform when its largest probability exceeds 2 / F; at F = 2 that would be 1, which no
    row can exceed, so the bar there is halfway between uniform and one-hot (0.75; the same formula gives 2 / 3 = 2 / F at F = 3)"""
    return min(2.0 / F, 0.5 * (1.0 / F + 1.0))


def _heads(x, H):     # [N, F, A] -> [N, H, F, dk]
    N, F, A = x.shape
    return x.reshape(N, F, H, A // H).transpose(0, 2, 1, 3)


def _merge(x):        # [N, H, F, dk] -> [N, F, A]
    N, H, F, dk = x.shape
    return x.transpose(0, 2, 1, 3).reshape(N, F, H * dk)


def layer_forward(X, Wq, Wk, Wv, Wr, br, H, details=False):
    """X [N, F, Din] -> Y [N, F, A] in float64 (details: also Q, K, V as [N, H, F, dk], P [N, H, F, F] and the scaled scores S)"""
    X, Wq, Wk, Wv, Wr, br = (np.asarray(a, dtype=np.float64) for a in (X, Wq, Wk, Wv, Wr, br))
    A = Wq.shape[0]
    Q, K, V = _heads(X @ Wq.T, H), _heads(X @ Wk.T, H), _heads(X @ Wv.T, H)
    S = Q @ K.transpose(0, 1, 3, 2) / np.sqrt(A // H)
    E = np.exp(S - S.max(-1, keepdims=True))
    P = E / E.sum(-1, keepdims=True)
    Y = np.maximum(_merge(P @ V) + X @ Wr.T + br, 0.0)
    return (Y, dict(Q=Q, K=K, V=V, P=P, S=S)) if details else Y


def layer_backward(X, Wq, Wk, Wv, Wr, br, H, dY):
    """-> dict(dX, dWq, dWk, dWv, dWr, dbr) in float64, by the formulas in this module's docstring"""
    X, Wq, Wk, Wv, Wr, br, dY = (np.asarray(a, dtype=np.float64) for a in (X, Wq, Wk, Wv, Wr, br, dY))
    A, Din = Wq.shape
    Y, f = layer_forward(X, Wq, Wk, Wv, Wr, br, H, details=True)
    dZ = dY * (Y > 0)
    dO = _heads(dZ, H)
    dP = dO @ f["V"].transpose(0, 1, 3, 2)
    dV = f["P"].transpose(0, 1, 3, 2) @ dO
    dS = f["P"] * (dP - (dP * f["P"]).sum(-1, keepdims=True))
    scale = 1.0 / np.sqrt(A // H)
    dQ, dK = _merge(dS @ f["K"]) * scale, _merge(dS.transpose(0, 1, 3, 2) @ f["Q"]) * scale
    dV = _merge(dV)
    X2 = X.reshape(-1, Din)
    flat = lambda g: g.reshape(-1, A)
    return dict(dX=dQ @ Wq + dK @ Wk + dV @ Wv + dZ @ Wr, dWq=flat(dQ).T @ X2, dWk=flat(dK).T @ X2, dWv=flat(dV).T @ X2,
                dWr=flat(dZ).T @ X2, dbr=flat(dZ).sum(0))


def rel_err(got, want, floor=0.0):
    """largest |got - want| over max(largest |want|, floor)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(float(np.abs(want).max()) if want.size else 0.0, floor, 1e-30)
    return float(np.abs(got - want).max()) / scale if want.size else 0.0


def random_layer(N, F, Din, A, H, seed, score_std=2.5, relu_shift=0.0):
    """a layer problem whose softmax rows are clearly non-uniform and whose ReLU is about half active: weights at N(0, 1 /
    sqrt(Din)), Wq and Wk rescaled so that the scaled scores have standard deviation score_std (the goldens' rule) and then, while
    fewer than 60 % of the softmax rows pass row_threshold, by a further 1.25 each; relu_shift is added to the residual bias (a large negative one makes every pre-activation negative)"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    X = rng.normal(0, 1.0, (N, F, Din)).astype(f32)
    W = [rng.normal(0, 1.0 / np.sqrt(Din), (A, Din)).astype(f32) for _ in range(4)]
    br = (rng.normal(0, 0.3, A) + relu_shift).astype(f32)
    S = layer_forward(X, *W, br, H, details=True)[1]["S"]
    s = np.sqrt(score_std / max(S.std(), 1e-30))
    W[0], W[1] = (W[0] * s).astype(f32), (W[1] * s).astype(f32)
    for _ in range(12):      # heavy-tailed scores (dk = 1: a product of two normals) leave many rows flat at that std: sharpen them
        P = layer_forward(X, *W, br, H, details=True)[1]["P"]
        if (P.max(-1) > row_threshold(F)).mean() >= 0.6:
            break
        W[0], W[1] = (W[0] * f32(1.25)).astype(f32), (W[1] * f32(1.25)).astype(f32)
    dY = rng.normal(0, 1.0, (N, F, A)).astype(f32)
    return X, W[0], W[1], W[2], W[3], br, dY


# ---- the goldens -------------------------------------------------------------------------------------------------------------------
def meta(g):
    n_users, n_items, d, A, H, L, B, C, seed, ctr = (int(x) for x in g["meta"][:10])
    return dict(n_users=n_users, n_items=n_items, d=d, A=A, H=H, L=L, B=B, C=C, seed=seed, ctr=bool(ctr),
                tower=[int(x) for x in g["meta"][10:]], fields=[str(f) for f in g["fields"]], numeric=[str(f) for f in g["numeric"]])


def is_categorical(f):
    return f.endswith("_c") or f.endswith("_id")


def state_keys(g):
    return [str(k) for k in g["state_keys"]]


def init_from_seed(g):
    """the state_dict the reference's constructor leaves under torch.manual_seed(seed), restated on plain torch modules: the same
    modules created in the same order (AutoInt.py:49-66, FM.py:34-42: their default initialisers draw from the global stream), then
    init_weights over them in registration order (BaseModel.py:29-35: N(0, 0.01) for every Linear / Embedding weight and Linear
    bias).  The generator asserts this to be bit-equal to the reference's own state_dict for every case."""
    import torch
    import torch.nn as nn
    m = meta(g)
    fmax = dict(zip(m["fields"], (int(x) for x in g["feature_max"])))
    torch.manual_seed(m["seed"])
    ctx, lin = nn.ModuleDict(), nn.ModuleDict()
    for f in m["fields"]:
        ctx[f] = nn.Embedding(fmax[f], m["d"]) if is_categorical(f) else nn.Linear(1, m["d"], bias=False)
        lin[f] = nn.Embedding(fmax[f], 1) if is_categorical(f) else nn.Linear(1, 1, bias=False)
    att, res, width = nn.ModuleList(), nn.ModuleList(), m["d"]
    for _ in range(m["L"]):
        a = nn.Module()
        a.q_linear, a.k_linear, a.v_linear = (nn.Linear(width, m["A"], bias=False) for _ in range(3))
        att.append(a)
        res.append(nn.Linear(width, m["A"]))
        width = m["A"]
    widths = [len(m["fields"]) * m["A"]] + m["tower"] + [1]
    mlp = nn.Sequential()
    k = 0
    for i in range(len(widths) - 1):
        mlp.add_module(str(k), nn.Linear(widths[i], widths[i + 1]))
        k += 1 if i == len(widths) - 2 else 2      # a ReLU sits behind every hidden Linear
    root = nn.Module()
    root.context_embedding, root.linear_embedding = ctx, lin
    root.overall_bias = nn.Parameter(torch.tensor([0.01]))
    root.autoint_attentions, root.residual_embeddings = att, res
    root.deep_layers = nn.Module()
    root.deep_layers.mlp = mlp
    for mod in root.modules():
        if isinstance(mod, nn.Linear):
            nn.init.normal_(mod.weight, mean=0.0, std=0.01)
            if mod.bias is not None:
                nn.init.normal_(mod.bias, mean=0.0, std=0.01)
        elif isinstance(mod, nn.Embedding):
            nn.init.normal_(mod.weight, mean=0.0, std=0.01)
    return {k: v.detach().numpy().copy() for k, v in root.state_dict().items()}


def initial_params(g):
    """{key: float32 array}: the state_dict straight after construction: I0/<key> where the golden stores it, else (the one case
    whose tensors would not fit the size limit a fourth time) regenerated from the seed by init_from_seed and held, tensor by
    tensor, to the SHA-256 of the reference's own bits that the golden stores instead (I0sha/<key>)"""
    if "I0/overall_bias" not in g:
        import hashlib
        out = init_from_seed(g)
        for k, v in out.items():
            assert hashlib.sha256(v.tobytes()).hexdigest() == str(g["I0sha/" + k]), k
        return out
    return {k: g["I0/" + k] for k in state_keys(g)}


def scaled_params(g):
    """{key: float32 array}: the parameters every stored result starts from, P0 = fl(fl(I0 * 20) * s_l) with s_l = qk_scale[l] on
    layer l's q_linear / k_linear weights and 1 elsewhere, in float32 as the generator applied it (which asserted that this
    derivation is bit-equal to the model it ran)"""
    out = {}
    for k, v in initial_params(g).items():
        p = v * np.float32(SCALE0)
        parts = k.split(".")
        if parts[0] == "autoint_attentions" and parts[2] in ("q_linear", "k_linear"):
            p = p * np.float32(g["qk_scale"][int(parts[1])])
        out[k] = p.astype(np.float32)
    return out


def batch(g, n):
    pre = "b%d/" % n
    return {k[len(pre):]: g[k] for k in g if k.startswith(pre)}


def field_vectors(P, g, b):
    """-> (X [B, C, F, d], first-order term [B, C]) in float64 from the parameters P (models/context/FM.py:44-57)"""
    m = meta(g)
    C = b["item_id"].shape[1]
    vecs, lin = [], []
    for f in m["fields"]:
        x = b[f]
        if is_categorical(f):
            v, w = P["context_embedding.%s.weight" % f].astype(np.float64)[x], P["linear_embedding.%s.weight" % f].astype(np.float64)[x]
        else:      # Linear(1, d, bias=False) on the value, which the reference casts to float32 first
            xv = x.astype(np.float32).astype(np.float64)[..., None]
            v, w = xv * P["context_embedding.%s.weight" % f].astype(np.float64)[:, 0], xv * P["linear_embedding.%s.weight" % f].astype(np.float64)[:, 0]
        if v.ndim == 2:
            v, w = np.repeat(v[:, None, :], C, 1), np.repeat(w[:, None, :], C, 1)
        vecs.append(v)
        lin.append(w)
    first = P["overall_bias"].astype(np.float64) + np.concatenate(lin, -1).sum(-1)
    return np.stack(vecs, -2), first


def layer_weights(P, l):
    pre = "autoint_attentions.%d." % l
    return (P[pre + "q_linear.weight"], P[pre + "k_linear.weight"], P[pre + "v_linear.weight"], P["residual_embeddings.%d.weight" % l],
            P["residual_embeddings.%d.bias" % l])


def tower(P, x):
    """MLP_Block: Linear -> ReLU per hidden layer, then the output Linear; -> (output [..., 1], the inputs and masks of every layer)"""
    ks = sorted({int(k.split(".")[2]) for k in P if k.startswith("deep_layers.mlp.")})
    trace = []
    for i, k in enumerate(ks):
        W, b = P["deep_layers.mlp.%d.weight" % k].astype(np.float64), P["deep_layers.mlp.%d.bias" % k].astype(np.float64)
        pre = x @ W.T + b
        last = i == len(ks) - 1
        trace.append((k, x, None if last else pre > 0))
        x = pre if last else np.maximum(pre, 0.0)
    return x, trace


def model_forward(P, g, b):
    """-> dict(X, first, Ys [per layer], deep_in, tower trace, raw [B, C]) in float64"""
    m = meta(g)
    X, first = field_vectors(P, g, b)
    Bn, C, F, d = X.shape
    x, Ys = X.reshape(Bn * C, F, d), []
    for l in range(m["L"]):
        x = layer_forward(x, *layer_weights(P, l), m["H"])
        Ys.append(x.reshape(Bn, C, F, -1))
    out, trace = tower(P, x.reshape(Bn, C, -1))
    return dict(X=X, first=first, Ys=Ys, trace=trace, raw=first + out[..., 0])


def attention_grads(P, g, b, graw):
    """gradients of every attention-path parameter and of the tower, from graw = d loss / d raw prediction [B, C], float64"""
    m = meta(g)
    f = model_forward(P, g, b)
    Bn, C, F, d = f["X"].shape
    G = {}
    gx = np.asarray(graw, dtype=np.float64)[..., None]
    for k, x, mask in reversed(f["trace"]):
        W = P["deep_layers.mlp.%d.weight" % k].astype(np.float64)
        if mask is not None:
            gx = gx * mask
        G["deep_layers.mlp.%d.weight" % k] = gx.reshape(-1, W.shape[0]).T @ x.reshape(-1, W.shape[1])
        G["deep_layers.mlp.%d.bias" % k] = gx.reshape(-1, W.shape[0]).sum(0)
        gx = gx @ W
    gy = gx.reshape(Bn * C, F, -1)
    xs = [f["X"].reshape(Bn * C, F, d)] + [y.reshape(Bn * C, F, -1) for y in f["Ys"][:-1]]
    for l in reversed(range(m["L"])):
        r = layer_backward(xs[l], *layer_weights(P, l), m["H"], gy)
        pre = "autoint_attentions.%d." % l
        G[pre + "q_linear.weight"], G[pre + "k_linear.weight"], G[pre + "v_linear.weight"] = r["dWq"], r["dWk"], r["dWv"]
        G["residual_embeddings.%d.weight" % l], G["residual_embeddings.%d.bias" % l] = r["dWr"], r["dbr"]
        gy = r["dX"]
    G["field_vectors"] = gy.reshape(Bn, C, F, d)
    return G


def graw_from_gpred(g):
    """d loss / d raw prediction from the stored gpred: the CTR classes hand out the probability (AutoInt.py:97), whose gradient
    passes the sigmoid; the TopK classes the raw score"""
    gp = g["gpred"].astype(np.float64)
    if not meta(g)["ctr"]:
        return gp
    p = g["pred"].astype(np.float64)
    return (gp * p * (1.0 - p)).reshape(-1, 1)


def bound_for(g, key):
    """(bound, why): 2e-5 of the largest entry; where the golden's stored fp32-vs-float64 deviation of the reference itself exceeds
    1e-5 for this tensor, twice that deviation"""
    k = "dev/" + key
    if k in g and float(g[k]) > 1e-5:
        return 2.0 * float(g[k]), "twice the reference's own fp32 deviation %.1e" % float(g[k])
    return TOL, "the cap"


def grad_floor(g):
    """the scale below which a gradient tensor is round-off (rel_err's floor), as tests/comirec_np.py sets it: a gradient that is
    exactly zero in exact arithmetic (under BPR the first-order terms of the user-side fields, which shift every candidate of a row
    alike; a field whose value never varies; an inactive unit) is compared no finer than 1e-6 of the batch's largest gradient entry"""
    top = max(float(np.abs(g[k]).max()) for k in g if k.startswith("G/"))
    return 1e-6 * top / TOL


# ---- the model file around the goldens (torch is imported only here) ---------------------------------------------------------------
def build_model(g, device, params=None):
    """the model file's class for this golden on `device`, loaded with `params` (default: the scaled parameters P0; an empty dict:
    nothing is loaded).  The corpus lists every side feature as a user feature: the model only sees their order, which `fields`
    fixes"""
    import torch
    from types import SimpleNamespace
    from models.context.AutoInt import AutoIntCTR, AutoIntTopK
    m = meta(g)
    args = SimpleNamespace(device=device, model_path="", buffer=1, num_neg=m["C"] - 1, dropout=0, test_all=0, emb_size=m["d"],
                           attention_size=m["A"], num_heads=m["H"], num_layers=m["L"], layers=str(m["tower"]),
                           loss_n="BCE" if m["ctr"] else "BPR")
    corpus = SimpleNamespace(n_users=m["n_users"], n_items=m["n_items"], user_feature_names=m["fields"][:-2], item_feature_names=[],
                             situation_feature_names=[], feature_max=dict(zip(m["fields"], (int(x) for x in g["feature_max"]))))
    model = (AutoIntCTR if m["ctr"] else AutoIntTopK)(args, corpus).to(device)
    if params is None or params:
        load_params(model, scaled_params(g) if params is None else params)
    return model


def load_params(model, P):
    import torch
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(torch.from_numpy(np.asarray(P[k])))


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
    if meta(g)["ctr"]:
        return torch.nn.functional.binary_cross_entropy(out["prediction"], out["label"].float())
    pred = out["prediction"]
    pos, neg = pred[:, 0], pred[:, 1:]
    w = (neg - neg.max()).softmax(dim=1)
    return -(((pos[:, None] - neg).sigmoid() * w).sum(dim=1)).clamp(min=1e-8, max=1 - 1e-8).log().mean()
