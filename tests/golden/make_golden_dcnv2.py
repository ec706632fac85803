"""Golden vectors for DCNv2 FROM THE REFERENCE ITSELF (models/context/DCNv2.py, helpers/BaseRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dcnv2.py [--out DIR]

Each dcnv2_*.npz holds
  meta [n_users, n_items, d, low_rank, E, L, B, C, seed, ctr, mixed, stacked, sub] + tower widths; fields (names in model order),
  numeric (names), user / item / sit (the corpus' feature name lists), fmax_names / fmax (the corpus' feature_max), reg_weight
  I0/<key>        the state_dict straight after construction under torch.manual_seed(seed): pins the init stream.  The one case
                  with sub = 1 (the demo width D = 512) stores I0sha/<key>, the SHA-256 of each tensor, instead
  v_scale, c_scale [L, E], gate_scale     the parameters every computation below starts from are P0 = I0 with V_{l,e} x v_scale[l, e],
                  C_{l,e} x c_scale[l, e] and every gating weight (not the bias) x gate_scale (tests/dcnv2_np.py:scale_state recomputes P0,
                  and this generator asserts that to be bit-equal to the parameters it ran).  Unscaled, both tanh stages run in
                  their linear regime (|argument| about 0.05) and every gate is uniform (logits about 1e-3): a kernel without tanh or
                  without the softmax would pass.  gate_scale makes the median row's largest gate probability 0.75 on the first batch's
                  x_0; then, layer by layer on the first batch, v_scale makes the median |V^T x_l| 1 and c_scale the median |C t| 1.
  b1/<f>, b2/<f>  two training batches (ids, features, label for CTR)
  X<l>            every cross layer's output on the first batch [B * C, D]
  pred, loss, gpred, G/<key>     first batch: prediction, loss, d loss / d prediction, every parameter's gradient
  <opt>/<key>, <opt>_losses, <opt>_hyper     parameters (and BatchNorm buffers) after two optimizer steps from P0, the two losses, (lr, l2)
  dev/X<l>, dev/pred, dev/loss, dev/G/<key>  the reference's own fp32 result against a float64 run of the same modules (the numeric
                  fields' Linear fed the float32 value as a double; the backward driven by the stored gpred), as
                  largest |difference| / largest |float64 entry|
  zero_grad_keys  gradients that are exactly zero in exact arithmetic (the bias of a Linear in front of BatchNorm1d; under BPR the
                  output bias): round-off in every precision, so no dev/ is recorded for them
  state_keys      the state_dict's keys in order
In the sub = 1 case every G/, <opt>/ tensor above dcnv2_np.BIG elements is stored as its every dcnv2_np.SUB-th element (flat): U, V
and the tower's first weight alone would be three times the size limit.
dcnv2_layer_dev.npz holds no tensors: <N>_<D>_<r>_<E>_<seed>/<tensor> and stack/<tensor> are the same kind of deviation for the random
layer problems of tests/test_gpu_dcnv2.py (dcnv2_np.LAYER_PROBLEMS, the demo-shape stack), which are regenerated from their seeds.
The generator asserts, in every mixed case: in every (layer, expert) the median |p| and the median |q| lie in [0.3, 2.0]; for
E >= 2, in every layer at least half of the rows have a largest gate probability above 0.6 and every expert's mean gate probability is
above 1 / (4 E).  A seed that misses the gate conditions is replaced by the next one (the seed used is the one in meta).
"""
import argparse
import copy
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (numpy alias shim too)
from make_golden_deepfm import MIND  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
import dcnv2_np  # noqa: E402

SMALL = {"i_category_c": 6, "i_subcategory_c": 12, "c_hour_c": 8, "c_period_c": 4, "c_weekday_c": 7}
MIND_S = dict(MIND, vocab=SMALL)                                       # F = 8, c_day_f numeric
ONE_FEATURE = dict(user=[], item=["i_category_c"], sit=[], vocab={"i_category_c": 11}, numeric={})      # F = 3
IDS_ONLY = dict(user=[], item=[], sit=[], vocab={}, numeric={})        # F = 2
GATE_MEDIAN = 0.75


class GateMiss(Exception):
    pass


def make_case(out_dir, name, mode, mixed, structure, d, r, E, L, tower, B, K, spec, opt, seed, n_users, n_items, sub=False):
    torch, _, BaseRunner = make_golden._import_reference()
    from models.context.DCNv2 import DCNv2CTR, DCNv2TopK
    torch.set_num_threads(1)   # one summation order for every rerun
    ctr = mode == "CTR"
    cls = DCNv2CTR if ctr else DCNv2TopK
    USER, ITEM, SIT, VOC, NUMERIC = spec["user"], spec["item"], spec["sit"], spec["vocab"], spec["numeric"]
    rng = np.random.default_rng(seed)
    reg_weight = 0.05
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=K, dropout=0, test_all=0, emb_size=d,
                           layers=str(tower), cross_layer_num=L, reg_weight=reg_weight, mixed=mixed, structure=structure, low_rank=r,
                           expert_num=E, loss_n="BCE" if ctr else "BPR")
    fmax = dict(VOC, user_id=n_users, item_id=n_items)
    for f, (_, top) in NUMERIC.items():
        fmax[f] = top
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, user_feature_names=USER, item_feature_names=ITEM,
                             situation_feature_names=SIT, feature_max=fmax)
    torch.manual_seed(seed)
    model = cls(args, corpus)
    C = 1 if ctr else 1 + K
    out = {"meta": np.array([n_users, n_items, d, r, E, L, B, C, seed, int(ctr), mixed, int(structure == "stacked"), int(sub)]
                            + list(tower), dtype=np.int64),
           "fields": np.array(model.context_features), "numeric": np.array(sorted(NUMERIC), dtype=str),
           "user": np.array(USER, dtype=str), "item": np.array(ITEM, dtype=str), "sit": np.array(SIT, dtype=str),
           "fmax_names": np.array(list(fmax)), "fmax": np.array(list(fmax.values()), dtype=np.int64),
           "reg_weight": np.float64(reg_weight), "state_keys": np.array(list(model.state_dict().keys()))}
    I0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    for k, v in I0.items():
        if sub:
            out["I0sha/" + k] = np.array(hashlib.sha256(v.tobytes()).hexdigest())
        else:
            out["I0/" + k] = v

    def column(f, size):
        if f not in NUMERIC:
            return rng.integers(0, VOC[f], size=size).astype(np.int64)
        dtype, top = NUMERIC[f]
        if dtype == "int64":
            return rng.integers(0, top, size=size).astype(np.int64)
        return (rng.random(size=size) * (top - 1)).astype(np.float64)

    item_cols = {f: column(f, n_items) for f in ITEM}

    def batch():
        b = {"user_id": rng.integers(1, n_users, size=B).astype(np.int64),
             "item_id": rng.integers(1, n_items, size=(B, C)).astype(np.int64)}
        b["item_id"][:, 0] = b["item_id"][:, 0] % 5 + 1  # duplicates
        for f in USER + SIT:
            b[f] = column(f, B)
        for f in ITEM:
            b[f] = item_cols[f][b["item_id"]]
        if ctr:
            b["label"] = rng.integers(0, 2, size=(B, 1)).astype(np.int64)
        return b

    batches = [batch(), batch()]
    for n, b in enumerate(batches, 1):
        for k, v in b.items():
            out["b%d/%s" % (n, k)] = v

    def feed(b):
        f = {k: torch.from_numpy(v) for k, v in b.items()}
        f.update(batch_size=B, phase="train")
        return f

    def x_layers(m, fd):
        """[x_0, x_1, ..., x_L], each [B * C, D]: the reference's own cross network, cut after l layers"""
        seen, net = {}, ("cross_net_mix" if mixed else "cross_net_2")
        plain = getattr(m, net)
        setattr(m, net, lambda x: seen.setdefault("x0", x) is None or plain(x))
        was_training = m.training
        m.eval()                   # (the tower's BatchNorm must not count this probe as a training batch)
        with torch.no_grad():
            m(fd)
        m.train(was_training)
        delattr(m, net)
        xs = [seen["x0"].reshape(B * C, -1)]
        n_layers = m.cross_layer_num
        with torch.no_grad():
            for l in range(1, n_layers + 1):
                m.cross_layer_num = l
                xs.append(plain(seen["x0"]).reshape(B * C, -1))
        m.cross_layer_num = n_layers
        return xs

    v_scale, c_scale, gate_scale = np.ones((L, E), np.float32), np.ones((L, E), np.float32), np.float32(1.0)
    if mixed:
        with torch.no_grad():
            x0 = x_layers(model, feed(batches[0]))[0]
            if E > 1:      # the smallest power of 1.25 that makes the median row's largest gate probability GATE_MEDIAN on x_0
                Wg = torch.cat([gt.weight for gt in model.gating], dim=0).double()
                bg = torch.cat([gt.bias for gt in model.gating], dim=0).double()
                s = 1.0
                while (x0.double() @ (Wg * s).T + bg).softmax(dim=1).max(1).values.median().item() < GATE_MEDIAN:
                    s *= 1.25
                gate_scale = np.float32(s)
            for gt in model.gating:
                gt.weight.mul_(float(gate_scale))
            for l in range(L):
                for e in range(E):
                    xl = x_layers(model, feed(batches[0]))[l]
                    p = xl @ model.cross_layer_v[l][e]
                    v_scale[l, e] = np.float32(1.0 / p.abs().median().item())
                    model.cross_layer_v[l][e].mul_(float(v_scale[l, e]))
                    q = torch.tanh(xl @ model.cross_layer_v[l][e]) @ model.cross_layer_c[l][e].T
                    c_scale[l, e] = np.float32(1.0 / q.abs().median().item())
                    model.cross_layer_c[l][e].mul_(float(c_scale[l, e]))
            xs = x_layers(model, feed(batches[0]))
            for l in range(L):
                for e in range(E):
                    p = xs[l] @ model.cross_layer_v[l][e]
                    q = torch.tanh(p) @ model.cross_layer_c[l][e].T
                    mp, mq = p.abs().median().item(), q.abs().median().item()
                    assert 0.3 <= mp <= 2.0 and 0.3 <= mq <= 2.0, (name, l, e, mp, mq)
                if E >= 2:
                    gp = torch.cat([gt(xs[l]) for gt in model.gating], dim=1).softmax(dim=1)
                    share, mean = (gp.max(1).values > 0.6).float().mean().item(), gp.mean(0)
                    if share < 0.5 or mean.min().item() <= 1.0 / (4 * E):
                        raise GateMiss((name, seed, l, share, mean.tolist()))
                    print("  layer %d: rows with a gate above 0.6: %.0f %%, mean gate %s" % (l, 100 * share, np.round(mean.numpy(), 3)))
    out["v_scale"], out["c_scale"], out["gate_scale"] = v_scale, c_scale, gate_scale
    P0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    derived = dcnv2_np.scale_state(I0, out)
    for k, v in P0.items():
        assert derived[k].tobytes() == v.tobytes(), (name, k)

    def keep(k, v):
        v = np.asarray(v)
        return v.reshape(-1)[::dcnv2_np.SUB].copy() if (sub and v.size > dcnv2_np.BIG) else v.copy()

    xs = x_layers(model, feed(batches[0]))
    for l in range(L):
        out["X%d" % l] = xs[l + 1].numpy().copy()
    model.zero_grad()
    model.train()
    o = model(feed(batches[0]))
    pred = o["prediction"]
    pred.retain_grad()
    loss = model.loss(o)
    loss.backward()
    out["pred"], out["loss"], out["gpred"] = pred.detach().numpy().copy(), np.float32(loss.item()), pred.grad.numpy().copy()
    G32 = {k: p.grad.numpy().copy() for k, p in model.named_parameters()}
    for k, v in G32.items():
        out["G/" + k] = keep(k, v)

    # the reference's own fp32 deviation from a float64 run of the same modules
    class _DoubleIn(torch.nn.Linear):
        def forward(self, x):
            return super().forward(x.double())
    m64 = copy.deepcopy(model).double()
    for f in NUMERIC:
        lin = _DoubleIn(1, d, bias=False).double()
        lin.weight = m64.context_embedding[f].weight
        m64.context_embedding[f] = lin
    m64.zero_grad()
    xs64 = x_layers(m64, feed(batches[0]))
    for l in range(L):
        out["dev/X%d" % l] = np.float64(dcnv2_np.rel_err(out["X%d" % l], xs64[l + 1].numpy()))
    p64 = m64(feed(batches[0]))["prediction"]
    p64.backward(torch.from_numpy(out["gpred"]).double().view_as(p64))
    out["dev/pred"] = np.float64(dcnv2_np.rel_err(out["pred"].reshape(-1), p64.detach().numpy().reshape(-1)))
    with torch.no_grad():
        if ctr:
            l64 = torch.nn.functional.binary_cross_entropy(p64.detach(), torch.from_numpy(batches[0]["label"]).view(-1).double())
        else:
            from models.BaseContextModel import ContextModel
            l64 = ContextModel.loss(m64, {"prediction": p64.detach()})
        if not mixed:
            l64 = l64 + reg_weight * sum(W.norm(2) for W in m64.cross_layer_w2)
    out["dev/loss"] = np.float64(abs(float(out["loss"]) - l64.item()) / abs(l64.item()))
    gmax = max(float(np.abs(v).max()) for v in G32.values())
    # exactly zero in exact arithmetic, round-off in every precision: the bias of a Linear in front of BatchNorm1d (the batch mean
    # takes it out again) and, under BPR, the output bias (it shifts every candidate of a row alike).  No dev/ for them.
    zero = ["deep_layers.mlp.%d.bias" % (3 * k) for k in range(len(tower))] + ([] if ctr else ["predict_layer.bias"])
    out["zero_grad_keys"] = np.array(zero)
    for k in zero:
        assert float(np.abs(G32[k]).max()) <= 1e-5 * gmax, (name, k)
    for k, p in m64.named_parameters():
        if k in zero:
            continue
        g64 = p.grad.numpy() if p.grad is not None else np.zeros(p.shape)
        if not mixed and k.startswith("cross_layer_w2"):     # gpred does not carry the norm term: add its gradient W / ||W||
            g64 = g64 + reg_weight * (p / p.norm(2)).detach().numpy()
        out["dev/G/" + k] = np.float64(dcnv2_np.rel_err(G32[k], g64, 1e-6 * gmax))
    print("  fp32 vs float64: x_L %.1e, pred %.1e, loss %.1e, worst gradient %.1e" % (
        out["dev/X%d" % (L - 1)], out["dev/pred"], out["dev/loss"], max(out["dev/G/" + k] for k in G32 if k not in zero)))

    opt_name, lr, l2 = opt
    m = cls(args, corpus)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P0.items()})
    m.train()
    runner = BaseRunner(make_golden._runner_args(BaseRunner, opt_name, lr, l2))
    m.optimizer = runner._build_optimizer(m)
    losses = []
    for b in batches:
        m.optimizer.zero_grad()
        ls = m.loss(m(feed(b)))
        ls.backward()
        m.optimizer.step()
        losses.append(ls.item())
    for k, v in m.state_dict().items():
        out["{}/{}".format(opt_name, k)] = keep(k, v.detach().numpy())
    out[opt_name + "_losses"] = np.array(losses, dtype=np.float32)
    out[opt_name + "_hyper"] = np.array([lr, l2], dtype=np.float64)
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 512 * 1024, (name, size)
    print("wrote", path, size >> 10, "KiB")


def make_layer_devs(out_dir):
    """dcnv2_layer_dev.npz: for every random layer problem of dcnv2_np.LAYER_PROBLEMS and for the demo-shape stack, per tensor, the
    deviation of the reference's expression (DCNv2.py:119-141) in float32 torch ops from float64 -- the dev/<key> of a problem that
    is regenerated from its seed instead of being stored.  The GPU tests hold the kernels to max(2e-5, 4 x these stored figures)."""
    torch, _, _ = make_golden._import_reference()
    torch.set_num_threads(1)
    out = {}
    for prob_id in dcnv2_np.LAYER_PROBLEMS:
        N, D, r, E, seed, zero_row = prob_id
        prob = dcnv2_np.random_layer(N, D, r, E, seed=seed, zero_row=zero_row)
        fwd, bwd = dcnv2_np.mix_layer_forward(*prob[:8]), dcnv2_np.mix_layer_backward(prob[8], *prob[:8])
        for name, v in dcnv2_np.fp32_deviation(prob, fwd, bwd).items():
            out["%s/%s" % (dcnv2_np.layer_key(*prob_id), name)] = np.float64(v)
    leaves, dY = dcnv2_np.stack_problem()
    L = dcnv2_np.STACK["L"]
    want = dcnv2_np.torch_stack([torch.from_numpy(a).double().requires_grad_(True) for a in leaves], L, torch.from_numpy(dY))
    got = dcnv2_np.torch_stack([torch.from_numpy(a).clone().requires_grad_(True) for a in leaves], L, torch.from_numpy(dY))
    for name, a, b in zip(dcnv2_np.STACK_NAMES, got, want):
        out["stack/" + name] = np.float64(dcnv2_np.rel_err(a.numpy(), b.numpy()))
    path = os.path.join(out_dir, "dcnv2_layer_dev.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB; largest deviation %.2e (%s)" % max((float(v), k) for k, v in out.items()))


ADAM, SGD, ADAGRAD = ("Adam", 1e-3, 1e-4), ("SGD", 0.05, 1e-3), ("Adagrad", 0.01, 1e-4)
CASES = [
    # name,                                   mode, mixed, structure,  d,  r, E, L, tower, B, K, fields,     optimizer, seed, users, items
    ("dcnv2_a_ctr_mix_stacked_d16_r8_e2_l3",   "CTR",  1, "stacked",  16,  8, 2, 3, [32],     33, 0, MIND_S,      ADAM,    71,  8, 10),
    ("dcnv2_b_topk_mix_parallel_d8_r4_e1_l4",  "TopK", 1, "parallel",  8,  4, 1, 4, [16],      5, 4, ONE_FEATURE, SGD,     72, 40, 60),
    ("dcnv2_c_ctr_mix_parallel_d64_r64_e2_l2", "CTR",  1, "parallel", 64, 64, 2, 2, [64],      3, 0, MIND_S,      ADAGRAD, 73,  8, 10, True),
    ("dcnv2_d_topk_mix_stacked_d4_r12_e4_l1",  "TopK", 1, "stacked",   4, 12, 4, 1, [8],       2, 1, IDS_ONLY,    ADAM,    74, 40, 60),
    ("dcnv2_e_ctr_plain_parallel_d8_l3",       "CTR",  0, "parallel",  8,  4, 1, 3, [16],     17, 0, MIND_S,      ADAM,    75,  8, 10),
    ("dcnv2_f_topk_plain_stacked_d16_l2",      "TopK", 0, "stacked",  16,  4, 1, 2, [32, 16],  4, 3, ONE_FEATURE, SGD,     76, 40, 60),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    make_layer_devs(a.out)
    for c in CASES:
        c = list(c)
        for attempt in range(200):
            print(c[0], "seed", c[13])
            try:
                make_case(a.out, *c)
                break
            except GateMiss as e:
                print("  gate conditions missed:", e)
                c[13] += 100
        else:
            raise SystemExit("no seed met the gate conditions for " + c[0])
