"""Golden vectors for DIN FROM THE REFERENCE ITSELF (models/context_seq/DIN.py, models/BaseContextModel.py, utils/layers.py,
helpers/BaseRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_din.py [--out DIR]

Each din_*.npz holds
  meta [n_users, n_items, d, L, B, C, seed, ctr, add_historical_situations], att_layers, dnn_layers, user / item / sit (field names),
  numeric (names), fmax_names / fmax (the corpus' feature_max)
  state_keys      the state_dict's keys in order (BatchNorm buffers included)
  I0sha/<key>     SHA-256 of every tensor of the state_dict straight after construction under torch.manual_seed(seed): pins the init
                  stream (the tensors themselves would not fit the size limit beside the gradients and the updated parameters; the
                  tests build the model under the same seed and compare digests)
  att_scale       the parameters every computation below starts from are P0: every PARAMETER of I0 times 20, then the weight and
                  bias of the l-th Linear of att_mlp_layers times att_scale[l], chosen layer by layer on the first batch so that its
                  output has standard deviation 2.5 over the valid positions (1.0 for the output layer) (the untouched init leaves every attention weight at
                  about b_out / sqrt(H): the attention would go untested).  P0 = fl(fl(I0 * 20) * att_scale) in float32; the
                  BatchNorm buffers stay as constructed
  b1/<f>, b2/<f>  two training batches (ids, features, histories right-padded with 0, lengths with 1, L and values between, label)
  att_out, att_w  first batch: DINBase.attention's output [N, H] and its weights (return_seq_weight) [N, L]
  pred, loss, G/<key>     first batch: prediction, loss, every parameter's gradient
  <opt>/<key>, <opt>_losses, <opt>_hyper     parameters and BatchNorm buffers after two optimizer steps from P0, the losses, (lr, l2)
  dev/att_out, dev/att_w, dev/pred, dev/loss, dev/G/<key>     cases without numeric fields: the reference's own fp32 result against
                  a float64 run of the same modules, as largest |difference| / largest |float64 entry| (gradients: the
                  denominator is at least 1e-6 of the largest entry of any gradient)
The generator asserts on the first batch: every attention layer's pre-activation has a standard deviation in [0.5, 3] over the
valid positions, and among the instances with at least two valid positions at least half have weights whose spread
(std / mean |w| over the valid positions) is at least 0.2.
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
from make_golden_autoint import GENERIC, IDS_ONLY, MIND_S  # noqa: E402

TARGET_STD = (2.5, 1.0)      # hidden layers, output layer


def zero_grad_keys(model):
    """the bias of a Linear that feeds a BatchNorm1d: its gradient is exactly zero in exact arithmetic (the batch mean is taken
    out right behind it) and round-off in every precision -- no dev/ entry; the tests bound it absolutely"""
    mods = list(model.dnn_mlp_layers.mlp)
    return ["dnn_mlp_layers.mlp.%d.bias" % i for i, m in enumerate(mods[:-1])
            if type(m).__name__ == "Linear" and type(mods[i + 1]).__name__ == "BatchNorm1d"]


def make_case(out_dir, name, mode, d, att, dnn, L, B, K, spec, hs, opt, seed, n_users, n_items):
    torch, _, BaseRunner = make_golden._import_reference()
    from models.context_seq.DIN import DINCTR, DINTopK
    torch.set_num_threads(1)   # one summation order for every rerun
    ctr = mode == "CTR"
    cls = DINCTR if ctr else DINTopK
    USER, ITEM, SIT, VOC, NUMERIC = spec["user"], spec["item"], spec["sit"], spec["vocab"], spec["numeric"]
    rng = np.random.default_rng(seed)
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=K, dropout=0, test_all=0, emb_size=d,
                           att_layers=str(att), dnn_layers=str(dnn), history_max=L, add_historical_situations=hs,
                           loss_n="BCE" if ctr else "BPR")
    fmax = dict(VOC, user_id=n_users, item_id=n_items)
    for f, (_, top) in NUMERIC.items():
        fmax[f] = top
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, user_feature_names=USER, item_feature_names=ITEM,
                             situation_feature_names=SIT, feature_max=fmax)
    torch.manual_seed(seed)
    model = cls(args, corpus)
    C = 1 if ctr else 1 + K
    N = B * C
    out = {"meta": np.array([n_users, n_items, d, L, B, C, seed, int(ctr), hs], dtype=np.int64),
           "att_layers": np.array(att, dtype=np.int64), "dnn_layers": np.array(dnn, dtype=np.int64),
           "user": np.array(USER, dtype=str), "item": np.array(ITEM, dtype=str), "sit": np.array(SIT, dtype=str),
           "numeric": np.array(sorted(NUMERIC), dtype=str), "fmax_names": np.array(sorted(fmax)),
           "fmax": np.array([fmax[f] for f in sorted(fmax)], dtype=np.int64)}
    out["state_keys"] = np.array(list(model.state_dict().keys()))
    for k, v in model.state_dict().items():
        out["I0sha/" + k] = np.array(hashlib.sha256(v.detach().numpy().tobytes()).hexdigest())

    def column(f, size):
        if f not in NUMERIC:
            return rng.integers(0, VOC[f], size=size).astype(np.int64)
        dtype, top = NUMERIC[f]
        if dtype == "int64":
            return rng.integers(0, top, size=size).astype(np.int64)
        return (rng.random(size=size) * (top - 1)).astype(np.float64)

    item_cols = {f: column(f, n_items) for f in ITEM}     # item_meta: one value per item

    def batch():
        b = {"user_id": rng.integers(1, n_users, size=B).astype(np.int64),
             "item_id": rng.integers(1, n_items, size=(B, C)).astype(np.int64)}
        for f in USER + SIT:
            b[f] = column(f, B)
        for f in ITEM:
            b[f] = item_cols[f][b["item_id"]]
        lens = rng.integers(1, L + 1, size=B).astype(np.int64)
        lens[0] = L                                   # the padded width of the batch is L
        if B > 1:
            lens[-1] = 1
        valid = np.arange(L)[None, :] < lens[:, None]
        hist = np.where(valid, rng.integers(1, n_items, size=(B, L)), 0).astype(np.int64)
        b["history_item_id"] = hist
        for f in ITEM:                                # right-padded with 0 like every ragged key (pad_sequence)
            b["history_" + f] = np.where(valid, item_cols[f][hist], 0).astype(item_cols[f].dtype)
        if hs:
            for f in SIT:
                col = column(f, (B, L))
                b["history_" + f] = np.where(valid, col, 0).astype(col.dtype)
        b["lengths"] = lens
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

    def spied(m, fd):
        """(output dict, attention output, attention weights, the pre-activations of att_mlp_layers' Linear modules)"""
        rec, pre, hooks = {}, [], []
        plain = type(m).attention

        def spy(q, k, kl, mask, softmax_stag=False, return_seq_weight=False):
            rec["w"] = plain(m, q, k, kl, mask, softmax_stag, True).detach().clone()
            o = plain(m, q, k, kl, mask, softmax_stag, return_seq_weight)
            rec["out"] = o.detach().clone()
            return o
        m.attention = spy
        for mod in m.att_mlp_layers.mlp:
            if isinstance(mod, torch.nn.Linear):
                hooks.append(mod.register_forward_hook(lambda _m, _i, o, pre=pre: pre.append(o.detach().clone())))
        o = m(fd)
        for h in hooks:
            h.remove()
        del m.attention
        n_lin = len(att) + 1
        return o, rec["out"], rec["w"], pre[-n_lin:]      # (the second call's pre-activations: the same values)

    lens0 = np.repeat(batches[0]["lengths"], C)
    valid0 = np.arange(L)[None, :] < lens0[:, None]                                       # [N, L]
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(20.0)
        linears = [mod for mod in model.att_mlp_layers.mlp if isinstance(mod, torch.nn.Linear)]
        att_scale = []
        for l, lin in enumerate(linears):
            z = spied(model, feed(batches[0]))[3][l].double().numpy().reshape(N, L, -1)[valid0]
            s = float(np.float32(TARGET_STD[l == len(att)] / z.std()))      # the spread ACROSS rows, unit by unit
            att_scale.append(s)
            lin.weight.mul_(s)
            lin.bias.mul_(s)
        _, _, w, pre = spied(model, feed(batches[0]))
    out["att_scale"] = np.array(att_scale, dtype=np.float32)
    for l, z in enumerate(pre):
        sd = float(z.double().numpy().reshape(N, L, -1)[valid0].std())
        print("  attention layer %d: pre-activation std %.3f" % (l, sd))
        assert 0.5 <= sd <= 3.0, (name, l, sd)
    wn = w.double().numpy().reshape(N, L)
    spreads = [wn[n][valid0[n]].std() / np.abs(wn[n][valid0[n]]).mean() for n in range(N) if valid0[n].sum() >= 2]
    if spreads:
        share = float((np.array(spreads) >= 0.2).mean())
        print("  instances with weight spread >= 0.2: %.0f %% of %d" % (100 * share, len(spreads)))
        assert share >= 0.5, (name, share)
    for mod in model.modules():      # the forwards above moved the running statistics: P0 carries them as constructed
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.reset_running_stats()
    P0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}

    model.zero_grad()
    o, a_out, a_w, _ = spied(model, feed(batches[0]))
    pred = o["prediction"]
    pred.retain_grad()
    loss = model.loss(o)
    loss.backward()
    out["att_out"], out["att_w"] = a_out.numpy().copy(), a_w.numpy().reshape(N, L).copy()
    out["pred"], out["loss"], out["gpred"] = pred.detach().numpy().copy(), np.float32(loss.item()), pred.grad.numpy().copy()
    for k, p in model.named_parameters():
        out["G/" + k] = p.grad.numpy().copy()
    out["zero_grad_keys"] = np.array(zero_grad_keys(model), dtype=str)

    if not NUMERIC:     # the reference's .float() calls stop a double run with numeric fields
        m64 = cls(args, corpus)
        m64.load_state_dict({k: torch.from_numpy(v) for k, v in P0.items()})
        m64 = m64.double()
        m64.zero_grad()
        o64, a_out64, a_w64, _ = spied(m64, feed(batches[0]))
        if ctr:     # CTRModel.loss casts the label to float32: nn.BCELoss spelled out for the double run
            loss64 = torch.nn.functional.binary_cross_entropy(o64["prediction"], o64["label"].double())
        else:
            loss64 = m64.loss(o64)
        loss64.backward()
        # a gradient that is exactly zero in exact arithmetic (a Linear bias in front of BatchNorm) is round-off on both sides: the
        # floor of 1e-6 of the largest gradient entry keeps its ratio meaningful (the tests compare with the same floor)
        floor = 1e-6 * max(float(p.grad.abs().max()) for p in m64.parameters())
        rel = lambda x, y, fl=0.0: float(np.abs(np.asarray(x, np.float64) - y).max() / max(np.abs(y).max(), fl, 1e-30))
        out["dev/att_out"] = np.float64(rel(out["att_out"], a_out64.numpy()))
        out["dev/att_w"] = np.float64(rel(out["att_w"], a_w64.numpy().reshape(N, L)))
        out["dev/pred"] = np.float64(rel(out["pred"], o64["prediction"].detach().numpy()))
        out["dev/loss"] = np.float64(abs(float(out["loss"]) - loss64.item()) / abs(loss64.item()))
        names = [k for k, _ in m64.named_parameters() if k not in zero_grad_keys(m64)]
        grads64 = dict((k, p.grad.numpy()) for k, p in m64.named_parameters())
        for k in names:
            out["dev/G/" + k] = np.float64(rel(out["G/" + k], grads64[k], floor))
        worst = max((out["dev/G/" + k], k) for k in names)
        print("  fp32 vs float64: att_out %.1e, pred %.1e, worst gradient %.1e (%s)" % (out["dev/att_out"], out["dev/pred"], *worst))

    opt_name, lr, l2 = opt
    m = cls(args, corpus)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P0.items()})
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
        out["{}/{}".format(opt_name, k)] = v.detach().numpy().copy()
    out[opt_name + "_losses"] = np.array(losses, dtype=np.float32)
    out[opt_name + "_hyper"] = np.array([lr, l2], dtype=np.float64)
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB")
    assert os.path.getsize(path) < (1 << 20), path


CASES = [
    # name,                                  mode,   d, att,          dnn,       L,  B,  K, fields,   hs, optimizer,             seed, users, items
    ("din_ctr_d4_a16_l1_b3",                "CTR",   4, [16],         [64],       1,  3, 0, IDS_ONLY, 0, ("SGD", 0.05, 1e-3),     71,  8, 10),   # the floor: H = 4, L = 1
    ("din_ctr_d64_a64x64_l40_b33",          "CTR",  64, [64, 64],     [64],      40, 33, 0, MIND_S,   0, ("Adam", 1e-3, 1e-4),    72,  8, 10),   # CTR_MIND.sh:24's layers, H = 192
    ("din_topk_d16_a64x64x64_l10_k4_b7_hs", "TopK", 16, [64, 64, 64], [128, 64], 10,  7, 4, GENERIC,  1, ("Adagrad", 0.01, 1e-4), 73, 40, 60),   # history situations: H = 64
    ("din_topk_d32_a256_l10_k1_b160",       "TopK", 32, [256],        [64, 64],  10, 160, 1, GENERIC, 0, ("SGD", 0.05, 1e-3),     74, 40, 60),   # H = 64
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    for c in CASES:
        print(c[0])
        make_case(a.out, *c)
