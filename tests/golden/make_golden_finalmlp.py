"""Golden vectors for FinalMLP FROM THE REFERENCE ITSELF (models/context/FinalMLP.py, utils/layers.py, helpers/BaseRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_finalmlp.py [--out DIR]

Each finalmlp_*.npz holds
  config          JSON: the model flags, the corpus' feature names and feature_max, B, C, seed, ctr
  state_keys      the state_dict's keys in order
  I0/<key>        the state_dict straight after construction under torch.manual_seed(seed): pins the init stream
  P0/<key>        the parameters every computation below starts from.  Untrained parameters leave every gate at 1 +- 0.01 and the loss
                  at ln 2, so after construction: every parameter x 20; the context biases (zero) drawn from N(0, 1); on the first
                  batch the gate's last Linear (weight and bias) scaled to a logit standard deviation of 1.5, w_xy scaled so the
                  bilinear term's standard deviation equals the linear terms', and (CTR) w_x, w_y, w_xy and the two biases scaled
                  together to a pre-sigmoid standard deviation of 1.5 and w_x's bias shifted to a pre-sigmoid mean of 0
                  (the streams' outputs are post-ReLU, so the untouched mean alone saturates the sigmoid)
  b1/<f>, b2/<f>  two training batches (ids, features, label for CTR)
  gate1, gate2    (use_fs) the gates 2 sigmoid(.) on the first batch [B, C, D];  A1, A2: the first layer's output of both streams
  pred, loss, gpred, G/<key>     first batch: prediction, loss, d loss / d prediction, every parameter's gradient
  <opt>/<key>, <opt>_losses, <opt>_hyper     parameters after two optimizer steps from P0, the two losses, (lr, l2)
  dev/<key>, dev/pred            cases without numeric fields (the reference's .float() calls stop a double run with them): the
                                 reference's own fp32 result against a float64 run of the same modules driven by the stored gpred,
                                 as largest |difference| / largest |float64 entry|
The generator asserts, per case: at least 30 % of each stream's gate values outside [0.5, 1.5]; between 20 % and 80 % of each
stream's output positive; the bilinear term's standard deviation at least half the linear terms'; CTR: at least 80 % of the
probabilities in (0.02, 0.98).
"""
import argparse
import copy
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (numpy alias shim too)
sys.path.insert(0, os.path.dirname(HERE))
import finalmlp_np  # noqa: E402

SMALL = {"i_category_c": 6, "i_subcategory_c": 12, "c_hour_c": 8, "c_period_c": 4, "c_weekday_c": 7}
MIND_S = dict(item=["i_category_c", "i_subcategory_c"], sit=["c_day_f", "c_hour_c", "c_period_c", "c_weekday_c"], vocab=SMALL,
              numeric={"c_day_f": ("int64", 7)})
CAT = dict(item=["i_category_c"], sit=["c_hour_c", "c_weekday_c"], vocab=SMALL, numeric={})
FLOOR = dict(item=[], sit=["c_hour_c"], vocab=SMALL, numeric={})
MIND_FS1, MIND_FS2 = "c_hour_c,c_weekday_c,c_period_c,c_day_f", "i_category_c,i_subcategory_c"


def make_case(out_dir, name, mode, d, mlp1, mlp2, fs, heads, fs1, fs2, use_fs, B, K, spec, opts, seed, n_users, n_items):
    torch, _, BaseRunner = make_golden._import_reference()
    from models.context.FinalMLP import FinalMLPCTR, FinalMLPTopK
    torch.set_num_threads(1)   # one summation order for every rerun
    ctr = mode == "CTR"
    cls = FinalMLPCTR if ctr else FinalMLPTopK
    ITEM, SIT, VOC, NUMERIC = spec["item"], spec["sit"], spec["vocab"], spec["numeric"]
    rng = np.random.default_rng(seed)
    flags = dict(emb_size=d, mlp1_hidden_units=str(mlp1), mlp1_hidden_activations="ReLU", mlp1_dropout=0, mlp1_batch_norm=0,
                 mlp2_hidden_units=str(mlp2), mlp2_hidden_activations="ReLU", mlp2_dropout=0, mlp2_batch_norm=0, use_fs=use_fs,
                 fs_hidden_units=str(fs), fs1_context=fs1, fs2_context=fs2, num_heads=heads, loss_n="BCE" if ctr else "BPR")
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=K, dropout=0, test_all=0, **flags)
    fmax = {f: VOC[f] for f in ITEM + SIT if f in VOC}
    fmax.update(user_id=n_users, item_id=n_items)
    for f, (_, top) in NUMERIC.items():     # helpers/ContextReader.py:52-53 records max + 1 for every feature; unused for '*_f'
        fmax[f] = top
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, user_feature_names=[], item_feature_names=ITEM,
                             situation_feature_names=SIT, feature_max=fmax)
    torch.manual_seed(seed)
    model = cls(args, corpus)
    C = 1 if ctr else 1 + K
    config = dict(flags=flags, item=ITEM, sit=SIT, feature_max={k: int(v) for k, v in fmax.items()}, n_users=n_users, n_items=n_items,
                  B=B, C=C, seed=seed, ctr=ctr, num_neg=K, context_features=list(model.context_features))
    out = {"config": np.array(json.dumps(config)), "state_keys": np.array(list(model.state_dict().keys()))}
    for k, v in model.state_dict().items():
        out["I0/" + k] = v.detach().numpy().copy()

    def column(f, size):
        if f not in NUMERIC:
            return rng.integers(0, VOC[f], size=size).astype(np.int64)
        return rng.integers(0, NUMERIC[f][1], size=size).astype(np.int64)

    item_cols = {f: column(f, n_items) for f in ITEM}     # item_meta: one value per item

    def batch():
        b = {"user_id": rng.integers(1, n_users, size=B).astype(np.int64),
             "item_id": rng.integers(1, n_items, size=(B, C)).astype(np.int64)}
        b["item_id"][:, 0] = b["item_id"][:, 0] % 5 + 1  # duplicates
        for f in SIT:
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

    def parts(m, fd):
        """FinalMLP.py:77-102 spelled out on the reference's own modules -> dict of the intermediate tensors"""
        user_emb = m.embedding_dict['user_id'](fd['user_id']).unsqueeze(1).unsqueeze(1)
        emb = lambda f: m.embedding_dict[f](fd[f]) if (f.endswith('_c') or f.endswith('_id')) else m.embedding_dict[f](fd[f].float().unsqueeze(-1))
        item_emb = torch.stack([emb(f) for f in m.context_features if f == 'item_id' or f.startswith('i_')], dim=-2)
        sit = torch.stack([emb(f) for f in m.context_features if f.startswith('c_')], dim=-2).unsqueeze(1)
        n = item_emb.shape[1]
        flat = torch.cat([user_emb.repeat(1, n, 1, 1), item_emb, sit.repeat(1, n, 1, 1)], dim=-2).flatten(start_dim=-2)
        r = {"flat": flat}
        if m.use_fs:
            feat1, feat2 = m.fs_module(fd, flat)
            gates = []
            for s in (1, 2):      # the gate and its logits: fs_module.forward's lines with the Sigmoid taken off
                ctxs = getattr(m.fs_module, "fs%d_context" % s)
                if len(ctxs) == 0:
                    z = getattr(m.fs_module, "fs%d_ctx_bias" % s).unsqueeze(1).repeat(flat.size(0), flat.size(1), 1)
                else:
                    zs = []
                    for i, ctx in enumerate(ctxs):
                        e = getattr(m.fs_module, "fs%d_ctx_emb" % s)[i]
                        v = e(fd[ctx]) if ctx.endswith('_c') else e(fd[ctx].float().unsqueeze(-1))
                        zs.append(v.unsqueeze(1).repeat(1, flat.size(1), 1) if v.dim() == 2 else v)
                    z = torch.cat(zs, dim=-1)
                gate = getattr(m.fs_module, "fs%d_gate" % s)
                logits = gate.mlp[:-1](z)
                r["logit%d" % s], r["gate%d" % s] = logits, gate(z) * 2
                gates.append(r["gate%d" % s])
            assert torch.equal(feat1, flat * gates[0]) and torch.equal(feat2, flat * gates[1])
        else:
            feat1, feat2 = flat, flat
        Bn = flat.shape[0]
        r["A1"] = m.mlp1.mlp[:2](feat1.view(-1, feat1.shape[-1])).view(Bn, n, -1)
        r["A2"] = m.mlp2.mlp[:2](feat2.view(-1, feat2.shape[-1])).view(Bn, n, -1)
        r["x"] = m.mlp1(feat1.view(-1, feat1.shape[-1])).view(Bn, n, -1)
        r["y"] = m.mlp2(feat2.view(-1, feat2.shape[-1])).view(Bn, n, -1)
        fm = m.fusion_module
        r["lin"] = (fm.w_x(r["x"]) + fm.w_y(r["y"])).squeeze(-1)
        r["logit"] = fm(r["x"], r["y"])
        r["bil"] = r["logit"] - r["lin"]
        return r

    fd1 = feed(batches[0])
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(20.0)
        if model.use_fs:
            for s in (1, 2):
                bias = getattr(model.fs_module, "fs%d_ctx_bias" % s, None)
                if bias is not None:
                    bias.copy_(torch.randn(bias.shape))
            for s in (1, 2):
                last = [mod for mod in getattr(model.fs_module, "fs%d_gate" % s).mlp if isinstance(mod, torch.nn.Linear)][-1]
                lg = parts(model, fd1)["logit%d" % s]
                sd = lg.double().std().item() if lg.numel() > 1 else 1.5
                sc = float(np.float32(1.5 / sd))
                last.weight.mul_(sc)
                last.bias.mul_(sc)
        r = parts(model, fd1)
        fm = model.fusion_module
        fm.w_xy.mul_(float(np.float32(r["lin"].double().std().item() / max(r["bil"].double().std().item(), 1e-30))))
        if ctr:
            sc = float(np.float32(1.5 / parts(model, fd1)["logit"].double().std().item()))
            for p in (fm.w_xy, fm.w_x.weight, fm.w_x.bias, fm.w_y.weight, fm.w_y.bias):
                p.mul_(sc)
            fm.w_x.bias.sub_(float(np.float32(parts(model, fd1)["logit"].double().mean().item())))      # post-ReLU inputs: centre it
        r = parts(model, fd1)
    P0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    for k, v in P0.items():
        out["P0/" + k] = v
    if model.use_fs:
        for s in (1, 2):
            g = r["gate%d" % s].numpy()
            share = float(((g < 0.5) | (g > 1.5)).mean())
            assert share >= 0.3, (name, s, share)
            out["gate%d" % s] = g.copy()
            print("  gate %d: logit std %.2f, outside [0.5, 1.5]: %.0f %%" % (s, r["logit%d" % s].std().item(), 100 * share))
    for s, key in ((1, "x"), (2, "y")):
        active = float((r[key] > 0).float().mean())
        assert 0.2 <= active <= 0.8, (name, key, active)
        out["A%d" % s] = r["A%d" % s].numpy().copy()
        print("  stream %d: positive outputs %.0f %%" % (s, 100 * active))
    ratio = r["bil"].std().item() / r["lin"].std().item()
    assert ratio >= 0.5, (name, ratio)
    print("  std(bilinear) / std(linear) = %.2f" % ratio)

    model.zero_grad()
    o = model(fd1)
    pred = o["prediction"]
    pred.retain_grad()
    loss = model.loss(o)
    loss.backward()
    out["pred"], out["loss"], out["gpred"] = pred.detach().numpy().copy(), np.float32(loss.item()), pred.grad.numpy().copy()
    if ctr:
        p_ = out["pred"]
        share = float(((p_ > 0.02) & (p_ < 0.98)).mean())
        assert share >= 0.8, (name, share)
        print("  probabilities in (0.02, 0.98): %.0f %%, loss %.4f" % (100 * share, out["loss"]))
    for k, p in model.named_parameters():
        out["G/" + k] = p.grad.numpy().copy()

    if not NUMERIC:
        m64 = copy.deepcopy(model).double()
        m64.zero_grad()
        ref_pred = m64(fd1)["prediction"]
        ref_pred.backward(torch.from_numpy(out["gpred"]).double().view_as(ref_pred))
        scale = ref_pred.detach().abs().max().item()
        out["dev/pred"] = np.float64((torch.from_numpy(out["pred"]).double().view(-1) - ref_pred.detach().view(-1)).abs().max().item() / scale)
        floor = finalmlp_np.grad_floor(out)
        for k, p in m64.named_parameters():
            out["dev/" + k] = np.float64(finalmlp_np.rel_err(out["G/" + k], p.grad.numpy(), floor))
        print("  fp32 vs float64: pred %.1e, worst gradient %.1e" % (out["dev/pred"], max(out["dev/" + k] for k, _ in m64.named_parameters())))

    for opt_name, lr, l2 in opts:
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
    assert os.path.getsize(path) <= 512 * 1024, name


ADAM = (("Adam", 1e-3, 1e-4),)
ADAM_SGD = (("Adam", 1e-3, 1e-4), ("SGD", 0.05, 1e-3))
CASES = [
    # name, mode, d, mlp1, mlp2, fs, heads, fs1, fs2, use_fs, B, K, fields, optimizers, seed, users, items
    ("finalmlp_mind_ctr_d8", "CTR", 8, [64], [32], [64], 1, MIND_FS1, MIND_FS2, 1, 48, 0, MIND_S, ADAM, 71, 8, 10),
    ("finalmlp_topk_d16_h2_k3", "TopK", 16, [16, 16, 16], [16, 16, 16], [16], 2, "", "", 1, 24, 3, CAT, ADAM_SGD, 72, 40, 60),
    ("finalmlp_topk_d8_h4_ctx", "TopK", 8, [16], [32, 8], [24, 12], 4, "c_hour_c", "i_category_c", 1, 24, 3, CAT, ADAM, 73, 40, 60),
    ("finalmlp_ctr_nofs", "CTR", 8, [32, 16], [16], [64], 2, "", "", 0, 33, 0, CAT, ADAM, 74, 8, 10),
    ("finalmlp_topk_floor_d4", "TopK", 4, [4], [4], [4], 1, "", "c_hour_c", 1, 24, 3, FLOOR, ADAM, 75, 40, 60),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    for c in CASES:
        print(c[0])
        make_case(a.out, *c)
