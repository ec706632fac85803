"""Golden vectors for KDA FROM THE REFERENCE ITSELF (models/sequential/KDA.py, helpers/KDAReader.py, utils/layers.py,
helpers/BaseRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kda.py [--out DIR] [--only model|kernel|reader|dataset]

Each kda_*.npz (one per entry of tests/kda_model_cases.py CASES, which also holds the args / corpus stand-ins) holds
  state_keys      the state_dict's keys in order (relational_dynamic_aggregation.relation_embeddings.weight, the second name of the
                  shared relation table, included)
  I0sha/<key>     SHA-256 of every tensor of the state_dict straight after construction under torch.manual_seed(seed): the init stream
  emb_scale, freq_scale     the float32 factors of tests/kda_model_cases.py scale_to_p0, which turns the constructed parameters into
                  P0, the parameters every computation below starts from
  b1/<f>, b2/<f>  two training batches: user_id, item_id, item_val, history_items (id 0 in the middle and as right padding; every
                  row keeps a valid position), history_delta_t (float64, as KDAReader.norm_time gives it; 0 in the first column),
                  lengths, head_id, tail_id, relation_id, value_id
  context         first batch: RelationalDynamicAggregation's output [B, C, R, V]
  pred, kg_pred, loss, G/<key>     first batch: both predictions, the loss, every parameter's gradient
  <opt>/<key>, <opt>_losses, <opt>_hyper     the state_dict after two optimizer steps from P0, the losses, (lr, l2)
  dev/context, dev/pred, dev/kg_pred, dev/loss, dev/G/<key>     the reference's own fp32 result against a float64 run of the same
                  modules (every .float() of the reference's forward turned into .double(), the frequency vector cast up), as largest
                  |difference| / largest |float64 entry| (gradients: the denominator is at least 1e-6 of the largest entry of any
                  gradient)
The generator asserts on the first batch of every case with L > 1: the aggregation's logits have a standard deviation in [1, 2]
over the valid positions, and the raw decays fall below 0, inside (0, 1) and above 1 for at least a tenth of the valid (b, l, r) each.

kda_kernel_dev.json: for every shape of tests/kda_data.py KERNEL_SHAPES and both include_val settings, the deviation of the reference's
fp32 RelationalDynamicAggregation (forward and autograd backward for kda_data's d_context) from its float64 run on kda_data's
arrays, per quantity, same measure; rows without a valid position are left out (the reference turns them into NaN).
kda_agg_<case>.npz: for the shapes small enough to commit, that float64 run's context and gradients themselves, and `keep`, the
rows that took part.

kda_reader.json: the reference KDAReader's n_dft, freq_x (real and imaginary parts) and interval counts on tests/slrc_data.py's corpus
(the one tests/golden/kg_reader.json describes) for --include_attr 0 and 1, --t_scalar 60, --n_dft 16.

kda_kg_dataset.npz: the reference's KDA.Dataset on both corpora under one numpy seed, with the item negative sampler replaced by
constants on both sides (stub_item_negatives): the sampled triplets (kg_data), negative heads and tails, and every training row's
item_val, history_delta_t, head_id, tail_id, relation_id and value_id.
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402  (numpy alias shim too)
import kda_data  # noqa: E402
import kda_model_cases as MC  # noqa: E402
import kda_np  # noqa: E402
import slrc_data  # noqa: E402

KG_SEED = 5          # tests/golden/make_golden_slrc.py's corpus
READER_FLAGS = ["--t_scalar", "60", "--n_dft", "16"]


def rel_err(x, y, floor=0.0):
    y = np.asarray(y, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - y).max() / max(np.abs(y).max(), floor, 1e-30))


class all_double:
    """inside: Tensor.float() gives float64 (the reference's forward casts delta_t and the decay to float32 by name)"""

    def __init__(self, torch):
        self.torch = torch

    def __enter__(self):
        self.plain = self.torch.Tensor.float
        self.torch.Tensor.float = lambda t, *a, **k: t.double()

    def __exit__(self, *exc):
        self.torch.Tensor.float = self.plain


def make_batches(rng, name):
    (n_users, n_items, n_ent, d, R, n_dft, L, B, K, *_rest) = MC.CASES[name]
    C = 1 + K

    def batch():
        item_val = np.zeros((B, C, R), dtype=np.int64)
        if R > 1 and n_ent > n_items:
            draw = rng.integers(n_items, n_ent, size=(B, C, R - 1))
            item_val[:, :, 1:] = np.where(rng.random((B, C, R - 1)) < 0.5, draw, 0)
        hist = kda_data.history(rng, B, L, n_items, empty_row=False)
        dt = rng.uniform(0., 20., size=(B, L))
        dt[:, 0] = 0.
        return {"user_id": rng.integers(1, n_users, size=B).astype(np.int64),
                "item_id": rng.integers(1, n_items, size=(B, C)).astype(np.int64), "item_val": item_val, "history_items": hist,
                "history_delta_t": dt, "lengths": (hist > 0).sum(axis=1).astype(np.int64),
                "head_id": rng.integers(1, n_items, size=(B, C)).astype(np.int64),
                "tail_id": rng.integers(1, n_ent, size=(B, C)).astype(np.int64),
                "relation_id": rng.integers(min(1, R - 1), R, size=B).astype(np.int64),
                "value_id": rng.integers(0, n_ent, size=B).astype(np.int64)}
    return [batch(), batch()]


def make_case(out_dir, name):
    torch, _, BaseRunner = make_golden._import_reference()
    from models.sequential.KDA import KDA
    torch.set_num_threads(1)   # one summation order for every rerun
    cfg = MC.CASES[name]
    (n_users, n_items, n_ent, d, R, n_dft, L, B, K, pooling, include_val, layers, heads, freq_rand, gamma, opt, seed) = cfg
    args, corpus = MC.stand_ins(name)
    torch.manual_seed(seed)
    model = KDA(args, corpus)
    out = {"state_keys": np.array(list(model.state_dict().keys()))}
    for k, v in model.state_dict().items():
        out["I0sha/" + k] = np.array(hashlib.sha256(v.detach().numpy().tobytes()).hexdigest())
    batches = make_batches(np.random.default_rng(seed), name)
    for n, b in enumerate(batches, 1):
        for k, v in b.items():
            out["b%d/%s" % (n, k)] = v

    def feed(b):
        f = {k: torch.from_numpy(v) for k, v in b.items()}
        f.update(batch_size=B, phase="train")
        return f

    def agg_inputs(m):
        b, E = batches[0], m.entity_embeddings.weight.detach().double().numpy()
        agg = m.relational_dynamic_aggregation
        return dict(seq=E[b["history_items"]], hist=b["history_items"], delta_t=b["history_delta_t"],
                    target=E[b["item_id"]], value=E[b["item_val"]], rel=m.relation_embeddings.weight.detach().double().numpy(),
                    freq_real=agg.freq_real.weight.detach().double().numpy(), freq_imag=agg.freq_imag.weight.detach().double().numpy())

    def logits_std(m):
        q = agg_inputs(m)
        rv = q["rel"][None, None] + q["value"] if include_val else np.broadcast_to(q["rel"][None, None], q["value"].shape)
        a = np.einsum("blv,bcrv->bclr", q["seq"], rv * q["target"][:, :, None, :])
        return float(a[np.broadcast_to((q["hist"] > 0)[:, None, :, None], a.shape)].std())

    def raw_decay(m):
        q = agg_inputs(m)
        return kda_np.decay_raw(q["delta_t"], q["freq_real"], q["freq_imag"])[0], q["hist"] > 0

    g = {"emb_scale": np.float32(1.0), "freq_scale": np.float32(1.0)}
    MC.scale_to_p0(model, g)
    sd = logits_std(model)
    emb_scale = np.float32((1.5 / sd) ** (1. / 3.)) if sd > 0 else np.float32(1.0)
    freq_scale = np.float32(1.0)
    if freq_rand:
        x, valid = raw_decay(model)
        freq_scale = np.float32(1.2 / x[np.broadcast_to(valid[:, :, None], x.shape)].std())
    # from the constructed parameters again, with the chosen factors: exactly what scale_to_p0 does in the tests
    torch.manual_seed(seed)
    model = KDA(args, corpus)
    out["emb_scale"], out["freq_scale"] = emb_scale, freq_scale
    MC.scale_to_p0(model, out)
    if L > 1:
        sd = logits_std(model)
        x, valid = raw_decay(model)
        shares = kda_data.clamp_shares(x, valid)
        print("  logits std %.3f; decays below 0 / inside / above 1: %.2f / %.2f / %.2f" % (sd, *shares))
        assert 1.0 <= sd <= 2.0, (name, sd)
        assert min(shares) >= 0.1, (name, shares)
    P0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}

    def run(m, fd):
        seen = {}
        h = m.relational_dynamic_aggregation.register_forward_hook(lambda _m, _i, o: seen.__setitem__("context", o.detach().clone()))
        m.zero_grad()
        o = m(fd)
        h.remove()
        loss = m.loss(o)
        loss.backward()
        return seen["context"], o, loss

    ctx, o, loss = run(model, feed(batches[0]))
    out["context"], out["pred"], out["kg_pred"] = ctx.numpy().copy(), o["prediction"].detach().numpy().copy(), \
        o["kg_prediction"].detach().numpy().copy()
    out["loss"] = np.float32(loss.item())
    for k, p in model.named_parameters():
        out["G/" + k] = p.grad.numpy().copy()
    # the second name of the shared table is no named_parameter: the test reads its gradient under the first
    assert "relational_dynamic_aggregation.relation_embeddings.weight" not in dict(model.named_parameters())

    m64 = KDA(args, corpus)
    m64.load_state_dict({k: torch.from_numpy(v) for k, v in P0.items()})
    m64 = m64.double()
    m64.relational_dynamic_aggregation.freqs = m64.relational_dynamic_aggregation.freqs.double()
    with all_double(torch):
        ctx64, o64, loss64 = run(m64, feed(batches[0]))
    assert ctx64.dtype == torch.float64 and o64["prediction"].dtype == torch.float64
    grads64 = {k: p.grad.numpy() for k, p in m64.named_parameters()}
    floor = 1e-6 * max(float(np.abs(v).max()) for v in grads64.values())
    out["dev/context"] = np.float64(rel_err(out["context"], ctx64.numpy()))
    out["dev/pred"] = np.float64(rel_err(out["pred"], o64["prediction"].detach().numpy()))
    out["dev/kg_pred"] = np.float64(rel_err(out["kg_pred"], o64["kg_prediction"].detach().numpy()))
    out["dev/loss"] = np.float64(abs(float(out["loss"]) - loss64.item()) / abs(loss64.item()))
    for k, v in grads64.items():
        out["dev/G/" + k] = np.float64(rel_err(out["G/" + k], v, floor))
    worst = max((float(out["dev/G/" + k]), k) for k in grads64)
    print("  fp32 vs float64: context %.1e, pred %.1e, loss %.1e, worst gradient %.1e (%s)" % (
        out["dev/context"], out["dev/pred"], out["dev/loss"], *worst))
    # the numpy restatement on the same inputs, here already: a generator that disagrees with it writes nothing
    q = agg_inputs(m64)
    assert rel_err(kda_np.forward(**q, include_val=bool(include_val)), ctx64.numpy()) < 1e-9, name

    opt_name, lr, l2 = opt
    m = KDA(args, corpus)
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


def make_kernel_devs(out_dir):
    torch, _, _ = make_golden._import_reference()
    from models.sequential.KDA import RelationalDynamicAggregation
    torch.set_num_threads(8)
    recorded = {}
    for shape in kda_data.KERNEL_SHAPES:
        B, C, L, R, V, F = shape
        q = kda_data.kernel_inputs(shape)
        keep = (q["hist"] > 0).any(axis=1)       # the reference gives NaN on a row without a valid position
        x = kda_np.decay_raw(q["delta_t"][keep], q["freq_real"], q["freq_imag"])[0]
        if L > 1:
            shares = kda_data.clamp_shares(x, q["hist"][keep] > 0)
            assert min(shares) >= 0.1, (shape, shares)
        for include_val in (1, 0):
            def run(dtype):
                t = lambda k, sel=True: torch.from_numpy(q[k][keep] if sel else q[k]).to(dtype)
                emb = torch.nn.Embedding(R, V).to(dtype)
                agg = RelationalDynamicAggregation(R, F, emb, include_val, torch.device("cpu")).to(dtype)
                with torch.no_grad():
                    emb.weight.copy_(t("rel", False))
                    agg.freq_real.weight.copy_(t("freq_real", False))
                    agg.freq_imag.weight.copy_(t("freq_imag", False))
                if dtype == torch.float64:
                    agg.freqs = agg.freqs.double()
                seq, target, value = (t(k).requires_grad_() for k in ("seq", "target", "value"))
                hist = torch.from_numpy(q["hist"][keep])
                valid_mask = (hist > 0).view(hist.shape[0], 1, L, 1)
                ctx = agg(seq, torch.from_numpy(q["delta_t"][keep]).to(dtype), target, value, valid_mask)
                ctx.backward(t("d_context"))
                res = {"context": ctx.detach().numpy(), "dseq": seq.grad.numpy(), "dtarget": target.grad.numpy(),
                       "drel": emb.weight.grad.numpy(), "dfreq_real": agg.freq_real.weight.grad.numpy(),
                       "dfreq_imag": agg.freq_imag.weight.grad.numpy()}
                if include_val:
                    res["dvalue"] = value.grad.numpy()
                return res
            r32 = run(torch.float32)
            with all_double(torch):
                r64 = run(torch.float64)
            assert r64["context"].dtype == np.float64
            args64 = {k: (q[k][keep] if k in ("seq", "hist", "delta_t", "target", "value") else q[k]) for k in kda_data.ARG_ORDER}
            assert rel_err(kda_np.forward(**args64, include_val=bool(include_val)), r64["context"]) < 1e-9, shape
            mine = kda_np.backward(**args64, d_context=q["d_context"][keep], include_val=bool(include_val))
            for k in kda_data.GRADS:
                if k in r64:
                    assert rel_err(mine[k], r64[k]) < 1e-8, (shape, k, rel_err(mine[k], r64[k]))
            name = kda_data.case_name(shape, include_val)
            recorded[name] = {k: rel_err(r32[k], r64[k]) for k in r64}
            print(name, " ".join("%s %.1e" % kv for kv in recorded[name].items()))
            if B * C * R * V <= 5000:     # small enough to commit: the float64 results themselves, for tests/kda_np.py
                np.savez_compressed(os.path.join(out_dir, "kda_agg_%s.npz" % name), keep=keep, **r64)
    path = os.path.join(out_dir, "kda_kernel_dev.json")
    with open(path, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
    print("wrote", path)


def make_reader_golden(out_dir):
    make_golden._import_reference()
    from helpers.KDAReader import KDAReader
    recorded = {}
    for include_attr in (0, 1):
        root = tempfile.mkdtemp(prefix="kda_golden_")
        slrc_data.make_kg_dataset(root, "synth_kg", seed=KG_SEED)
        p = KDAReader.parse_data_args(argparse.ArgumentParser())
        a, _ = p.parse_known_args(["--path", root + "/", "--dataset", "synth_kg", "--include_attr", str(include_attr)] + READER_FLAGS)
        a.regenerate = 0
        plain = KDAReader._cal_freq_x
        counts = {}

        def spy(self):
            counts.update({k: [len(v), int(np.sum(v))] for k, v in self.interval_dict.items()})
            return plain(self)
        KDAReader._cal_freq_x = spy
        corpus = KDAReader(a)
        KDAReader._cal_freq_x = plain
        recorded["include_attr_%d" % include_attr] = {
            "n_dft": int(corpus.n_dft), "t_scalar": int(corpus.t_scalar), "relations": list(corpus.relations),
            "interval_counts": counts,       # name -> [number of intervals, their sum]
            "freq_x_real": np.real(corpus.freq_x).tolist(), "freq_x_imag": np.imag(corpus.freq_x).tolist()}
    path = os.path.join(out_dir, "kda_reader.json")
    with open(path, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB")


def stub_item_negatives(GeneralModel, n_neg):
    """the item negative sampler draws in another order here than in the reference (vectorised rejection sampling): both sides
    replace it by constant negatives, so that the numpy stream reaches the knowledge-graph sampling in the same state"""
    GeneralModel.Dataset.actions_before_epoch = lambda self: self.data.__setitem__(
        "neg_items", np.ones((len(self), n_neg), dtype=int))


def make_dataset_golden(out_dir):
    """kda_kg_dataset.npz: the reference KDA.Dataset on the --include_attr 0 and 1 corpora under np.random.seed(DATASET_SEED)"""
    from types import SimpleNamespace
    make_golden._import_reference()
    from helpers.KDAReader import KDAReader
    from models.BaseModel import GeneralModel
    from models.sequential.KDA import KDA
    plain = GeneralModel.Dataset.actions_before_epoch
    out = {}
    for include_attr in (0, 1):
        root = tempfile.mkdtemp(prefix="kda_golden_")
        slrc_data.make_kg_dataset(root, "synth_kg", seed=KG_SEED)
        p = KDAReader.parse_data_args(argparse.ArgumentParser())
        a, _ = p.parse_known_args(["--path", root + "/", "--dataset", "synth_kg", "--include_attr", str(include_attr)] + READER_FLAGS)
        a.regenerate = 0
        corpus = KDAReader(a)
        model = SimpleNamespace(test_all=0, buffer=0, history_max=4, num_neg=3, neg_head_p=0.5)
        stub_item_negatives(GeneralModel, 3)
        try:
            np.random.seed(MC.DATASET_SEED)
            train = KDA.Dataset(model, corpus, "train")
            train.actions_before_epoch()
            feeds = [train._get_feed_dict(k) for k in range(len(train))]
        finally:
            GeneralModel.Dataset.actions_before_epoch = plain
        pre = "attr%d/" % include_attr
        out[pre + "kg_data"] = train.kg_data[["head", "relation", "tail", "value"]].values.astype(np.int64)
        out[pre + "neg_heads"], out[pre + "neg_tails"] = train.neg_heads.astype(np.int64), train.neg_tails.astype(np.int64)
        out[pre + "item_val"] = np.array([f["item_val"] for f in feeds], dtype=np.int64)
        out[pre + "history_delta_t"] = np.concatenate([f["history_delta_t"] for f in feeds])
        out[pre + "head_id"] = np.stack([f["head_id"] for f in feeds]).astype(np.int64)
        out[pre + "tail_id"] = np.stack([f["tail_id"] for f in feeds]).astype(np.int64)
        out[pre + "relation_value"] = np.array([[f["relation_id"], f["value_id"]] for f in feeds], dtype=np.int64)
        assert (out[pre + "kg_data"][:, 3] > 0).any() == bool(include_attr)
    path = os.path.join(out_dir, "kda_kg_dataset.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    if a.only in ("", "reader"):
        make_reader_golden(a.out)
    if a.only in ("", "dataset"):
        make_dataset_golden(a.out)
    if a.only in ("", "model"):
        for c in MC.CASES:
            print(c)
            make_case(a.out, c)
    if a.only in ("", "kernel"):
        make_kernel_devs(a.out)
