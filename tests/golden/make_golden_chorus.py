"""Golden vectors for Chorus FROM THE REFERENCE ITSELF (models/sequential/Chorus.py, helpers/KGReader.py, the optimizer construction
of helpers/BaseRunner.py), on CPU with one thread.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_chorus.py [--out DIR] [--tolerances FILE]

The reference's constructor wants the pre-trained file for --stage 2; the generator builds every model with --stage 1 (which only
sets a path) and then sets `stage` on the object, which is all forward, loss and customize_parameters read.

Each chorus_d*.npz (stage 2) holds
  meta [n_users, n_items, n_cat, d, R, B, K, seed, redraw, gmf], hyper [lr, l2, lr_scale], opt (name), relations (the r_* column names)
  <P>0 for the nine parameters P of tests/chorus_np.py's PARAMS: what every computation below starts from -- what Chorus.__init__
                           leaves after torch.manual_seed(seed) (redraw = 0: normal(0, 0.01), the demo flags), or (redraw = 1) re-drawn
                           wider: with the native init every score is ~1e-3 and the category tables' gradients ~1e-6
  uid, iid, cid, intervals one training batch: users [B], candidates and their categories [B, 1 + K], relational_interval [B, 1 + K, R]
  pred, loss, G<P>         Chorus.forward's prediction, GeneralModel.loss and the dense gradients (a parameter the head does not read has
                           none: has_grad, PARAMS order -- prediction.weight under BPR, the biases under GMF, and sigmas and mus
                           where no relation is a 'substitute' one)
  <P>2                     the parameters after TWO steps of the torch.optim optimizer BaseRunner builds from customize_parameters
                           (dense semantics: weight decay and Adam's moments reach every row)
  pred64 (the first 16 tuples), loss64, G<P>64, <P>2_64     the reference's own float64 run of the same case; for the two wide
                           tables U and I only the deviations below are kept
  dev_*                    per array, the smallest rtol = atol_scale that holds the fp32 run to the float64 one (the tests allow the
                           larger of 2e-5 and four times this)
  ub_ratio                 max|Guser_bias| / max|Gitem_bias| (BPR): 0 in exact arithmetic, asserted below 1e-5
  special                  rows (category, relation, kind): betas + 1 below 1e-10 / exactly 10 / above 10 (0 / 1 / 2), the same for
                           sigmas + 1 (3 / 4 / 5, on 'substitute' relations, whose kernel alone reads sigma), betas + 1 = 0.2 on a
                           'substitute' relation with an interval of 0 (6: the unclamped kernel value falls below -1)
  state_keys, model_flags, reader_flags, groups (JSON: the parameter names, lr and weight decay of the three groups)
Ids are Zipf-distributed over small tables.  Set by hand: a negative equal to the positive, a candidate repeated inside a tuple, a
tuple whose intervals are all -1, an interval of exactly 0, the clamp entries above.  Asserted, so that no test excludes anything:
every gradient is finite; every unmasked kernel value of the float64 restatement lies at least 1e-3 from +-1 (fp32 evaluates it to a
few 1e-7 relative, so it is on the same side there); every betas + 1 / sigmas + 1 is exactly on a bound or at least 1e-3 from it;
every hand-set clamp entry is read by an unmasked kernel value inside [-1, 1]; a kernel value beyond -1 (entry 6) and one beyond +1
occur in every case with item relations and re-drawn parameters.  The seed is advanced until that holds.

chorus_kg_stage1.npz: one stage-1 batch: head_id / tail_id / relation_id [B, 4] in the reference's feed layout with repeats, pred,
loss, GI, GRel, I1 / Rel1 / I2 / Rel2, x64 (the float64 hinge arguments); only seeds where no hinge differs between fp32 and float64
outside exact ties are kept.
chorus_kg_dataset.npz: the reference Dataset on tests/slrc_data.py's corpus: category_id and relational_interval for every train row
(fixed negatives) and the first dev rows; the stage-1 negatives of two epochs after np.random.seed(s).
"""
import argparse
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import chorus_np  # noqa: E402
import make_golden  # noqa: E402
import slrc_data  # noqa: E402
from chorus_np import PARAMS, STATE_KEYS  # noqa: E402

KG_SEED, SAMPLE_SEED, KG_TIME_SCALAR, KG_DEV_ROWS = 5, 11, 100000, 8
TOL_LINES = []


def _flags(add):
    p = argparse.ArgumentParser()
    before = {s for a in p._actions for s in a.option_strings}
    p = add(p)
    return np.array(sorted({s for a in p._actions for s in a.option_strings} - before))


def _needed(got, want):
    """the smallest rtol = atol_scale with |got - want| <= rtol |want| + atol_scale max|want| everywhere"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    den = np.abs(want) + np.abs(want).max()
    return float(np.max(np.abs(got - want) / np.where(den > 0, den, 1.0)))


def _reference():
    import pandas as pd
    torch, _, BaseRunner = make_golden._import_reference()
    from helpers.KGReader import KGReader
    from models.sequential.Chorus import Chorus
    torch.set_num_threads(1)   # one summation order for every rerun
    return torch, pd, BaseRunner, KGReader, Chorus


def _args(torch, d, K, base, lr, lr_scale, margin=1.0, time_scalar=8640000, history_max=20):
    return SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=K, dropout=0, test_all=0, emb_size=d,
                           history_max=history_max, time_scalar=time_scalar, stage=1, base_method=base, category_col="i_category",
                           lr_scale=lr_scale, margin=margin, lr=lr)


def try_case(name, n_users, n_items, n_cat, d, relations, B, K, opt, lr, l2, lr_scale, seed, redraw, base):
    torch, pd, BaseRunner, KGReader, Chorus = _reference()
    rng = np.random.default_rng(seed)
    R, gmf = len(relations) + 1, base == "GMF"
    kinds = chorus_np.kinds_of(relations)
    meta = {"item_id": np.arange(1, n_items)}
    if n_cat > 1:
        cats = rng.integers(0, n_cat, n_items - 1)
        cats[0] = n_cat - 1
        meta["i_category"] = cats
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, item_relations=list(relations), item_meta_df=pd.DataFrame(meta),
                             dataset="golden")
    args = _args(torch, d, K, base, lr, lr_scale)
    item2cate = dict(zip(meta["item_id"], meta["i_category"])) if n_cat > 1 else {}

    def zipf(n, size):
        p = 1.0 / np.arange(1, n)
        return rng.choice(np.arange(1, n), size=size, p=p / p.sum()).astype(np.int64)

    uid, iid = zipf(n_users, B), zipf(n_items, (B, 1 + K))
    if K >= 2:
        iid[0, 1] = iid[0, 0]          # a negative equals the positive
        iid[0, 2] = iid[0, 1]          # ... and a candidate repeats inside the tuple
    cid = np.vectorize(lambda i: item2cate.get(i, 0))(iid).astype(np.int64)
    iv = np.where(rng.random((B, 1 + K, R)) < 0.4, -1.0, rng.uniform(0.0, 3.0, (B, 1 + K, R))).astype(np.float32)
    iv[:, :, 0] = -1.0                 # entry 0 is always -1 in the Dataset's feed ...
    if R == 1 or rng.random() < 0.5:
        iv[0, 0, 0] = 0.7              # ... the head itself takes any: one case in two feeds it a value
    dead = B - 1 if B > 1 else None    # a tuple whose intervals are all -1 (B = 1: one candidate's)
    if dead is None:
        iv[0, 1, :] = -1.0
    else:
        iv[dead] = -1.0
    if R > 1:
        iv[0, 0, 1] = 0.0              # an interval of exactly 0

    drawn = {}
    if redraw:
        sd = {"U": 0.3, "I": 0.3, "Rel": 0.3, "w": 0.7, "user_bias": 0.3, "item_bias": 0.3, "betas": 0.3, "sigmas": 0.2, "mus": 0.5}
        shape = {"U": (n_users, d), "I": (n_items, d), "Rel": (R, d), "w": (1, d), "user_bias": (n_users, 1), "item_bias": (n_items, 1)}
        for k in PARAMS:
            drawn[k] = (sd[k] * rng.standard_normal(shape.get(k, (n_cat, R)))).astype(np.float32)
    # the clamp entries, on (category, relation) slots that occur in the batch outside the dead tuple.  A value is placed where the
    # head READS it: the three sigma entries and the betas + 1 = 0.2 entry on 'substitute' relations (the only kernel that reads
    # sigma, and the only one that can fall below -1), the three beta entries on any item relation
    live_c = cid if dead is None else cid[:dead]
    cats = [int(c) for c in np.unique(live_c)]
    values = [("betas", -1.5), ("betas", 9.0), ("betas", 11.0), ("sigmas", -1.5), ("sigmas", 9.0), ("sigmas", 11.0), ("betas", -0.8)]
    special = []
    if redraw and R > 1:
        sub_slots = [(c, r) for c in cats for r in range(1, R) if kinds[r] == 2]
        assert len(sub_slots) >= 4, name
        chosen = {3 + j: sub_slots[(j * len(sub_slots)) // 4] for j in range(4)}      # kinds 3, 4, 5 (sigmas) and 6
        rest = [(c, r) for c in cats for r in range(1, R) if (c, r) not in chosen.values()]
        assert len(rest) >= 3, name
        chosen.update({j: rest[(j * len(rest)) // 3] for j in range(3)})               # kinds 0, 1, 2 (betas)
        for kind in range(7):
            cat, r = chosen[kind]
            where = [(b, c) for b, c in np.argwhere(live_c == cat) if (b, c) != (0, 0)]     # (0, 0) holds the hand-set interval of 0
            if not where:
                return None
            b, c = where[0]
            special.append((cat, r, kind))
            iv[b, c, r] = 0.0 if kind == 6 else 0.7      # the entry takes part in a score

    def build(double=False):
        torch.manual_seed(seed)
        model = Chorus(args, corpus)
        model.stage = 2
        with torch.no_grad():
            sd_ = model.state_dict()
            for k, v in drawn.items():
                sd_[STATE_KEYS[k]].copy_(torch.from_numpy(v))
            for (cat, r, kind) in special:
                table, val = values[kind]
                sd_[STATE_KEYS[table]][cat, r] = val
        return model.double() if double else model

    def snapshot(model, tag, out):
        sd_ = model.state_dict()
        for k in PARAMS:
            out[k + tag] = sd_[STATE_KEYS[k]].detach().numpy().copy()

    def feed_of(dtype):
        return {"user_id": torch.from_numpy(uid), "item_id": torch.from_numpy(iid), "category_id": torch.from_numpy(cid),
                "relational_interval": torch.from_numpy(iv.astype(dtype)), "batch_size": B, "phase": "train"}

    out = {"meta": np.array([n_users, n_items, n_cat, d, R, B, K, seed, int(redraw), int(gmf)], dtype=np.int64),
           "hyper": np.array([lr, l2, lr_scale], dtype=np.float64), "opt": np.array(opt), "relations": np.array(list(relations), dtype=str),
           "special": np.array(special, dtype=np.int64).reshape(-1, 3), "uid": uid, "iid": iid, "cid": cid, "intervals": iv}
    model = build()
    snapshot(model, "0", out)
    P0 = {k: out[k + "0"] for k in PARAMS}

    # the conditions on the case itself, from the float64 restatement of the kernels
    _, kappa, _ = chorus_np.kernels(chorus_np.f64(P0), cid, iv, kinds)
    on = iv >= 0
    if on.any() and np.abs(np.abs(kappa[on]) - 1.0).min() < 1e-3:
        return None
    for t in ("betas", "sigmas"):
        x = P0[t].astype(np.float64) + 1.0
        for bound in (1e-10, 10.0):
            if ((x != bound) & (np.abs(x - bound) < 1e-3)).any():
                return None
    if special:
        # every hand-set clamp entry is read by an unmasked, unclamped kernel value, so its gate decides a gradient the reference
        # records; the betas + 1 = 0.2 entry pushes the substitute kernel below -1 at an interval of 0, a complement or
        # exponential entry elsewhere in the batch may or may not exceed +1 (the seed is advanced until one does)
        for cat, r, kind in special:
            hit = on[:, :, r] & (cid == cat)
            assert hit.any() and kinds[r] == (2 if kind >= 3 else kinds[r]), (name, cat, r, kind)
            if kind < 6:
                assert (np.abs(kappa[:, :, r][hit]) <= 1.0).any(), (name, cat, r, kind)
        cat, r, _ = special[6]
        assert (kappa[:, :, r][on[:, :, r] & (cid == cat) & (iv[:, :, r] == 0)] < -1).any(), name
        if not (kappa[on] > 1).any():
            return None

    def run(m, dtype):
        res = {}
        feed = feed_of(dtype)
        m.zero_grad()
        o = m(feed)
        loss = m.loss(o)
        loss.backward()
        res["pred"], res["loss"] = o["prediction"].detach().numpy().copy(), loss.item()
        named = dict(m.named_parameters())
        for k in PARAMS:
            g = named[STATE_KEYS[k]].grad
            res["G" + k] = None if g is None else g.numpy().copy()
        return res

    r32, r64 = run(model, np.float32), run(build(double=True), np.float64)
    out["pred"], out["loss"] = r32["pred"], np.array(r32["loss"], dtype=np.float32)
    out["pred64"], out["loss64"] = r64["pred"], np.array(r64["loss"], dtype=np.float64)
    assert np.isfinite(out["pred"]).all() and np.isfinite(out["loss"])
    has_grad, devs = [], {"pred": _needed(r32["pred"], r64["pred"]), "loss": abs(r32["loss"] - r64["loss"]) / max(abs(r64["loss"]), 1e-30)}
    for k in PARAMS:
        g = r32["G" + k]
        has_grad.append(g is not None)
        assert (g is None) == (r64["G" + k] is None)
        if g is None:
            continue
        assert np.isfinite(g).all() and np.isfinite(r64["G" + k]).all(), (name, k)
        out["G" + k], out["G" + k + "64"] = g, r64["G" + k]
        if k != "user_bias":
            devs["G" + k] = _needed(g, r64["G" + k])
    sub = 2 in kinds      # sigmas and mus are read by the 'substitute' kernel alone
    assert has_grad == [True] * 4 + [sub, sub, gmf, not gmf, not gmf], (name, has_grad)
    out["has_grad"] = np.array(has_grad)
    if not gmf:
        # sum_c d loss / d pred[b, c] = 0 in exact arithmetic: what the reference records for user_bias is round-off
        ratio = np.abs(out["Guser_bias"]).max() / np.abs(out["Gitem_bias"]).max()
        assert ratio < 1e-5, (name, ratio)
        out["ub_ratio"] = np.array([ratio, np.abs(out["Guser_bias64"]).max() / np.abs(out["Gitem_bias64"]).max()])

    def two_steps(m, dtype, tags):
        runner = BaseRunner(make_golden._runner_args(BaseRunner, opt, lr, l2))
        m.optimizer = runner._build_optimizer(m)
        m.train()
        feed = feed_of(dtype)
        for tag in tags:
            m.optimizer.zero_grad()
            m.loss(m(feed)).backward()
            m.optimizer.step()
            if tag:
                snapshot(m, tag, out)
        return m

    m = two_steps(build(), np.float32, ("1", "2"))
    two_steps(build(double=True), np.float64, ("", "2_64"))
    for k in PARAMS:
        assert np.isfinite(out[k + "2"]).all(), (name, k)
        if k != "user_bias":
            devs[k + "2"] = _needed(out[k + "2"] - out[k + "0"], out[k + "2_64"] - out[k + "0"])
    for k, v in devs.items():
        out["dev_" + k] = np.array(v)
    # size: the float64 copies of the two wide tables are kept as their deviations only, the float64 scores for the first 16 tuples,
    # and of the two steps the second one's parameters
    for k in PARAMS:
        out.pop(k + "1", None)
        if k in ("U", "I"):
            out.pop("G" + k + "64", None)
            out.pop(k + "2_64", None)
    out["pred64"] = out["pred64"][:16]
    TOL_LINES.append("%-34s " % name + "  ".join("%s %.2e" % kv for kv in devs.items()))

    groups = [{"names": sorted(n for n, p in m.named_parameters() if any(p is q for q in g["params"])), "lr": g["lr"],
               "weight_decay": g["weight_decay"]} for g in m.optimizer.param_groups]
    out["groups"] = np.array(json.dumps(groups))
    out["state_keys"] = np.array(list(m.state_dict().keys()))
    out["extra_log_args"] = np.array(Chorus.extra_log_args)
    out["model_flags"] = _flags(Chorus.parse_model_args)
    out["reader_flags"] = _flags(KGReader.parse_data_args)
    return out


def _save(out_dir, name, out):
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    cap = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("slrc_") and f.endswith(".npz"))
    assert size <= cap, (name, size, cap)      # no larger than the SLRC+ fixtures
    print("wrote", path, size >> 10, "KiB")


def make_case(out_dir, name, *spec):
    seed = spec[11]
    for s in range(seed, seed + 200):
        out = try_case(name, *spec[:11], s, *spec[12:])
        if out is not None:
            break
    else:
        raise SystemExit(name + ": no seed satisfies the case's conditions")
    print(name, "seed", s)
    _save(out_dir, name, out)


def make_stage1(out_dir, n_items=60, R=3, d=32, B=48, opt="Adam", lr=5e-4, l2=1e-5, margin=1.0, seed=91):
    torch, pd, BaseRunner, KGReader, Chorus = _reference()
    for s in range(seed, seed + 200):
        rng = np.random.default_rng(s)
        corpus = SimpleNamespace(n_users=10, n_items=n_items, item_relations=["r_complement", "r_substitute"][:R - 1],
                                 item_meta_df=pd.DataFrame({"item_id": np.arange(1, n_items)}), dataset="golden")
        args = _args(torch, d, 1, "BPR", lr, 0.1, margin)
        p = 1.0 / np.arange(1, n_items)
        h, t, hn, tn = (rng.choice(np.arange(1, n_items), size=B, p=p / p.sum()).astype(np.int64) for _ in range(4))
        r = rng.integers(1, R, B).astype(np.int64)
        tn[0], hn[1], h[2] = t[0], h[1], t[2]      # exact ties of either pair, and a head that is its own tail
        head_id, tail_id = np.stack([t, t, tn, t], axis=1), np.stack([h, h, h, hn], axis=1)   # the reference's reversed feed
        rel = np.repeat(r[:, None], 4, axis=1)
        ties = np.stack([tn == t, hn == h], axis=1)
        I0 = (0.3 * rng.standard_normal((n_items, d))).astype(np.float32)
        R0 = (0.3 * rng.standard_normal((R, d))).astype(np.float32)

        def build(double=False):
            torch.manual_seed(s)
            m = Chorus(args, corpus)
            with torch.no_grad():
                m.state_dict()["i_embeddings.weight"].copy_(torch.from_numpy(I0))
                m.state_dict()["r_embeddings.weight"].copy_(torch.from_numpy(R0))
            return m.double() if double else m

        feed = {"head_id": torch.from_numpy(head_id), "tail_id": torch.from_numpy(tail_id), "relation_id": torch.from_numpy(rel),
                "batch_size": B, "phase": "train"}
        m64 = build(True)
        p64 = m64(feed)["prediction"].detach().numpy()
        x64 = margin - p64[:, :2] + p64[:, 2:]
        near = np.abs(x64) < 1e-4 * (np.abs(p64[:, :2]) + np.abs(p64[:, 2:]) + margin)      # a hinge that fp32 could flip
        if (near & ~ties).any() or not ((x64 >= 0).any() and (x64 < 0).any()):
            continue
        m = build()
        o = m(feed)
        loss = m.loss(o)
        loss.backward()
        named = dict(m.named_parameters())
        out = {"meta": np.array([n_items, R, d, B, s], dtype=np.int64), "hyper": np.array([lr, l2, margin]), "opt": np.array(opt),
               "head_id": head_id, "tail_id": tail_id, "relation_id": rel, "ties": ties, "x64": x64, "I0": I0, "Rel0": R0,
               "pred": o["prediction"].detach().numpy().copy(), "loss": np.array(loss.item(), dtype=np.float32),
               "GI": named["i_embeddings.weight"].grad.numpy().copy(), "GRel": named["r_embeddings.weight"].grad.numpy().copy()}
        assert all(named[STATE_KEYS[k]].grad is None for k in PARAMS if k not in ("I", "Rel"))
        m = build()
        m.optimizer = BaseRunner(make_golden._runner_args(BaseRunner, opt, lr, l2))._build_optimizer(m)
        m.train()
        for tag in ("1", "2"):
            m.optimizer.zero_grad()
            m.loss(m(feed)).backward()
            m.optimizer.step()
            out["I" + tag] = m.state_dict()["i_embeddings.weight"].numpy().copy()
            out["Rel" + tag] = m.state_dict()["r_embeddings.weight"].numpy().copy()
        _save(out_dir, "chorus_kg_stage1", out)
        return
    raise SystemExit("stage 1: no seed without a near-tie hinge")


def make_dataset_golden(out_dir):
    torch, pd, BaseRunner, KGReader, Chorus = _reference()
    root = tempfile.mkdtemp(prefix="chorus_golden_")
    slrc_data.make_kg_dataset(root, "synth_kg", seed=KG_SEED)
    p = KGReader.parse_data_args(argparse.ArgumentParser())
    a, _ = p.parse_known_args(["--path", root + "/", "--dataset", "synth_kg", "--include_attr", "0"])
    corpus = KGReader(a)
    margs = _args(torch, 16, 3, "BPR", 1e-3, 0.1, time_scalar=KG_TIME_SCALAR, history_max=4)
    margs.buffer = 0
    model = Chorus(margs, corpus)
    out = {"time_scalar": np.array(KG_TIME_SCALAR), "history_max": np.array(4), "sample_seed": np.array(SAMPLE_SEED),
           "category_num": np.array(model.category_num), "relation_num": np.array(model.relation_num)}
    kg = Chorus.Dataset(model, corpus, "train")      # stage 1: the triplet rows
    np.random.seed(SAMPLE_SEED)
    for epoch in (1, 2):
        kg.actions_before_epoch()
        out["neg_heads%d" % epoch], out["neg_tails%d" % epoch] = kg.neg_heads.astype(np.int64), kg.neg_tails.astype(np.int64)
    feeds = [kg._get_feed_dict(k) for k in range(len(kg))]
    for key in ("head_id", "tail_id", "relation_id"):
        out["kg_" + key] = np.stack([f[key] for f in feeds]).astype(np.int64)
    model.stage = 2
    train = Chorus.Dataset(model, corpus, "train")
    rng = np.random.default_rng(KG_SEED)
    negs = rng.integers(1, corpus.n_items, size=(len(train), 3))
    train.data["neg_items"] = negs
    feeds = [train._get_feed_dict(k) for k in range(len(train))]
    out["train_neg_items"] = negs.astype(np.int64)
    out["train_item_id"] = np.stack([f["item_id"] for f in feeds]).astype(np.int64)
    out["train_category_id"] = np.stack([f["category_id"] for f in feeds]).astype(np.int64)
    out["train_intervals"] = np.stack([f["relational_interval"] for f in feeds])
    dev = Chorus.Dataset(model, corpus, "dev")
    feeds = [dev._get_feed_dict(k) for k in range(KG_DEV_ROWS)]
    out["dev_item_id"] = np.stack([f["item_id"] for f in feeds]).astype(np.int64)
    out["dev_category_id"] = np.stack([f["category_id"] for f in feeds]).astype(np.int64)
    out["dev_intervals"] = np.stack([f["relational_interval"] for f in feeds])
    both = out["train_intervals"]
    assert (both[:, :, 0] < 0).all() and (both[:, :, 1] >= 0).any() and (both[:, :, 2] >= 0).any()
    _save(out_dir, "chorus_kg_dataset", out)


MIXED = ["r_complement", "r_substitute", "r_also_bought", "r_substitute_b", "r_complement_b", "r_substitute_of_complement", "r_view"]
CASES = [
    # name,                             n_users, n_items, n_cat,  d, relations,                         B,  K, opt,      lr,   l2,  lr_scale, seed, redraw, base
    ("chorus_d16_r1_sgd_b1_k1",              20,      30,    1,  16, [],                                1,  1, "SGD",     0.1,  1e-5, 0.1, 171, True,  "BPR"),
    ("chorus_d32_r3_sgd_b160_k4",            64,     200,   12,  32, ["r_complement", "r_substitute"], 160,  4, "SGD",     0.5,  0.0,  0.1, 172, True,  "BPR"),
    ("chorus_d64_r3_adam_b77_k99",           40,     100,    7,  64, ["r_complement", "r_substitute"],  77, 99, "Adam",    1e-3, 0.0,  0.1, 173, False, "BPR"),   # the demo flags
    ("chorus_d128_r8_adagrad_b33_k9",        30,      60,    5, 128, MIXED,                             33,  9, "Adagrad", 0.01, 1e-4, 0.1, 174, True,  "BPR"),
    ("chorus_d32_r3_sgd_b160_k4_gmf",        64,     200,   12,  32, ["r_complement", "r_substitute"], 160,  4, "SGD",     0.5,  0.0,  0.1, 172, True,  "GMF"),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--tolerances", default=None)
    a = ap.parse_args()
    for c in CASES:
        make_case(a.out, *c)
    make_stage1(a.out)
    make_dataset_golden(a.out)
    print("\n".join(TOL_LINES))
    if a.tolerances:
        with open(a.tolerances, "w") as f:
            f.write("\n".join(TOL_LINES) + "\n")
