"""Golden vectors for SLRC+ and KGReader FROM THE REFERENCE ITSELF (models/sequential/SLRCPlus.py, helpers/KGReader.py, the optimizer
construction of helpers/BaseRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_slrc.py [--out DIR]

Each slrc_*.npz holds
  meta [n_users, n_items, d, R, B, K, seed, redraw], hyper [lr, l2], opt (name)
  <P>0 for the ten parameters P of tests/slrc_np.py's PARAMS: what every computation below starts from -- what SLRCPlus.__init__
                           leaves after torch.manual_seed(seed) (redraw = 0: normal(0, 0.01), the demo line), or (redraw = 1) re-drawn
                           wider: with the native init every score is ~1e-3 and a wrong product hides in the loss
  uid, iid, intervals      one training batch: users [B], candidates [B, 1 + K] (column 0 the target), relational_interval [B, 1 + K, R]
  pred, loss               SLRCPlus.forward's prediction [B, 1 + K] and GeneralModel.loss
  G<P>                     the ten dense gradients of that loss
  <P>1                     the parameters after one step of the torch.optim optimizer BaseRunner builds (dense semantics: weight decay
                           reaches every row; the two bias tables take none)
  special                  rows (item, relation, kind) of the hand-set clamp entries: kind 0 / 1 / 2 = betas + 1 below 1e-10 / exactly
                           10 / above 10, kind 3 / 4 / 5 the same for sigmas + 1
  state_keys, model_flags, reader_flags     the state_dict keys and the option strings SLRCPlus.parse_model_args / KGReader.parse_data_args add
Ids are Zipf-distributed over small tables, so users and candidates repeat inside the batch; set by hand: a negative equal to the
positive, a candidate repeated inside a tuple, a tuple whose intervals are all -1, an interval of exactly 0, the clamp entries above.
The generator asserts that every gradient is finite and records, for the Adam / Adagrad cases, the share of a table's touched
elements with a loss gradient 0 < |g| < 1e-7 (tiny_share, PARAMS order: the elements an Adam / Adagrad comparison could name as
ill-conditioned; the demo-line case exceeds 0.5 % on I, so the tests name none).  user_bias is the exception, and not by
choice: its gradient sum_c d loss / d pred[b, c] is exactly 0 in exact arithmetic, so what the reference records for it is round-off
(asserted here to stay below 1e-5 of the item_bias gradient's largest entry).

kg_reader.json: the reference KGReader's attributes on tests/slrc_data.py's corpus for --include_attr 0 and 1.
slrc_kg_dataset.npz: the reference Dataset's relational_interval for every train row (fixed negatives) and the first dev rows.
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
import make_golden  # noqa: E402
import slrc_data  # noqa: E402
from slrc_np import PARAMS, STATE_KEYS  # noqa: E402

KG_SEED, KG_TIME_SCALAR, KG_DEV_ROWS = 5, 100000, 8


def _flags(add):
    p = argparse.ArgumentParser()
    before = {s for a in p._actions for s in a.option_strings}
    p = add(p)
    return np.array(sorted({s for a in p._actions for s in a.option_strings} - before))


def make_case(out_dir, name, n_users, n_items, d, R, B, K, opt, lr, l2, seed, redraw):
    torch, _, BaseRunner = make_golden._import_reference()
    from helpers.KGReader import KGReader
    from models.sequential.SLRCPlus import SLRCPlus
    torch.set_num_threads(1)   # one summation order for every rerun
    rng = np.random.default_rng(seed)
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=K, dropout=0, test_all=0, emb_size=d,
                           history_max=20, time_scalar=8640000)
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, item_relations=["r_%d" % k for k in range(R - 1)])

    def zipf(n, size):
        p = 1.0 / np.arange(1, n)
        return rng.choice(np.arange(1, n), size=size, p=p / p.sum()).astype(np.int64)

    uid, iid = zipf(n_users, B), zipf(n_items, (B, 1 + K))
    if K >= 2:
        iid[0, 1] = iid[0, 0]          # a negative equals the positive
        iid[0, 2] = iid[0, 1]          # ... and a candidate repeats inside the tuple
    iv = np.where(rng.random((B, 1 + K, R)) < 0.4, -1.0, rng.uniform(0.0, 3.0, (B, 1 + K, R))).astype(np.float32)
    dead = B - 1 if B > 1 else None    # a tuple whose intervals are all -1 (B = 1: one candidate's)
    if dead is None:
        iv[0, 1, :] = -1.0
    else:
        iv[dead] = -1.0
    iv[0, 0, 0] = 0.0                  # an interval of exactly 0

    drawn = {}
    if redraw:
        sd = {"U": 0.3, "I": 0.3, "user_bias": 0.3, "item_bias": 0.3, "alphas": 0.5, "pis": 0.2, "betas": 0.4, "sigmas": 0.4, "mus": 0.5}
        shape = {"U": (n_users, d), "I": (n_items, d), "user_bias": (n_users, 1), "item_bias": (n_items, 1)}
        for k in PARAMS:
            drawn[k] = (np.array(0.3) if k == "global_alpha" else sd[k] * rng.standard_normal(shape.get(k, (n_items, R)))).astype(np.float32)
    # the clamp entries, on (item, relation) slots of items that occur in the batch outside the dead tuple
    live = iid if dead is None else iid[:dead]
    slots = [(int(i), r) for i in np.unique(live) for r in range(R)]
    values = [("betas", -1.5), ("betas", 9.0), ("betas", 11.0), ("sigmas", -1.5), ("sigmas", 9.0), ("sigmas", 11.0)]
    special = []
    for kind, (slot, (table, val)) in enumerate(zip(slots[:: max(1, len(slots) // 6)], values)):
        special.append((slot[0], slot[1], kind))
        b, c = np.argwhere(live == slot[0])[0]
        if (b, c) != (0, 1) or dead is not None:
            iv[b, c, slot[1]] = 0.7 if (b, c, slot[1]) != (0, 0, 0) else 0.0   # the entry takes part in a score
    assert dead is None or len(special) == 6, name

    def build():
        torch.manual_seed(seed)
        model = SLRCPlus(args, corpus)
        with torch.no_grad():
            sd_ = model.state_dict()
            for k, v in drawn.items():
                sd_[STATE_KEYS[k]].copy_(torch.from_numpy(v))
            for (item, r, kind) in special:
                table, val = values[kind]
                sd_[STATE_KEYS[table]][item, r] = val
        return model

    def snapshot(model, tag, out):
        sd_ = model.state_dict()
        for k in PARAMS:
            out[k + tag] = sd_[STATE_KEYS[k]].detach().numpy().copy()

    out = {"meta": np.array([n_users, n_items, d, R, B, K, seed, int(redraw)], dtype=np.int64),
           "hyper": np.array([lr, l2], dtype=np.float64), "opt": np.array(opt), "special": np.array(special, dtype=np.int64).reshape(-1, 3)}
    model = build()
    snapshot(model, "0", out)
    out.update(uid=uid, iid=iid, intervals=iv)
    feed = {"user_id": torch.from_numpy(uid), "item_id": torch.from_numpy(iid), "relational_interval": torch.from_numpy(iv),
            "batch_size": B, "phase": "train"}

    model.zero_grad()
    o = model(feed)
    loss = model.loss(o)
    loss.backward()
    out["pred"] = o["prediction"].detach().numpy().copy()
    out["loss"] = np.array(loss.item(), dtype=np.float32)
    named = dict(model.named_parameters())
    tiny = {}
    touched = {k: (np.unique(uid) if k in ("U", "user_bias") else np.unique(iid)) for k in PARAMS if k != "global_alpha"}
    for k in PARAMS:
        g = named[STATE_KEYS[k]].grad.numpy().copy()
        assert np.isfinite(g).all(), (name, k)
        out["G" + k] = g
        if k == "user_bias":
            # sum_c d loss / d pred[b, c] = 0 in exact arithmetic (the loss does not change when a tuple's scores shift together),
            # so this gradient is the reference's own round-off: held to a floor, not to the cap below
            assert np.abs(g).max() <= 1e-5 * np.abs(named[STATE_KEYS["item_bias"]].grad.numpy()).max(), (name, k)
        elif k != "global_alpha" and opt != "SGD":   # (SGD's step is linear in g: nothing is ill-conditioned there)
            a = np.abs(g[touched[k]])
            tiny[k] = float(((a > 0) & (a < 1e-7)).mean())
    assert np.isfinite(out["pred"]).all() and np.isfinite(out["loss"])
    # recorded, not capped: with the demo line's native init 1.1 % of the touched elements of I have 0 < |g| < 1e-7 under the reference
    # alone, above the 0.5 % an exclusion by name would be allowed -- so the tests exclude nothing (tiny_share is what they would have named)
    out["tiny_share"] = np.array([tiny.get(k, 0.0) for k in PARAMS])
    print(name, "share of touched elements with 0 < |g| < 1e-7:", {k: round(v, 4) for k, v in tiny.items()})

    m = build()
    runner = BaseRunner(make_golden._runner_args(BaseRunner, opt, lr, l2))
    m.optimizer = runner._build_optimizer(m)
    m.train()
    m.optimizer.zero_grad()
    m.loss(m(feed)).backward()
    m.optimizer.step()
    snapshot(m, "1", out)
    for k in PARAMS:
        assert np.isfinite(out[k + "1"]).all(), (name, k)

    out["state_keys"] = np.array(sorted(m.state_dict().keys()))
    out["model_flags"] = _flags(SLRCPlus.parse_model_args)
    out["reader_flags"] = _flags(KGReader.parse_data_args)

    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 << 10, (name, size)
    print("wrote", path, size >> 10, "KiB")


def _plain(x):
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    return x


def make_reader_goldens(out_dir):
    torch, _, _ = make_golden._import_reference()
    from helpers.KGReader import KGReader
    from models.sequential.SLRCPlus import SLRCPlus
    root = tempfile.mkdtemp(prefix="slrc_golden_")
    slrc_data.make_kg_dataset(root, "synth_kg", seed=KG_SEED)
    recorded = {}
    for include_attr in (0, 1):
        p = KGReader.parse_data_args(argparse.ArgumentParser())
        a, _ = p.parse_known_args(["--path", root + "/", "--dataset", "synth_kg", "--include_attr", str(include_attr)])
        corpus = KGReader(a)
        rec = {"item_relations": corpus.item_relations, "attr_relations": corpus.attr_relations, "relations": corpus.relations,
               "n_relations": int(corpus.n_relations), "n_entities": int(corpus.n_entities), "n_users": int(corpus.n_users),
               "n_items": int(corpus.n_items),
               "relation_df": _plain(corpus.relation_df[["head", "relation", "tail"]].values.tolist()),
               "triplet_set": sorted(_plain(list(t)) for t in corpus.triplet_set),
               "item_meta_columns": list(corpus.item_meta_df.columns),
               "item_meta_rows": _plain(corpus.item_meta_df.values.tolist())}
        if include_attr:
            rec["attr_max"] = _plain(list(corpus.attr_max))
            rec["share_attr_dict"] = {str(k): _plain(v) for k, v in sorted(corpus.share_attr_dict.items())}
        recorded["include_attr_%d" % include_attr] = rec
        if include_attr == 0:
            margs = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=0, num_neg=3, dropout=0, test_all=0, emb_size=16,
                                    history_max=4, time_scalar=KG_TIME_SCALAR)
            model = SLRCPlus(margs, corpus)
            out = {"time_scalar": np.array(KG_TIME_SCALAR), "history_max": np.array(4)}
            train = SLRCPlus.Dataset(model, corpus, "train")
            rng = np.random.default_rng(KG_SEED)
            negs = rng.integers(1, corpus.n_items, size=(len(train), 3))
            # some negatives are drawn from the user's own history, so that the self relation shows among the negatives too
            for k in range(0, len(train), 4):
                u, pos = train.data["user_id"][k], train.data["position"][k]
                negs[k, 0] = corpus.user_his[u][pos - 1][0]
            train.data["neg_items"] = negs
            feeds = [train._get_feed_dict(k) for k in range(len(train))]
            out["train_neg_items"] = negs.astype(np.int64)
            out["train_item_id"] = np.stack([f["item_id"] for f in feeds]).astype(np.int64)
            out["train_intervals"] = np.stack([f["relational_interval"] for f in feeds])
            dev = SLRCPlus.Dataset(model, corpus, "dev")
            feeds = [dev._get_feed_dict(k) for k in range(KG_DEV_ROWS)]
            out["dev_item_id"] = np.stack([f["item_id"] for f in feeds]).astype(np.int64)
            out["dev_intervals"] = np.stack([f["relational_interval"] for f in feeds])
            both = out["train_intervals"]
            assert (both[:, :, 0] >= 0).any() and (both[:, :, 1] >= 0).any() and (both[:, :, 2] >= 0).any() and (both < 0).any()
            path = os.path.join(out_dir, "slrc_kg_dataset.npz")
            np.savez_compressed(path, **out)
            print("wrote", path, os.path.getsize(path) >> 10, "KiB")
    path = os.path.join(out_dir, "kg_reader.json")
    with open(path, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
    assert os.path.getsize(path) < 512 << 10
    print("wrote", path, os.path.getsize(path) >> 10, "KiB")


CASES = [
    # name,                          n_users, n_items,  d,  R,   B,  K, opt,       lr,   l2,   seed, redraw
    ("slrc_d16_r1_sgd_b1_k1",             20,      30,  16, 1,   1,  1, "SGD",     0.1,  1e-5, 71, True),
    ("slrc_d32_r3_sgd_b160_k4",           64,     300,  32, 3, 160,  4, "SGD",     0.5,  0.0,  72, True),
    ("slrc_d64_r3_adam_b77_k99",          40,     120,  64, 3,  77, 99, "Adam",    5e-4, 1e-5, 73, False),   # the demo line: pins the init stream
    ("slrc_d128_r8_adagrad_b33_k9",       30,      60, 128, 8,  33,  9, "Adagrad", 0.01, 1e-4, 74, True),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    for c in CASES:
        make_case(a.out, *c)
    make_reader_goldens(a.out)
