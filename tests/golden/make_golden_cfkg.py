"""Golden vectors for CFKG FROM THE REFERENCE ITSELF (models/general/CFKG.py, helpers/KGReader.py, the optimizer construction of
helpers/BaseRunner.py), on CPU with one thread.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cfkg.py [--out DIR] [--tolerances FILE]

The reference's runner cannot train CFKG (BaseRunner.fit reads batch['item_id'], which CFKG's feed does not have), so forward, loss,
Dataset and the optimizer BaseRunner builds are driven directly; runner.fit is never called.

Each cfkg_d*.npz holds
  meta [n_users, n_items, n_entities, n_rel, d, B, seed, redraw], hyper [lr, l2, margin], opt (name)
  E0, R0                   what every computation below starts from: what CFKG.__init__ leaves after torch.manual_seed(seed)
                           (redraw = 0: normal(0, 0.01), the demo init), or (redraw = 1) re-drawn wider, so that both hinge states occur
  head, tail, rel          one [B, 4] training feed in CFKG.Dataset's layout, row indices of E (n_users already added)
  pred, loss, GE, GR       CFKG.forward's prediction [B, 4], CFKG.loss and the two dense gradients
  E1, R1                   the tables after one step of the torch.optim optimizer BaseRunner builds (dense semantics)
  x64                      float64 rerun: margin - pos + neg of the 2 B pairs, [B, 2]
  ties                     [B, 2] bool: pairs that are exact ties in every precision (t' = t, or h' = h): row 0's first pair by hand, and
                           whatever the Zipf draw repeats by itself
  state_keys, model_flags, reader_flags
Ids are Zipf-distributed over small tables, so rows repeat.  Set by hand: row 0 has t' = t (with margin 0 an exact tie, which must
come back ACTIVE: clamp_min(0)'s backward passes at 0); row 1's head row equals its tail row; row 2's h' is row 3's t; the batch
lacks the last relation (n_rel > 1).  The generator asserts that active and inactive pairs both occur (B > 1) and that, in the
float64 rerun, no pair outside the exact ties has |x| < 1e-4 (|pos| + |neg| + margin): a pair that close could flip between
fp32 and float64.  The seed is advanced until that holds, so the tests exclude nothing.

cfkg_kg_dataset.npz: the reference Dataset on tests/slrc_data.py's corpus for --include_attr 0 and 1: len(train), neg_heads /
neg_tails after np.random.seed(s); actions_before_epoch(), and the feed dicts of fixed indices in the three phases.
"""
import argparse
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

KG_SEED, SAMPLE_SEED, KG_ROWS = 5, 11, 6
STATE_KEYS = {"E": "e_embeddings.weight", "R": "r_embeddings.weight"}
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


def try_case(name, n_users, n_items, n_entities, n_rel, d, B, opt, lr, l2, margin, seed, redraw):
    torch, _, BaseRunner = make_golden._import_reference()
    from helpers.KGReader import KGReader
    from models.general.CFKG import CFKG
    torch.set_num_threads(1)   # one summation order for every rerun
    rng = np.random.default_rng(seed)
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=d,
                           margin=margin)
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, n_relations=n_rel, n_entities=n_entities)

    def zipf(n, size):
        p = 1.0 / np.arange(1, n)
        return rng.choice(np.arange(1, n), size=size, p=p / p.sum()).astype(np.int64)

    live_rel = max(1, n_rel - 1)                       # the batch lacks the last relation
    r = rng.integers(0, live_rel, size=B).astype(np.int64)
    h = np.where(r == 0, zipf(n_users, B), n_users + zipf(n_entities, B))
    hn = np.where(r == 0, zipf(n_users, B), n_users + zipf(n_entities, B))
    t = n_users + np.where(r == 0, zipf(n_items, B), zipf(n_entities, B))
    tn = n_users + np.where(r == 0, zipf(n_items, B), zipf(n_entities, B))
    tn[0] = t[0]                                       # an exact tie of the first pair at margin 0
    if B > 3:
        r[1] = live_rel - 1
        h[1] = t[1]                                    # the head row IS the tail row (an entity related to itself)
        hn[2] = t[3]                                   # a corrupted head that is another row's tail
    head, tail = np.stack([h, h, h, hn], axis=1), np.stack([t, t, tn, t], axis=1)
    rel = np.repeat(r[:, None], 4, axis=1)
    ties = np.stack([tn == t, hn == h], axis=1)        # the hand-set tie and every tie the Zipf draw repeats by itself

    drawn = {}
    if redraw:
        drawn = {"E": (0.3 * rng.standard_normal((n_users + n_entities, d))).astype(np.float32),
                 "R": (0.3 * rng.standard_normal((n_rel, d))).astype(np.float32)}

    def build(double=False):
        torch.manual_seed(seed)
        model = CFKG(args, corpus)
        with torch.no_grad():
            for k, v in drawn.items():
                model.state_dict()[STATE_KEYS[k]].copy_(torch.from_numpy(v))
        return model.double() if double else model

    feed = {"head_id": torch.from_numpy(head), "tail_id": torch.from_numpy(tail), "relation_id": torch.from_numpy(rel),
            "batch_size": B, "phase": "train"}
    out = {"meta": np.array([n_users, n_items, n_entities, n_rel, d, B, seed, int(redraw)], dtype=np.int64),
           "hyper": np.array([lr, l2, margin], dtype=np.float64), "opt": np.array(opt), "ties": ties,
           "head": head, "tail": tail, "rel": rel}

    # float64 rerun first: the flip hazard decides whether this seed is kept
    m64 = build(double=True)
    o64 = m64(feed)
    p64 = o64["prediction"].detach().numpy()
    x64 = margin - p64[:, :2] + p64[:, 2:]
    guard = 1e-4 * (np.abs(p64[:, :2]) + np.abs(p64[:, 2:]) + margin)
    near = np.abs(x64) < guard
    if (near & ~ties).any():
        return None
    assert ties[0, 0] and np.array_equal(p64[:, :2][ties], p64[:, 2:][ties])
    active = x64 >= 0
    if B > 1 and not (active.any() and (~active).any()):
        return None
    loss64 = m64.loss(o64)
    loss64.backward()
    g64 = {k: dict(m64.named_parameters())[STATE_KEYS[k]].grad.numpy().copy() for k in STATE_KEYS}
    out["x64"] = x64

    model = build()
    out["E0"], out["R0"] = (model.state_dict()[STATE_KEYS[k]].numpy().copy() for k in ("E", "R"))
    model.zero_grad()
    o = model(feed)
    loss = model.loss(o)
    loss.backward()
    out["pred"] = o["prediction"].detach().numpy().copy()
    out["loss"] = np.array(loss.item(), dtype=np.float32)
    assert out["pred"].shape == (B, 4) and np.array_equal(out["pred"][:, 0], out["pred"][:, 1])
    named = dict(model.named_parameters())
    for k in STATE_KEYS:
        out["G" + k] = named[STATE_KEYS[k]].grad.numpy().copy()
        assert np.isfinite(out["G" + k]).all(), (name, k)
    if margin == 0:   # the tie came back active: the pair's gradient is -+1 / 2B, so row 0's t and t' rows see a - and a + term
        x32 = margin - out["pred"][0, 0] + out["pred"][0, 2]
        assert x32 == 0.0
    # the reference's own fp32 error against its float64 run: what the GPU tests' tolerances are a stated factor above
    TOL_LINES.append("%-32s pred %.3e  loss %.3e  GE %.3e  GR %.3e" % (
        name, _needed(out["pred"], p64), abs(float(out["loss"]) - loss64.item()) / max(abs(loss64.item()), 1e-30),
        _needed(out["GE"], g64["E"]), _needed(out["GR"], g64["R"])))

    m = build()
    runner = BaseRunner(make_golden._runner_args(BaseRunner, opt, lr, l2))
    m.optimizer = runner._build_optimizer(m)
    m.train()
    m.optimizer.zero_grad()
    m.loss(m(feed)).backward()
    m.optimizer.step()
    out["E1"], out["R1"] = (m.state_dict()[STATE_KEYS[k]].numpy().copy() for k in ("E", "R"))
    assert np.isfinite(out["E1"]).all() and np.isfinite(out["R1"]).all()
    out["state_keys"] = np.array(sorted(m.state_dict().keys()))
    out["model_flags"] = _flags(CFKG.parse_model_args)
    out["reader_flags"] = _flags(KGReader.parse_data_args)
    return out


def make_case(out_dir, name, n_users, n_items, n_entities, n_rel, d, B, opt, lr, l2, margin, seed, redraw):
    for s in range(seed, seed + 200):
        out = try_case(name, n_users, n_items, n_entities, n_rel, d, B, opt, lr, l2, margin, s, redraw)
        if out is not None:
            break
    else:
        raise SystemExit(name + ": no seed without a near-tie pair")
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 << 10, (name, size)
    print("wrote", path, size >> 10, "KiB", "seed", s)


def make_dataset_golden(out_dir):
    torch, _, _ = make_golden._import_reference()
    from helpers.KGReader import KGReader
    from models.general.CFKG import CFKG
    root = tempfile.mkdtemp(prefix="cfkg_golden_")
    slrc_data.make_kg_dataset(root, "synth_kg", seed=KG_SEED)
    out = {"sample_seed": np.array(SAMPLE_SEED)}
    for include_attr in (0, 1):
        p = KGReader.parse_data_args(argparse.ArgumentParser())
        a, _ = p.parse_known_args(["--path", root + "/", "--dataset", "synth_kg", "--include_attr", str(include_attr)])
        corpus = KGReader(a)
        margs = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=0, num_neg=1, dropout=0, test_all=0, emb_size=16, margin=0)
        model = CFKG(margs, corpus)
        tag = "a%d_" % include_attr
        train = CFKG.Dataset(model, corpus, "train")
        np.random.seed(SAMPLE_SEED)
        train.actions_before_epoch()
        out[tag + "len_train"] = np.array(len(train))
        out[tag + "neg_heads"], out[tag + "neg_tails"] = train.neg_heads.astype(np.int64), train.neg_tails.astype(np.int64)
        idx = np.unique(np.linspace(0, len(train) - 1, 2 * KG_ROWS).astype(np.int64))   # graph triplets and interactions
        out[tag + "train_idx"] = idx
        feeds = [train._get_feed_dict(int(k)) for k in idx]
        assert sorted(feeds[0]) == ["head_id", "relation_id", "tail_id"]
        for key in ("head_id", "tail_id", "relation_id"):
            out[tag + "train_" + key] = np.stack([f[key] for f in feeds]).astype(np.int64)
        rels = np.asarray(train.data["relation"])
        assert (rels[idx] == 0).any() and (rels[idx] > 0).any()
        for phase in ("dev", "test"):
            ds = CFKG.Dataset(model, corpus, phase)
            feeds = [ds._get_feed_dict(k) for k in range(KG_ROWS)]
            assert sorted(feeds[0]) == ["head_id", "relation_id", "tail_id"]
            for key in ("head_id", "tail_id", "relation_id"):
                out[tag + phase + "_" + key] = np.stack([f[key] for f in feeds]).astype(np.int64)
        model.test_all = 1
        f = CFKG.Dataset(model, corpus, "test")._get_feed_dict(0)
        for key in ("head_id", "tail_id", "relation_id"):
            out[tag + "test_all_" + key] = np.asarray(f[key]).astype(np.int64)
    path = os.path.join(out_dir, "cfkg_kg_dataset.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB")


CASES = [
    # name,                          n_users, n_items, n_entities, n_rel,  d,   B, opt,       lr,   l2,  margin, seed, redraw
    ("cfkg_d16_sgd_b1_r1_m0",             20,      30,        30,     1,  16,   1, "SGD",     0.1,  1e-5, 0.0,   81, True),
    ("cfkg_d32_sgd_b160_r4_m1",           64,     200,       240,     4,  32, 160, "SGD",     0.5,  0.0,  1.0,   82, True),
    ("cfkg_d64_adam_b77_r4_m0",           40,     100,       130,     4,  64,  77, "Adam",    1e-4, 1e-6, 0.0,   83, False),   # the demo init: pins the init stream
    ("cfkg_d128_adagrad_b33_r8_m05",      30,      60,        90,     8, 128,  33, "Adagrad", 0.01, 1e-4, 0.5,   84, True),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--tolerances", default=None)
    a = ap.parse_args()
    for c in CASES:
        make_case(a.out, *c)
    make_dataset_golden(a.out)
    print("\n".join(TOL_LINES))
    if a.tolerances:
        with open(a.tolerances, "w") as f:
            f.write("\n".join(TOL_LINES) + "\n")
