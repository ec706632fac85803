"""CPU: CFKG's host side -- the float64 restatement (tests/cfkg_np.py) against the reference's own numbers (tests/golden/cfkg_*.npz,
cfkg_kg_dataset.npz, written by tests/golden/make_golden_cfkg.py), the Dataset's sampling loop and feeds, the model file's class
lookup, flags, state_dict keys and shape check, the runner's handling of a feed without `item_id`, and the C entry points'
declarations and refusals.  No kernel runs.

Tolerances: the goldens are float32 results of the reference, the restatement is float64: conftest.assert_close at its default 1e-5.
Nothing is excluded: the generator kept only seeds at which no hinge is close enough to 0 to flip between the precisions, and the
exact ties (t' = t, h' = h) are exact in every precision -- and ACTIVE (clamp_min(0)'s backward passes at 0)."""
import argparse
import ctypes as C
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT, assert_close, assert_update_close, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cfkg_np  # noqa: E402
from cfkg_np import STATE_KEYS  # noqa: E402
from slrc_data import make_kg_dataset  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

CASES = golden_cases("cfkg_d")
KG_SEED = 5      # tests/golden/make_golden_cfkg.py's


def _args(**kw):
    a = dict(device="cpu", model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=64, margin=0.0)
    a.update(kw)
    return SimpleNamespace(**a)


def _corpus(n_users=5, n_items=6, n_entities=8, n_rel=3):
    return SimpleNamespace(n_users=n_users, n_items=n_items, n_entities=n_entities, n_relations=n_rel)


def test_golden_cases_exist_and_hold_the_hand_set_rows():
    assert tuple(CASES) == tuple(sorted(cfkg_np.GOLDEN_CASES))
    shapes = set()
    for c in CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", c + ".npz")) < 512 << 10
        g = load_golden(c)
        n_users, n_items, n_entities, n_rel, d, B, seed, redraw = (int(x) for x in g["meta"])
        lr, l2, margin = (float(x) for x in g["hyper"])
        shapes.add((str(g["opt"]), d, B, n_rel, margin, lr, l2))
        head, tail, rel = g["head"], g["tail"], g["rel"]
        h, t, hn, tn, r = cfkg_np.quad(head, tail, rel)
        assert head.shape == tail.shape == rel.shape == (B, 4) and g["E0"].shape == (n_users + n_entities, d) and g["R0"].shape == (n_rel, d)
        assert (head[:, :3] == h[:, None]).all() and (tail[:, [0, 1, 3]] == t[:, None]).all() and (rel == r[:, None]).all()
        assert tail.min() >= n_users and head.max() < n_users + n_entities and (h[r == 0] < n_users).all()
        assert tn[0] == t[0] and g["ties"][0, 0] and np.array_equal(g["ties"], np.stack([tn == t, hn == h], axis=1))
        x = g["x64"]
        guard = 1e-4 * (np.abs(g["pred"][:, :2]) + np.abs(g["pred"][:, 2:]) + margin)
        assert not ((np.abs(x) < guard) & ~g["ties"]).any()                  # no pair can flip between fp32 and float64
        if B > 3:
            assert len(np.unique(head)) < head.size and len(np.unique(tail)) < tail.size      # rows repeat
            assert h[1] == t[1] and hn[2] == t[3]
            assert set(r.tolist()) == set(range(n_rel - 1))                   # the batch lacks the last relation
            assert (x >= 0).any() and (x < 0).any()                           # both hinge states
            assert np.abs(g["GR"][n_rel - 1]).max() == 0.0
    assert shapes == {("SGD", 16, 1, 1, 0.0, 0.1, 1e-5), ("SGD", 32, 160, 4, 1.0, 0.5, 0.0), ("Adam", 64, 77, 4, 0.0, 1e-4, 1e-6),
                      ("Adagrad", 128, 33, 8, 0.5, 0.01, 1e-4)}


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference(case):
    g = load_golden(case)
    E0, R0, head, tail, rel = g["E0"], g["R0"], g["head"], g["tail"], g["rel"]
    lr, l2, margin = (float(x) for x in g["hyper"])
    B = head.shape[0]
    pred = cfkg_np.scores(E0, R0, head, tail, rel)
    assert_close(g["pred"], pred, what=case + " pred")
    loss, loss_vec, x, gpred = cfkg_np.hinge(pred, margin)
    assert_close(float(g["loss"]), loss, what=case + " loss")
    assert np.array_equal(x >= 0, g["x64"] >= 0)
    GE, GR = cfkg_np.dense_grads(E0, R0, head, tail, rel, gpred)
    assert_close(g["GE"], GE, what=case + " GE")
    assert_close(g["GR"], GR, what=case + " GR")
    # the fused front's formulas are the same numbers
    fpred, floss_vec, grows, FGR = cfkg_np.front(E0, R0, head, tail, rel, margin)
    assert np.abs(fpred - pred).max() <= 1e-12 and np.abs(floss_vec - loss_vec).max() <= 1e-12 and np.abs(FGR - GR).max() <= 1e-12
    h, t, hn, tn, _ = cfkg_np.quad(head, tail, rel)
    acc = np.zeros_like(GE)
    np.add.at(acc, np.stack([h, t, hn, tn], axis=1).reshape(-1), grows.reshape(4 * B, -1))
    assert np.abs(acc - GE).max() <= 1e-12
    if margin == 0:      # the exact tie is ACTIVE: its two gradient rows are w b and w (a - b) = 0, not both 0
        assert x[0, 0] == 0.0 and gpred[0, 0] == -0.5 / B and gpred[0, 2] == 0.5 / B
        assert np.abs(grows[0, 3]).max() > 0
    # torch.optim's step is dense: weight decay reaches every row
    opt = str(g["opt"])
    for k in ("E", "R"):
        W0 = g[k + "0"]
        W1, _, _ = cfkg_np.optimizer_rows(W0, g["G" + k], np.arange(W0.shape[0]), opt, lr, l2)
        assert_update_close(g[k + "1"], W0, W1, what=f"{case} {k} update", rtol=2e-5, extra_atol=0.0 if opt == "SGD" else 1e-3 * lr,
                            strict=True)


def test_restated_gradients_agree_with_autograd_in_float64():
    import torch
    rng = np.random.default_rng(3)
    n_rows, n_rel, d, B = 11, 3, 6, 9
    E, R = rng.normal(0, 0.5, (n_rows, d)), rng.normal(0, 0.5, (n_rel, d))
    h, t, hn, tn = (rng.integers(0, n_rows, B) for _ in range(4))
    r = rng.integers(0, n_rel, B)
    tn[0], h[1] = t[0], t[1]
    head, tail, rel = np.stack([h, h, h, hn], 1), np.stack([t, t, tn, t], 1), np.repeat(r[:, None], 4, 1)
    for margin in (0.0, 0.7):
        tE, tR = torch.tensor(E, requires_grad=True), torch.tensor(R, requires_grad=True)
        pred = -((tE[head] + tR[rel] - tE[tail]) ** 2).sum(-1)
        loss = torch.nn.MarginRankingLoss(margin=margin)(pred[:, :2].flatten(), pred[:, 2:].flatten(), torch.ones(2 * B, dtype=torch.float64))
        loss.backward()
        fpred, loss_vec, grows, GR = cfkg_np.front(E, R, head, tail, rel, margin)
        assert np.abs(fpred - pred.detach().numpy()).max() <= 1e-12 and abs(loss_vec.mean() - loss.item()) <= 1e-12
        GE = np.zeros_like(E)
        np.add.at(GE, np.stack([h, t, hn, tn], 1).reshape(-1), grows.reshape(4 * B, d))
        assert np.abs(GE - tE.grad.numpy()).max() <= 1e-12 and np.abs(GR - tR.grad.numpy()).max() <= 1e-12
        if margin == 0:      # at the tie the pair's gradient is -+1 / 2B, not 0
            assert np.abs(grows[0, 3]).max() > 0


# ---- the Dataset against the recorded reference ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kg_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("cfkg_kg"))
    make_kg_dataset(root, "synth_kg", seed=KG_SEED)
    return root


def _reader(kg_root, include_attr):
    from helpers.KGReader import KGReader
    a, _ = KGReader.parse_data_args(argparse.ArgumentParser()).parse_known_args(
        ["--path", kg_root + "/", "--dataset", "synth_kg", "--include_attr", str(include_attr)])
    return KGReader(a)


@pytest.mark.parametrize("include_attr", [0, 1])
def test_dataset_equals_the_recorded_reference(include_attr, kg_root):
    from models.general.CFKG import CFKG
    g = load_golden("cfkg_kg_dataset")
    tag = "a%d_" % include_attr
    corpus = _reader(kg_root, include_attr)
    model = SimpleNamespace(test_all=0, buffer=0)
    train = CFKG.Dataset(model, corpus, "train")
    assert len(train) == int(g[tag + "len_train"]) == len(corpus.relation_df) + len(corpus.data_df["train"])
    assert np.array_equal(np.asarray(train.data["relation"])[:len(corpus.relation_df)], corpus.relation_df["relation"].values)
    np.random.seed(int(g["sample_seed"]))
    train.actions_before_epoch()
    assert np.array_equal(train.neg_heads, g[tag + "neg_heads"]) and np.array_equal(train.neg_tails, g[tag + "neg_tails"])
    feeds = [train[int(k)] for k in g[tag + "train_idx"]]
    assert sorted(feeds[0]) == ["head_id", "relation_id", "tail_id"]             # no user_id in training
    for key in ("head_id", "tail_id", "relation_id"):
        got = np.stack([f[key] for f in feeds])
        assert got.dtype == np.int64 and got.shape == (len(feeds), 4)
        assert np.array_equal(got, g[tag + "train_" + key]), key
    rel = g[tag + "train_relation_id"][:, 0]
    assert (rel == 0).any() and (rel > 0).any()
    if include_attr:
        assert int(np.max(np.asarray(train.data["relation"]))) == corpus.n_relations - 1 == 3
    for phase in ("dev", "test"):
        ds = CFKG.Dataset(model, corpus, phase)
        n = g[tag + phase + "_head_id"].shape[0]
        feeds = [ds[k] for k in range(n)]
        assert sorted(feeds[0]) == ["head_id", "relation_id", "tail_id", "user_id"]   # the one extra key
        for key in ("head_id", "tail_id", "relation_id"):
            assert np.array_equal(np.stack([f[key] for f in feeds]), g[tag + phase + "_" + key]), (phase, key)
        assert [f["user_id"] for f in feeds] == [int(f["head_id"][0]) for f in feeds] == list(ds.data["user_id"][:n])
        batch = ds.collate_batch(feeds[:3])
        assert tuple(batch["head_id"].shape) == tuple(batch["tail_id"].shape) == (3, g[tag + phase + "_head_id"].shape[1])
        assert tuple(batch["user_id"].shape) == (3,)
    model.test_all = 1
    f = CFKG.Dataset(model, corpus, "test")[0]
    for key in ("head_id", "tail_id", "relation_id"):
        assert np.array_equal(f[key], g[tag + "test_all_" + key]), key
    assert f["tail_id"].shape == (corpus.n_items,) and f["tail_id"][1] == corpus.n_users + 1


# ---- the model file ----------------------------------------------------------------------------------------------------------------

def test_class_lookup_flags_and_log_args():
    import main
    cls = main.find_class("model", ("CFKG", ""))
    assert cls.__name__ == "CFKG" and cls.reader == "KGReader" and cls.runner == "BaseRunner"
    assert cls.extra_log_args == ["emb_size", "margin", "include_attr"]
    assert cls.candidate_permutation_equivariant is True
    assert hasattr(cls, "hip_train_step") and hasattr(cls, "hip_rowwise_supported") and not hasattr(cls, "full_catalogue_vectors")
    d, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
    assert (d.emb_size, d.margin, d.num_neg, d.test_all) == (64, 0, 1, 0)
    assert main.find_class("helper", cls.reader).__name__ == "KGReader"


def _added_flags(add):
    p = argparse.ArgumentParser()
    before = {s for a in p._actions for s in a.option_strings}
    p = add(p)
    return sorted({s for a in p._actions for s in a.option_strings} - before)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_and_flags_equal_the_recorded_reference(case):
    import torch
    from helpers.KGReader import KGReader
    from models.general.CFKG import CFKG
    from rechorus_amd import nn as hnn
    g = load_golden(case)
    n_users, n_items, n_entities, n_rel, d, B, seed, redraw = (int(x) for x in g["meta"])
    torch.manual_seed(seed)
    m = CFKG(_args(emb_size=d, margin=float(g["hyper"][2])), _corpus(n_users, n_items, n_entities, n_rel))
    assert sorted(m.state_dict().keys()) == sorted(g["state_keys"].tolist()) == sorted(STATE_KEYS.values())
    assert list(m.state_dict().keys()) == ["e_embeddings.weight", "r_embeddings.weight"]            # the definition order
    assert isinstance(m.e_embeddings, hnn.HipEmbedding) and isinstance(m.r_embeddings, hnn.HipEmbedding)
    for k in ("E", "R"):
        assert tuple(m.state_dict()[STATE_KEYS[k]].shape) == g[k + "0"].shape
    if not redraw:      # the demo init: the same seed leaves the reference's tables, bit for bit (the init stream)
        assert np.array_equal(m.state_dict()["e_embeddings.weight"].numpy(), g["E0"])
        assert np.array_equal(m.state_dict()["r_embeddings.weight"].numpy(), g["R0"])
    m.load_state_dict({STATE_KEYS[k]: torch.from_numpy(g[k + "1"]) for k in ("E", "R")})
    assert np.array_equal(m.state_dict()["r_embeddings.weight"].numpy(), g["R1"])
    assert _added_flags(CFKG.parse_model_args) == g["model_flags"].tolist() and {"--emb_size", "--margin"} <= set(g["model_flags"].tolist())
    assert _added_flags(KGReader.parse_data_args) == g["reader_flags"].tolist() and "--include_attr" in g["reader_flags"].tolist()
    assert m.loss_function.margin == float(g["hyper"][2]) and m.hip_rowwise_supported()


def test_unsupported_shapes_are_refused_at_construction_with_the_flag_named():
    from models.general.CFKG import CFKG
    with pytest.raises(ValueError, match=r"--emb_size 48.*16, 32, 64, 128"):
        CFKG(_args(emb_size=48), _corpus())
    with pytest.raises(ValueError, match=r"9 relations.*n_rel=9 outside 1\.\.8"):
        CFKG(_args(emb_size=16), _corpus(n_rel=9))
    m = CFKG(_args(emb_size=16), _corpus(n_rel=8))
    assert m.hip_rowwise_supported() and m.relation_num == 8 and m.e_embeddings.weight.shape == (5 + 8, 16)
    with pytest.raises(RuntimeError, match="GPU only"):
        import torch
        ids = torch.zeros((2, 4), dtype=torch.int64)
        m({"head_id": ids, "tail_id": ids, "relation_id": ids, "batch_size": 2})


def test_dataset_kind_is_none():
    from models.general.CFKG import CFKG
    from rechorus_amd import pipeline
    assert pipeline.dataset_kind(object.__new__(CFKG.Dataset)) is None      # the DataLoader path: negatives are sampled on the host


def test_the_runner_reads_item_id_only_where_it_shuffles():
    """the one change outside new files: fit() takes batch['item_id'] inside the `if not equivariant:` branch, so a feed without
    that key trains (the reference's runner raises KeyError on CFKG's feed)"""
    src = open(os.path.join(PLUGIN, "helpers", "BaseRunner.py")).read()
    body = src[src.index("    def fit("):src.index("    def _after_step(")]
    branch = body.index("if not equivariant:")
    assert body.count("batch['item_id']") == 2 and all(m.start() > branch for m in re.finditer(re.escape("batch['item_id']"), body))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

WANT = {"rc_cfkg_check_shape", "rc_cfkg_fwd_bwd_rows_per_block", "rc_cfkg_scores", "rc_cfkg_scores_bwd",
        "rc_cfkg_fwd_bwd_workspace_bytes", "rc_cfkg_fwd_bwd"}


def test_lib_signatures_and_header_agree_on_every_cfkg_symbol():
    from rechorus_amd import _lib
    header = open(os.path.join(ROOT, "include", "rechorus_hip.h")).read()
    assert not re.search(r"^int rc_cfkg_", header, re.M)
    protos = dict((m.group(2), (m.group(1), m.group(3))) for m in
                  re.finditer(r"^(enum rc_status|size_t) (rc_cfkg_\w+)\(([^;]*)\);", header, re.M | re.S))
    assert set(protos) == WANT == {k for k in _lib.SIGNATURES if k.startswith("rc_cfkg_")}
    # each prototype cites the reference lines it replaces
    for name in WANT:
        before = header[:header.index(" " + name + "(")]
        assert re.search(r"CFKG\.py:\d+", before[before.rindex("/*", 0, len(before)):]), name
    lib = _lib.load()
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert hasattr(lib, name), name
        assert (restype is C.c_size_t) == (ret == "size_t"), name
        kinds = []
        for p in (q.strip() for q in params.split(",")):
            if "*" in p or p.startswith("rc_stream_t"):
                kinds.append("ptr")
            else:
                kinds.append({"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "size_t": C.c_size_t}[p.rsplit(" ", 1)[0]])
        got = ["ptr" if t is C.c_void_p else t for t in argtypes]
        assert got == kinds, name


def test_entry_points_refuse_bad_calls_without_a_gpu():
    from rechorus_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(256)      # non-null, aligned; never dereferenced
    odd = C.c_void_p(260)
    INVALID = -1
    err = lambda: lib.rc_last_error_string()
    assert lib.rc_cfkg_check_shape(64, 100, 4) == 0 and lib.rc_cfkg_check_shape(16, 1, 1) == 0 and lib.rc_cfkg_check_shape(128, 1, 8) == 0
    assert lib.rc_cfkg_check_shape(48, 100, 3) == INVALID and b"d=48" in err() and err().startswith(b"rc_cfkg_check_shape:")
    assert lib.rc_cfkg_check_shape(64, 0, 3) == INVALID and b"C >= 1" in err()
    assert lib.rc_cfkg_check_shape(64, 5, 0) == INVALID and b"n_rel=0 outside 1..8" in err()
    assert lib.rc_cfkg_check_shape(64, 5, 9) == INVALID and b"n_rel=9 outside 1..8" in err()
    assert [lib.rc_cfkg_fwd_bwd_rows_per_block(d) for d in (16, 32, 64, 128, 48)] == [256, 128, 64, 32, 0]

    def scores(E=p, pred=p, d=64, Cn=1, n_rel=3, B=4, n_rows=10):
        return lib.rc_cfkg_scores(E, p, p, p, p, B, Cn, d, n_rows, n_rel, pred, None)
    assert scores(E=None) == INVALID and err().startswith(b"rc_cfkg_scores: null pointer")
    assert scores(pred=None) == INVALID and b"null pointer" in err()
    assert scores(d=48) == INVALID and b"d=48" in err()
    assert scores(Cn=0) == INVALID and b"C >= 1" in err()
    assert scores(n_rel=9) == INVALID and b"n_rel=9" in err()
    assert scores(B=-1) == INVALID and b"B >= 1" in err()
    assert scores(n_rows=0) == INVALID and b"n_rows" in err()
    assert scores(E=odd) == INVALID and b"16-byte aligned" in err()
    assert scores(B=0) == 0                                                      # an empty batch: nothing to do

    def bwd(gpred=p, G=p, d=64, n_rel=3):
        return lib.rc_cfkg_scores_bwd(p, p, p, p, p, gpred, 4, 5, d, 10, n_rel, G, None)
    assert bwd(gpred=None) == INVALID and err().startswith(b"rc_cfkg_scores_bwd: null pointer")
    assert bwd(G=None) == INVALID and b"null pointer" in err()
    assert bwd(G=odd) == INVALID and b"16-byte aligned" in err()
    assert bwd(d=48) == INVALID and b"d=48" in err()
    assert bwd(n_rel=0) == INVALID and b"n_rel=0" in err()

    def fwd_bwd(E=p, GR=p, pred=None, ws=p, d=64, n_rel=4, B=100, ws_bytes=0):
        return lib.rc_cfkg_fwd_bwd(E, p, p, p, p, p, p, B, d, 1000, n_rel, 0.5, 0.01, p, pred, p, GR, ws, ws_bytes, None)
    # everything that inspects only the arguments comes before the workspace-size check: ws_bytes = 0, so a lost check would end
    # in RC_ERR_WORKSPACE, not in a launch on the made-up pointers
    assert fwd_bwd(E=None) == INVALID and err().startswith(b"rc_cfkg_fwd_bwd: null pointer")
    assert fwd_bwd(GR=None) == INVALID and b"null pointer" in err()
    assert fwd_bwd(ws=None) == INVALID and b"null pointer" in err()
    assert fwd_bwd(d=48) == INVALID and b"d=48" in err()
    assert fwd_bwd(n_rel=9) == INVALID and b"n_rel=9" in err()
    assert fwd_bwd(pred=odd) == INVALID and b"16-byte aligned" in err()
    assert fwd_bwd() == -2 and b"workspace 0 <" in err()
    need = lib.rc_cfkg_fwd_bwd_workspace_bytes(100, 64, 4)
    assert need == 2 * 4 * 64 * 4 and fwd_bwd(ws_bytes=need - 1) == -2
    sizes = [lib.rc_cfkg_fwd_bwd_workspace_bytes(n, 64, 4) for n in (0, 1, 64, 65, 1000, 65536)]
    assert sizes == sorted(sizes) and sizes[0] == sizes[1] == sizes[2] == 1024 and sizes[3] == 2048 and sizes[-1] == 1024 * 1024
    assert lib.rc_cfkg_fwd_bwd_workspace_bytes(100, 48, 4) == 0 and lib.rc_cfkg_fwd_bwd_workspace_bytes(100, 64, 9) == 0


def test_cfkg_kernels_use_no_float_atomics():
    src = open(os.path.join(ROOT, "rechorus_amd", "csrc", "cfkg.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.findall(r"atomic\w*\s*\([^;]*;", code)          # no atomic at all, integer or floating-point
    assert not re.search(r"__hip_atomic|__atomic_fetch", code)
