"""CPU: FPMC's host side -- the float64 restatement (tests/fpmc_np.py) against the reference's own numbers
(tests/golden/fpmc_*.npz, written by tests/golden/make_golden_fpmc.py), the model file's class lookup, flags, state_dict keys and
shape check, the Dataset's feed dict, the device pipeline's dataset kind, and the C entry points' refusals.  No kernel runs.

Tolerances: the goldens are float32 results of the reference, the restatement is float64: conftest.assert_close at its default
1e-5 (relative to the entry plus 1e-5 of the tensor's largest entry)."""
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
import fpmc_np  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

CASES = golden_cases("fpmc_")


def _args(**kw):
    a = dict(device="cpu", model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=64, history_max=20)
    a.update(kw)
    return SimpleNamespace(**a)


def test_golden_cases_exist_and_fit_the_size_limit():
    assert tuple(CASES) == tuple(sorted(fpmc_np.GOLDEN_CASES))
    shapes = set()
    for c in CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", c + ".npz")) < 512 << 10
        g = load_golden(c)
        n_users, n_items, d, B, K, seed, redraw = (int(x) for x in g["meta"])
        assert n_users <= 64 and n_items <= 300
        shapes.add((str(g["opt"]), d, B, K, float(g["hyper"][1])))
        assert g["iid"].shape == (B, 1 + K) and g["uid"].shape == (B,) and g["lid"].shape == (B,)
        if B > 1:   # ids repeat: across tuples on every side
            assert len(np.unique(g["uid"])) < B and len(np.unique(g["lid"])) < B and len(np.unique(g["iid"])) < g["iid"].size
        if K >= 2:
            assert g["iid"][0, 1] == g["iid"][0, 0] and g["iid"][0, 2] == g["iid"][0, 1]
        assert g["lid"][B - 1] in g["iid"][B - 1]
    assert shapes == {("SGD", 16, 1, 1, 1e-5), ("SGD", 32, 160, 4, 0.0), ("Adam", 64, 77, 99, 1e-6), ("Adagrad", 128, 33, 9, 1e-4)}


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference(case):
    g = load_golden(case)
    T = [g[k + "0"] for k in fpmc_np.TABLES]
    uid, lid, iid = g["uid"], g["lid"], g["iid"]
    pred = fpmc_np.scores(*T, uid, lid, iid)
    assert_close(g["pred"], pred, what=case + " pred")
    loss_vec, gpred = fpmc_np.bpr(pred)
    assert_close(float(g["loss"]), loss_vec.mean(), what=case + " loss")
    grads = dict(zip(fpmc_np.TABLES, fpmc_np.dense_grads(*T, uid, lid, iid, gpred)))
    for k in fpmc_np.TABLES:
        assert_close(g["G" + k], grads[k], what=f"{case} G{k}")
    # torch.optim's step is dense: weight decay reaches every row
    lr, l2 = (float(x) for x in g["hyper"])
    opt = str(g["opt"])
    for k in fpmc_np.TABLES:
        W1, _, _ = fpmc_np.optimizer_rows(g[k + "0"], grads[k], np.arange(g[k + "0"].shape[0]), opt, lr, l2)
        # looser than 2e-5 for Adam / Adagrad, the reason being conftest.assert_update_close's: the first step is
        # lr * g / (|g| + eps), ill-conditioned where |g| ~ eps -- with the native N(0, 0.01) init and l2 = 1e-6 the rows outside
        # the batch have |g| = l2 |w| ~ 1e-8 = eps, so the reference's own fp32 rounding of g moves its step by 1e-4 relative
        assert_update_close(g[k + "1"], g[k + "0"], W1, what=f"{case} {k} update", rtol=2e-5,
                            extra_atol=0.0 if opt == "SGD" else 1e-3 * lr, strict=True)


def test_restated_gradients_agree_with_autograd_in_float64():
    import torch
    rng = np.random.default_rng(7)
    n_users, n_items, d, B, Cn = 5, 9, 6, 8, 5
    T = [rng.normal(0, 0.5, (n, d)) for n in (n_users, n_items, n_items, n_items)]
    uid, lid, iid = rng.integers(0, n_users, B), rng.integers(0, n_items, B), rng.integers(0, n_items, (B, Cn))
    iid[0, 1] = iid[0, 0]
    tt = [torch.tensor(t, requires_grad=True) for t in T]
    UI, LI, IU, IL = tt
    pred = (UI[uid][:, None, :] * IU[iid]).sum(-1) + (LI[lid][:, None, :] * IL[iid]).sum(-1)
    pos, neg = pred[:, 0], pred[:, 1:]
    loss = -(((pos[:, None] - neg).sigmoid() * (neg - neg.max()).softmax(dim=1)).sum(dim=1)).log().mean()
    loss.backward()
    mine = fpmc_np.scores(*T, uid, lid, iid)
    assert np.abs(mine - pred.detach().numpy()).max() <= 1e-12
    loss_vec, gpred = fpmc_np.bpr(mine)
    assert abs(loss_vec.mean() - loss.item()) <= 1e-12
    for got, t in zip(fpmc_np.dense_grads(*T, uid, lid, iid, gpred), tt):
        assert np.abs(got - t.grad.numpy()).max() <= 1e-12


def test_class_lookup_flags_and_log_args():
    import main
    cls = main.find_class("model", ("FPMC", ""))
    assert cls.__name__ == "FPMC" and cls.reader == "SeqReader" and cls.runner == "BaseRunner"
    assert cls.extra_log_args == ["emb_size"]
    assert cls.candidate_permutation_equivariant is True
    assert hasattr(cls, "hip_train_step") and hasattr(cls, "hip_rowwise_supported") and not hasattr(cls, "full_catalogue_vectors")
    d, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
    assert (d.emb_size, d.history_max, d.num_neg, d.test_all) == (64, 20, 1, 0)


def _added_flags(add):
    p = argparse.ArgumentParser()
    before = {s for a in p._actions for s in a.option_strings}
    p = add(p)
    return sorted({s for a in p._actions for s in a.option_strings} - before)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_and_flags_equal_the_recorded_reference(case):
    from helpers.SeqReader import SeqReader
    from models.sequential.FPMC import FPMC
    g = load_golden(case)
    n_users, n_items, d = (int(x) for x in g["meta"][:3])
    m = FPMC(_args(emb_size=d), SimpleNamespace(n_users=n_users, n_items=n_items))
    want = ["il_embeddings.weight", "iu_embeddings.weight", "li_embeddings.weight", "ui_embeddings.weight"]
    assert sorted(m.state_dict().keys()) == sorted(g["state_keys"].tolist()) == want
    for key, full in (("UI", "ui_embeddings.weight"), ("IU", "iu_embeddings.weight"), ("LI", "li_embeddings.weight"),
                      ("IL", "il_embeddings.weight")):
        assert tuple(m.state_dict()[full].shape) == g[key + "0"].shape
    assert 0.005 < float(m.iu_embeddings.weight.detach().std()) < 0.02          # BaseModel.init_weights: N(0, 0.01)
    # the flags the model and its reader add are the reference's, as the generator recorded them
    assert _added_flags(FPMC.parse_model_args) == g["model_flags"].tolist()
    assert "--emb_size" in g["model_flags"].tolist() and "--history_max" in g["model_flags"].tolist()
    assert _added_flags(SeqReader.parse_data_args) == g["reader_flags"].tolist()


def test_unsupported_emb_size_is_refused_at_construction_with_the_flag_named():
    from models.sequential.FPMC import FPMC
    with pytest.raises(ValueError, match=r"--emb_size 48.*16, 32, 64, 128"):
        FPMC(_args(emb_size=48), SimpleNamespace(n_users=5, n_items=6))
    m = FPMC(_args(emb_size=16), SimpleNamespace(n_users=5, n_items=6))
    assert m.hip_rowwise_supported()


def _synthetic_corpus():
    """three users; user 2's first instance has position 0 (dropped), so its first KEPT instance has position 1"""
    import pandas as pd
    his = {1: [(4, 10), (2, 11), (5, 12), (3, 13)], 2: [(6, 20), (1, 21)], 3: [(2, 30), (2, 31), (7, 32)]}
    rows = [(u, i, t, p) for u, seq in his.items() for p, (i, t) in enumerate(seq)]
    df = pd.DataFrame(rows, columns=["user_id", "item_id", "time", "position"])
    df["neg_items"] = [[1 + (k % 7), 1 + ((k + 3) % 7)] for k in range(len(df))]
    return SimpleNamespace(n_users=4, n_items=8, user_his=his, data_df={"train": df.drop(columns="neg_items"), "test": df},
                           train_clicked_set={u: {i for i, _ in s} for u, s in his.items()}, residual_clicked_set={})


def test_dataset_feed_dict_reproduces_the_last_item():
    from models.sequential.FPMC import FPMC
    corpus = _synthetic_corpus()
    for test_all in (0, 1):
        model = SimpleNamespace(test_all=test_all, buffer=0, history_max=20, num_neg=2)
        ds = FPMC.Dataset(model, corpus, "test")
        assert len(ds) == 6                                        # the three position-0 instances are dropped
        seen = []
        for k in range(len(ds)):
            f = ds[k]
            assert sorted(f) == ["item_id", "last_item_id", "user_id"]
            u, pos = ds.data["user_id"][k], ds.data["position"][k]
            assert f["user_id"] == u and f["last_item_id"] == corpus.user_his[u][pos - 1][0]
            assert f["item_id"][0] == corpus.user_his[u][pos][0]
            if test_all:
                assert f["item_id"][1:].tolist() == list(range(1, corpus.n_items))
            else:
                assert f["item_id"][1:].tolist() == ds.data["neg_items"][k]
            seen.append((u, pos, f["last_item_id"]))
        assert (2, 1, 6) in seen and (1, 3, 5) in seen and (3, 1, 2) in seen


def test_dataset_kind():
    from models.BaseModel import GeneralModel, SequentialModel
    from models.general.BPRMF import BPRMF
    from models.general.DirectAU import DirectAU
    from models.sequential.FPMC import FPMC
    from models.sequential.SASRec import SASRec
    from rechorus_amd import pipeline
    kind = lambda cls: pipeline.dataset_kind(object.__new__(cls))
    assert kind(FPMC.Dataset) == "last_item"
    assert kind(BPRMF.Dataset) == "general" and kind(SASRec.Dataset) == "sequential" and kind(DirectAU.Dataset) == "general_unsampled"
    assert kind(GeneralModel.Dataset) == "general" and kind(SequentialModel.Dataset) == "sequential"

    class Again(FPMC.Dataset):       # a subclass with a feed dict of its own does not inherit the declaration
        def _get_feed_dict(self, index):
            return {}
    assert kind(Again) is None

    class Resampled(FPMC.Dataset):   # ... and one with its own negative sampling keeps the DataLoader path
        def actions_before_epoch(self):
            pass
    assert kind(Resampled) is None


def test_entry_points_refuse_bad_calls_without_a_gpu():
    from rechorus_amd import _lib
    lib = _lib.load()
    p, q, r, s, t = (C.c_void_p(256 * k) for k in range(1, 6))      # non-null, aligned, distinct; never dereferenced
    INVALID = -1
    err = lambda: lib.rc_last_error_string()
    assert lib.rc_fpmc_check_shape(64, 100) == 0 and lib.rc_fpmc_check_shape(16, 1) == 0
    assert lib.rc_fpmc_check_shape(48, 100) == INVALID and b"d=48" in err()
    assert lib.rc_fpmc_check_shape(64, 0) == INVALID and b"C >= 1" in err()

    def scores(UI=p, pred=p, d=64, Cn=1):
        return lib.rc_fpmc_scores(UI, q, r, s, p, p, p, 4, Cn, d, pred, None)
    assert scores(UI=None) == INVALID and err().startswith(b"rc_fpmc_scores: null pointer")
    assert scores(pred=None) == INVALID and b"null pointer" in err()
    assert scores(d=48) == INVALID and b"d=48" in err()
    assert scores(Cn=0) == INVALID and b"C >= 1" in err()

    def fwd_bwd(UI=p, lgrad=p, d=64, Cn=2):
        return lib.rc_fpmc_fwd_bwd(UI, q, r, s, p, p, p, 4, Cn, d, 0.25, None, p, p, p, lgrad, None)
    assert fwd_bwd(UI=None) == INVALID and err().startswith(b"rc_fpmc_fwd_bwd: null pointer")
    assert fwd_bwd(lgrad=None) == INVALID and b"null pointer" in err()
    assert fwd_bwd(d=48) == INVALID and b"d=48" in err()
    assert fwd_bwd(Cn=1) == INVALID and b"C >= 2" in err()

    h = C.byref(_lib.OptHyper(opt=_lib.RC_OPT_SGD, lr=0.1))
    adam = C.byref(_lib.OptHyper(opt=_lib.RC_OPT_ADAM, lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, step=1))

    def upd(IU=r, IL=s, UI=p, d=64, dense=(None, None), heads=p, hyper=h, ws_bytes=0):
        return lib.rc_fpmc_item_update(IU, None, None, IL, None, None, d, p, p, 100, p, UI, q, p, p, 4, hyper, dense[0], dense[1],
                                       heads, heads, p, ws_bytes, None)
    # everything that inspects only the arguments comes before the workspace-size check: ws_bytes = 0, so a lost check would end
    # in RC_ERR_WORKSPACE, not in a launch on the made-up pointers
    for dense in ((p, None), (None, p)):
        assert upd(dense=dense) == INVALID and b"both dense gradients or none" in err()
    assert upd(UI=None) == INVALID and err().startswith(b"rc_fpmc_item_update: null pointer")
    assert upd(heads=None) == INVALID and b"head list" in err()
    assert upd(IU=None) == INVALID and b"no output" in err()
    assert upd(d=48) == INVALID and b"d=48" in err()
    assert upd(UI=r) == INVALID and b"distinct" in err()
    assert upd(hyper=None) == INVALID and b"hyper-parameters missing" in err()
    assert upd(hyper=adam) == INVALID and b"Adam needs m and v" in err()
    assert upd() == -2 and b"workspace 0 <" in err()
    assert upd(dense=(p, q)) == -2 and b"workspace 0 <" in err()
    assert lib.rc_fpmc_item_update_workspace_bytes(100, 64) >= 256 + 4 * (100 // 33 + 1)


def test_fwd_bwd_layout_envelope():
    """the register path's envelope as the dispatcher reports it (host logic): C <= 264 / 200 / 100 / 50 at d = 16 / 32 / 64 / 128,
    streaming beyond; d = 64 with C = 100, the benchmark shape, holds 50 pair rows per lane-group in registers"""
    from rechorus_amd import engine
    assert engine.fpmc_fwd_bwd_layout(64, 100) == (2, 50)
    for d, top in ((16, 264), (32, 200), (64, 100), (128, 50)):
        assert engine.fpmc_fwd_bwd_layout(d, top) is not None and engine.fpmc_fwd_bwd_layout(d, top + 1) is None
        assert engine.fpmc_fwd_bwd_layout(d, 2) is not None and engine.fpmc_fwd_bwd_layout(d, 1) is None
        for Cn in range(2, top + 1):
            gs, cpl = engine.fpmc_fwd_bwd_layout(d, Cn)
            assert gs * cpl >= Cn and gs * (d // 2) <= 64 and cpl <= 50
    assert engine.fpmc_fwd_bwd_layout(48, 10) is None


def test_fpmc_kernels_use_no_float_atomics():
    src = open(os.path.join(ROOT, "rechorus_amd", "csrc", "fpmc.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    atomics = re.findall(r"atomic\w*\s*\([^;]*;", code)
    assert len(atomics) == 1 and "a.n_long, 1u" in atomics[0]        # the one integer ticket of the long-row list
    assert not re.search(r"__hip_atomic|__atomic_fetch", code)
