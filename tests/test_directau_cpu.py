"""CPU: DirectAU's host side against the reference's goldens (tests/golden/make_golden_directau.py) -- a float64 restatement of the
closed-form loss and gradient (tests/directau_np.py, the 1/S factor applied after the pair sums as the kernels do) against the
reference and against central differences, the model file's class lookup, flags, state_dict keys, init and shape envelope, and
the device pipeline's dataset kinds.  No kernel runs here."""
import argparse
import importlib
import inspect
import os
import pkgutil
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import directau_np  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

CASES = golden_cases("directau_")
GEN = os.path.join(ROOT, "tests", "golden", "make_golden_directau.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden import REF_SRC  # noqa: E402   (where the generator imports the reference from)


def _args(**kw):
    a = dict(device="cpu", model_path="", buffer=1, num_neg=0, dropout=0, test_all=0, emb_size=64, gamma=1.0)
    a.update(kw)
    return SimpleNamespace(**a)


def test_golden_cases_exist_and_fit_the_size_limit():
    assert len(CASES) == 6, CASES
    for c in CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", c + ".npz")) < 1 << 20
    ds = {int(load_golden(c)["meta"][2]) for c in CASES}
    gammas = {float(load_golden(c)["hyper"][0]) for c in CASES}
    opts = {str(load_golden(c)["opt"]) for c in CASES}
    bs = {int(load_golden(c)["meta"][3]) for c in CASES}
    assert ds == {32, 64, 128} and gammas == {0.0, 0.3, 1.0} and opts == {"SGD", "Adam", "Adagrad"}
    assert {1, 2} <= bs and any(b % 32 for b in bs if b > 2)


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="the reference exists in the build container only")
def test_generator_reruns_bit_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, GEN, "--out", str(tmp_path)], check=True, env=env, capture_output=True, timeout=900)
    for c in CASES:
        a, b = load_golden(c), np.load(os.path.join(str(tmp_path), c + ".npz"))
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (c, k)


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference(case):
    g = load_golden(case)
    gamma = float(g["hyper"][0])
    loss, GU, GI, pred = directau_np.table_grads(g["U0"], g["I0"], g["uid"], g["iid"], gamma)
    np.testing.assert_allclose(pred, g["pred"], rtol=0, atol=1e-6 * max(1.0, np.abs(g["pred"]).max()))
    if np.isnan(g["loss"]):
        assert np.isnan(loss) and g["uid"].size == 1   # B = 1: no pair, the mean of torch.pdist's empty result
    else:
        assert abs(loss - float(g["loss"])) <= 2e-6 * max(1.0, abs(float(g["loss"])))
    for got, want in ((GU, g["GU"]), (GI, g["GI"])):
        tol = 2e-5 * np.abs(want).max()
        assert np.abs(got - want).max() <= tol, (case, np.abs(got - want).max(), tol)


def test_batch_of_one_carries_the_alignment_term_only():
    """what the reference recorded for B = 1: a NaN loss, gradients of the alignment term alone"""
    g = load_golden("directau_d64_g1_adam_b1")
    assert np.isnan(g["loss"])
    u = g["U0"][g["uid"]].astype(np.float64)
    v = g["I0"][g["iid"].reshape(-1)].astype(np.float64)
    uh, du, nu = directau_np.normalize(u)
    vh, dv, nv = directau_np.normalize(v)
    gu = directau_np.unnormalize(2.0 * (uh - vh), uh, du, nu)
    np.testing.assert_allclose(g["GU"][g["uid"][0]], gu[0], rtol=1e-5, atol=1e-7)
    assert np.count_nonzero(np.abs(g["GU"]).sum(1)) == 1


@pytest.mark.parametrize("B,d,gamma,dup", [(7, 8, 0.3, False), (12, 4, 1.0, True), (5, 16, 0.0, False)])
def test_closed_form_agrees_with_central_differences(B, d, gamma, dup):
    rng = np.random.default_rng(B * d)
    u, v = rng.standard_normal((B, d)), rng.standard_normal((B, d))
    if dup:
        u[3] = u[1]
        v[4] = v[2] * 3.0
    _, _, _, _, gu, gv = directau_np.loss_and_row_grads(u, v, gamma)
    h = 1e-6
    for x, gx in ((u, gu), (v, gv)):
        num = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            old = x[idx]
            x[idx] = old + h
            lp = directau_np.loss_and_row_grads(u, v, gamma)[0]
            x[idx] = old - h
            lm = directau_np.loss_and_row_grads(u, v, gamma)[0]
            x[idx] = old
            num[idx] = (lp - lm) / (2 * h)
        np.testing.assert_allclose(gx, num, rtol=1e-5, atol=1e-7)


def test_identical_rows_give_zero_uniformity():
    x = np.tile(np.array([[0.5, -1.0, 2.0, 0.25]]), (9, 1))
    loss, align, uu, ui, gu, gv = directau_np.loss_and_row_grads(x, x, 1.0)
    assert abs(uu) < 1e-12 and abs(ui) < 1e-12 and align == 0.0
    assert np.abs(gu).max() < 1e-12 and np.abs(gv).max() < 1e-12


def test_class_lookup_flags_and_log_args():
    import main
    cls = main.find_class("model", ("DirectAU", ""))
    assert cls.__name__ == "DirectAU" and cls.reader == "BaseReader" and cls.runner == "BaseRunner"
    assert cls.extra_log_args == ["emb_size", "gamma"]
    assert cls.candidate_permutation_equivariant is True
    assert not hasattr(cls, "hip_train_step")   # the runner keeps dense updates, the reference's semantics
    d, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
    assert (d.emb_size, d.gamma, d.num_neg, d.test_all) == (64, 1.0, 1, 0)
    a, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args(["--emb_size", "32", "--gamma", "0.3"])
    assert (a.emb_size, a.gamma) == (32, 0.3)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_and_init_match_the_reference(case):
    import torch
    from models.general.DirectAU import DirectAU
    g = load_golden(case)
    n_users, n_items, d, _, seed = (int(x) for x in g["meta"])
    torch.manual_seed(seed)
    m = DirectAU(_args(emb_size=d, gamma=float(g["hyper"][0])), SimpleNamespace(n_users=n_users, n_items=n_items))
    assert sorted(m.state_dict().keys()) == sorted(g["state_keys"].tolist()) == ["i_embeddings.weight", "u_embeddings.weight"]
    # the same RNG stream as the reference's construction: two default inits, then xavier_normal_ user table, item table
    assert np.array_equal(m.u_embeddings.weight.detach().numpy(), g["U0"])
    assert np.array_equal(m.i_embeddings.weight.detach().numpy(), g["I0"])


@pytest.mark.parametrize("d", [0, 2, 30, 260, 512])
def test_envelope_raises_in_init(d):
    from models.general.DirectAU import DirectAU
    with pytest.raises(ValueError, match="envelope"):
        DirectAU(_args(emb_size=d), SimpleNamespace(n_users=5, n_items=6))


def test_check_shape_reports_the_envelope():
    from rechorus_amd import _lib, engine
    lib = _lib.load()
    for d, B in ((4, 1), (256, 1 << 20), (64, 65536), (36, 77)):
        assert lib.rc_directau_check_shape(d, B) == _lib.RC_OK, (d, B)
        assert lib.rc_directau_workspace_bytes(d, B) > 8 * B * d
        engine.directau_check_shape(d, B)
    for d, B in ((0, 4), (2, 4), (30, 4), (260, 4), (64, 0), (64, (1 << 20) + 1), (64, -1)):
        assert lib.rc_directau_check_shape(d, B) == -4, (d, B)      # RC_ERR_UNSUPPORTED
        assert b"outside the envelope" in lib.rc_last_error_string()
        assert lib.rc_directau_workspace_bytes(d, B) == 0
        with pytest.raises(ValueError, match="envelope"):
            engine.directau_check_shape(d, B)


def test_entry_points_refuse_bad_calls_without_a_gpu():
    import ctypes as C
    from rechorus_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(256)
    assert lib.rc_directau_fwd(p, None, p, None, 8, 30, 1.0, 3, p, 1 << 30, None, p, None) == -4
    assert lib.rc_directau_bwd(p, 0, 64, 1.0, 0.5, 0.5, p, 1 << 30, p, p, None) == -4
    assert lib.rc_directau_fwd(p, None, p, None, 8, 64, 1.0, 3, p, 16, None, p, None) == -1     # workspace too small
    assert b"workspace" in lib.rc_last_error_string()
    assert lib.rc_directau_fwd(None, None, p, None, 8, 64, 1.0, 3, p, 1 << 30, None, p, None) == -1
    assert b"null pointer" in lib.rc_last_error_string()
    assert lib.rc_directau_fwd(p, None, p, None, 8, 64, 1.0, 4, p, 1 << 30, None, p, None) == -1   # sets is a 2-bit mask


def test_engine_wrappers_raise_outside_the_envelope_without_touching_the_gpu():
    import torch
    from rechorus_amd import engine
    with pytest.raises(ValueError, match="envelope"):
        engine.directau_fwd(torch.zeros(3, 30), torch.zeros(3, 30))
    with pytest.raises(ValueError, match="envelope"):
        engine.directau_bwd(torch.zeros(1), 0, 64, (1.0, 0.5, 0.5), torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\[batch, 64\]"):
        engine.directau_fwd(torch.zeros(3, 64), torch.zeros(4, 64))


# the parent commit's kinds: DirectAU is the only new entry, every other class keeps its kind
KINDS = {"BPRMF": "general", "BPRMFImpression": "impression", "LightGCN": "general", "LightGCNImpression": "impression",
         "NeuMF": "general", "SASRec": "sequential", "SASRecImpression": "impression_seq", "DeepFMCTR": "ctr", "DeepFMTopK": "context",
         "FMCTR": "ctr", "FMTopK": "context", "WideDeepCTR": "ctr", "WideDeepTopK": "context", "DirectAU": "general_unsampled"}


def test_dataset_kind_of_every_model_class():
    from models.BaseModel import BaseModel
    from rechorus_amd import pipeline
    got = {}
    for sub in ("general", "sequential", "context"):
        pkg = importlib.import_module("models." + sub)
        for m in pkgutil.iter_modules(pkg.__path__):
            mod = importlib.import_module("models.{}.{}".format(sub, m.name))
            for name, c in vars(mod).items():
                if inspect.isclass(c) and issubclass(c, BaseModel) and c.__module__ == mod.__name__:
                    got[name] = pipeline.dataset_kind(object.__new__(c.Dataset))
    assert got == KINDS


def test_unsampled_kind_is_not_inherited_by_an_override():
    """a subclass that samples its own negatives again keeps the DataLoader path"""
    from models.general.DirectAU import DirectAU
    from rechorus_amd import pipeline

    class Resampled(DirectAU.Dataset):
        def actions_before_epoch(self):
            self.data['neg_items'] = [[1] for _ in range(len(self))]

    class Plain(DirectAU.Dataset):
        pass
    assert pipeline.dataset_kind(object.__new__(Resampled)) is None
    assert pipeline.dataset_kind(object.__new__(Plain)) == "general_unsampled"


def test_dataset_writes_empty_negative_lists():
    from models.general.DirectAU import DirectAU
    ds = object.__new__(DirectAU.Dataset)
    ds.data = {"user_id": np.array([1, 2, 3]), "item_id": np.array([4, 5, 6])}
    ds.actions_before_epoch()
    assert ds.data["neg_items"] == [[], [], []]


def test_directau_kernels_use_no_float_atomics():
    src = open(os.path.join(ROOT, "rechorus_amd", "csrc", "directau.hip")).read()
    assert not re.search(r"atomic\w*\s*\(|__hip_atomic|__atomic", src)


def test_no_pdist_or_cdist_on_the_package_path():
    hits = []
    for base, _, files in os.walk(os.path.join(ROOT, "rechorus_amd")):
        for f in files:
            if f.endswith(".py"):
                p = os.path.join(base, f)
                if re.search(r"\b(pdist|cdist)\s*\(", open(p).read()):
                    hits.append(p)
    assert not hits, hits
