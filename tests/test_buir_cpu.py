"""CPU: BUIR's host side against the reference's goldens (tests/golden/make_golden_buir.py) -- a float64 restatement of the loss, its
four gradients, the scoring identity and the separately-rounded fp32 target update (tests/buir_np.py) against the reference and
against central differences; the model file's and the runner's class lookup, flags, state_dict keys, the init stream, frozen
targets, the dataset kind and the shape envelope at every layer.  No kernel runs here."""
import argparse
import ctypes as C
import os
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
import buir_np  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

CASES = golden_cases("buir_")
GEN = os.path.join(ROOT, "tests", "golden", "make_golden_buir.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden import REF_SRC  # noqa: E402   (where the generator imports the reference from)

TOL = 2e-5
KEYS = ["item_online.weight", "item_target.weight", "predictor.bias", "predictor.weight", "user_online.weight", "user_target.weight"]


def _args(**kw):
    a = dict(device="cpu", model_path="", buffer=1, num_neg=0, dropout=0, test_all=0, emb_size=64, momentum=0.995)
    a.update(kw)
    return SimpleNamespace(**a)


def _close(got, want, what, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max())
    assert err <= tol * scale, f"{what}: max |diff| {err:.3e} > {tol:g} * {scale:.3e}"


def _model(case):
    import torch
    from models.general.BUIR import BUIR
    g = load_golden(case)
    n_users, n_items, d, _, seed, _ = (int(x) for x in g["meta"])
    torch.manual_seed(seed)
    return g, BUIR(_args(emb_size=d, momentum=float(g["hyper"][0])), SimpleNamespace(n_users=n_users, n_items=n_items))


def test_golden_cases_exist_and_fit_the_size_limit():
    assert len(CASES) == 5, CASES
    for c in CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", c + ".npz")) < 600 << 10   # the largest golden before these
        g = load_golden(c)
        assert max(int(g["meta"][0]), int(g["meta"][1])) <= 300
    shapes = {(int(load_golden(c)["meta"][2]), int(load_golden(c)["meta"][3]), str(load_golden(c)["opt"])) for c in CASES}
    assert shapes == {(64, 77, "Adam"), (32, 160, "SGD"), (128, 33, "Adagrad"), (16, 1, "SGD"), (64, 2, "Adam")}
    assert sorted(int(load_golden(c)["meta"][5]) for c in CASES) == [0, 1, 1, 1, 1]   # one native init, the others re-drawn
    for c in CASES:   # Zipf batches: ids repeat inside every batch that is large enough
        g = load_golden(c)
        if len(g["uid"]) >= 33:
            assert len(set(g["uid"].tolist())) < len(g["uid"]) and len(set(g["iid"].reshape(-1).tolist())) < len(g["uid"])


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
    loss, pred, GU, GI, dW, db = buir_np.table_grads(g["UO0"], g["UT0"], g["IO0"], g["IT0"], g["W0"], g["b0"], g["uid"], g["iid"])
    _close(pred, g["pred"], case + " pred")
    assert abs(loss - float(g["loss"])) <= 2e-6 * max(1.0, abs(float(g["loss"])))
    for got, key in ((GU, "GUO"), (GI, "GIO"), (dW, "GW"), (db, "Gb")):
        _close(got, g[key], case + " " + key)


@pytest.mark.parametrize("B,d,dup,g0", [(7, 8, False, 1.0), (12, 4, True, 3.0), (1, 16, False, 1.0)])
def test_closed_form_agrees_with_central_differences(B, d, dup, g0):
    rng = np.random.default_rng(B * d)
    uo, ut, io, it = (rng.standard_normal((B, d)) for _ in range(4))
    W, b = rng.standard_normal((d, d)) / np.sqrt(d), rng.standard_normal(d)
    if dup:
        uo[3], io[3], ut[3], it[3] = uo[1], io[1], ut[1], it[1]
    _, _, duo, dio, dW, db = buir_np.row_grads(uo, ut, io, it, W, b, g0)
    h = 1e-6
    for x, gx in ((uo, duo), (io, dio), (W, dW), (b, db)):
        num = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            old = x[idx]
            x[idx] = old + h
            lp = buir_np.row_grads(uo, ut, io, it, W, b)[0]
            x[idx] = old - h
            lm = buir_np.row_grads(uo, ut, io, it, W, b)[0]
            x[idx] = old
            num[idx] = g0 * (lp - lm) / (2 * h)
        np.testing.assert_allclose(gx, num, rtol=2e-5, atol=1e-7)


def test_zero_target_row_is_finite_in_the_forward_pass():
    rng = np.random.default_rng(0)
    uo, ut, io, it = (rng.standard_normal((3, 8)) for _ in range(4))
    it[1] = 0.0
    W, b = rng.standard_normal((8, 8)), rng.standard_normal(8)
    loss = buir_np.row_grads(uo, ut, io, it, W, b)[0]
    assert np.isfinite(loss)


@pytest.mark.parametrize("case", CASES)
def test_oracle_ema_is_bit_equal_to_the_reference(case):
    g = load_golden(case)
    m = float(g["hyper"][0])
    for t in ("U", "I"):
        for step in (1, 2):
            got = buir_np.ema(g[f"{t}T{step - 1}"], g[f"{t}O{step}"], m)
            assert got.dtype == np.float32 and np.array_equal(got, g[f"{t}T{step}"]), (case, t, step)
    # a single rounding (fused multiply-add, emulated in double) is NOT what the reference computes
    t, o = g["UT0"].astype(np.float64), g["UO1"].astype(np.float64)
    fused = (np.float64(np.float32(m)) * t + (o * np.float64(np.float32(1.0 - m))).astype(np.float32)).astype(np.float32)
    if g["UT0"].size >= 1000 and not np.array_equal(g["UT0"], g["UO1"]):
        assert not np.array_equal(fused, g["UT1"])


@pytest.mark.parametrize("case", CASES)
def test_scoring_identity_reproduces_the_eval_predictions(case):
    g = load_golden(case)
    args = (g["UO2"], g["IO2"], g["W2"], g["b2"], g["eval_uid"], g["eval_iid"])
    _close(buir_np.scores_reference_order(*args), g["eval_pred"], case + " reference order", 2e-6)
    _close(buir_np.scores(*args), g["eval_pred"], case + " <q, i> + c", 2e-6)


def test_class_lookup_flags_and_log_args():
    import main
    from helpers.BaseRunner import BaseRunner
    cls = main.find_class("model", ("BUIR", ""))
    assert cls.__name__ == "BUIR" and cls.reader == "BaseReader" and cls.runner == "BUIRRunner"
    assert cls.extra_log_args == ["emb_size", "momentum"]
    assert cls.candidate_permutation_equivariant is True
    assert not hasattr(cls, "hip_train_step")   # dense updates, the reference's semantics
    d, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
    assert (d.emb_size, d.momentum, d.num_neg, d.test_all) == (64, 0.995, 1, 0)
    a, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args(["--emb_size", "32", "--momentum", "0.9"])
    assert (a.emb_size, a.momentum) == (32, 0.9)
    runner = main.find_class("helper", cls.runner)
    assert runner.__name__ == "BUIRRunner" and issubclass(runner, BaseRunner)
    assert runner.fit is BaseRunner.fit and runner._after_step is not BaseRunner._after_step


def test_runner_moves_the_targets_after_every_step_and_refuses_rowwise():
    from helpers.BaseRunner import BaseRunner
    from helpers.BUIRRunner import BUIRRunner
    calls = []
    model = SimpleNamespace(_update_target=lambda: calls.append(1))
    r = object.__new__(BUIRRunner)
    r._after_step(model)
    assert calls == [1]
    assert BaseRunner._after_step(object.__new__(BaseRunner), model) is None and calls == [1]
    r.engine = "auto"
    assert r._use_rowwise(model) is False
    r.engine = "rowwise"
    with pytest.raises(ValueError, match="row-wise"):
        r._use_rowwise(model)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_init_stream_and_frozen_targets(case):
    g, m = _model(case)
    assert sorted(m.state_dict().keys()) == sorted(g["state_keys"].tolist()) == KEYS
    # the same RNG stream as the reference's construction: five default inits, then Xavier-normal on the four tables and W, a
    # normal bias.  W and b are what the stream leaves in every case, the tables in the case that keeps the native init
    assert np.array_equal(m.predictor.weight.detach().numpy(), g["W0"])
    assert np.array_equal(m.predictor.bias.detach().numpy(), g["b0"])
    if int(g["meta"][5]) == 0:
        assert np.array_equal(m.user_online.weight.detach().numpy(), g["UO0"])
        assert np.array_equal(m.item_online.weight.detach().numpy(), g["IO0"])
    for online, target in ((m.user_online, m.user_target), (m.item_online, m.item_target)):
        assert np.array_equal(online.weight.detach().numpy(), target.weight.detach().numpy())
        assert online.weight.requires_grad and not target.weight.requires_grad
        assert online.weight.data_ptr() != target.weight.data_ptr()
    trained = [p for grp in m.customize_parameters() for p in grp["params"]]
    assert {id(p) for p in trained} == {id(m.user_online.weight), id(m.item_online.weight), id(m.predictor.weight), id(m.predictor.bias)}
    assert not list(m.buffers())


@pytest.mark.parametrize("d", [0, 8, 24, 72, 144, 256])
def test_envelope_raises_in_init(d):
    from models.general.BUIR import BUIR
    with pytest.raises(ValueError, match="envelope"):
        BUIR(_args(emb_size=d), SimpleNamespace(n_users=5, n_items=6))


def test_check_shape_reports_the_envelope():
    from rechorus_amd import _lib, engine
    lib = _lib.load()
    for d in range(16, 129, 16):
        for B in (1, 77, 1 << 20):
            assert lib.rc_buir_check_shape(d, B) == _lib.RC_OK, (d, B)
            assert lib.rc_buir_workspace_bytes(d, B) >= 4 * (d * d + d + 4)
            engine.buir_check_shape(d, B)
    assert lib.rc_buir_workspace_bytes(128, 1 << 20) <= 64 << 20      # the partials are capped, not one per tile
    for d, B in ((0, 4), (8, 4), (24, 4), (144, 4), (256, 4), (64, 0), (64, (1 << 20) + 1), (64, -1)):
        assert lib.rc_buir_check_shape(d, B) == -4, (d, B)      # RC_ERR_UNSUPPORTED
        assert b"outside the envelope" in lib.rc_last_error_string()
        assert lib.rc_buir_workspace_bytes(d, B) == 0
        with pytest.raises(ValueError, match="envelope"):
            engine.buir_check_shape(d, B)


def test_entry_points_refuse_bad_calls_without_a_gpu():
    from rechorus_amd import _lib
    lib = _lib.load()
    p, q = C.c_void_p(256), C.c_void_p(260)      # never dereferenced; q is not 16-byte aligned
    big = 1 << 30
    INVALID, UNSUPPORTED = -1, -4

    def fwd(d=64, B=8, ws=p, ws_bytes=big, uo=p, loss=p, uid=p):
        return lib.rc_buir_fwd(uo, p, p, p, p, p, uid, p, B, d, ws, ws_bytes, None, loss, None)

    def bwd(d=64, B=8, ws=p, ws_bytes=big, g=p, dW=p, gu=p):
        return lib.rc_buir_bwd(p, p, p, p, p, p, p, p, g, B, d, ws, ws_bytes, gu, p, dW, p, None)
    table = [
        (lambda: fwd(d=24), UNSUPPORTED, b"outside the envelope"), (lambda: fwd(B=0), UNSUPPORTED, b"outside the envelope"),
        (lambda: bwd(d=144), UNSUPPORTED, b"outside the envelope"), (lambda: bwd(B=(1 << 20) + 1), UNSUPPORTED, b"outside the envelope"),
        (lambda: fwd(ws_bytes=16), INVALID, b"workspace"), (lambda: bwd(ws_bytes=16), INVALID, b"workspace"),
        (lambda: fwd(ws=None), INVALID, b"workspace"), (lambda: fwd(ws=q), INVALID, b"workspace"),
        (lambda: fwd(uo=None), INVALID, b"null pointer"), (lambda: fwd(loss=None), INVALID, b"null pointer"),
        (lambda: fwd(uid=None), INVALID, b"null pointer"), (lambda: fwd(uo=q), INVALID, b"16-byte aligned"),
        (lambda: bwd(g=None), INVALID, b"null pointer"), (lambda: bwd(dW=None), INVALID, b"null pointer"),
        (lambda: bwd(gu=None), INVALID, b"null pointer"), (lambda: bwd(gu=q), INVALID, b"16-byte aligned"),
        (lambda: lib.rc_buir_query(p, p, p, p, 8, 20, p, p, None), UNSUPPORTED, b"outside the envelope"),
        (lambda: lib.rc_buir_query(p, None, p, p, 8, 64, p, p, None), INVALID, b"null pointer"),
        (lambda: lib.rc_buir_query(p, p, p, p, 8, 64, p, None, None), INVALID, b"null pointer"),
        (lambda: lib.rc_buir_scores(p, p, p, p, 8, 100, 20, p, None), UNSUPPORTED, b"outside the envelope"),
        (lambda: lib.rc_buir_scores(p, p, p, p, 8, 0, 64, p, None), INVALID, b"candidates"),
        (lambda: lib.rc_buir_scores(p, p, p, p, 1 << 20, 1 << 20, 64, p, None), INVALID, b"candidates"),
        (lambda: lib.rc_buir_scores(p, p, None, p, 8, 100, 64, p, None), INVALID, b"null pointer"),
        (lambda: lib.rc_buir_scores(q, p, p, p, 8, 100, 64, p, None), INVALID, b"16-byte aligned"),
        (lambda: lib.rc_buir_ema(None, p, 64, p, p, 64, 0.995, None), INVALID, b"null pointer"),
        (lambda: lib.rc_buir_ema(p, p, 64, p, None, 64, 0.995, None), INVALID, b"null pointer"),
        (lambda: lib.rc_buir_ema(p, p, -1, p, p, 64, 0.995, None), INVALID, b"negative"),
        (lambda: lib.rc_buir_ema(p, p, 0, p, p, 0, 0.995, None), INVALID, b"both 0"),
        (lambda: lib.rc_buir_ema(p, q, 64, p, p, 64, 0.995, None), INVALID, b"16-byte aligned"),
    ]
    for i, (call, code, text) in enumerate(table):
        got = call()
        msg = lib.rc_last_error_string()
        assert got == code and text in msg, (i, got, msg)


def test_engine_wrappers_raise_outside_the_envelope_without_touching_the_gpu():
    import torch
    from rechorus_amd import engine, nn as hnn
    ids = torch.zeros(3, dtype=torch.int64)
    for d in (24, 144):
        tabs = [torch.zeros(5, d) for _ in range(4)]
        W, b = torch.zeros(d, d), torch.zeros(d)
        with pytest.raises(ValueError, match="envelope"):
            engine.buir_fwd(*tabs, W, b, ids, ids)
        with pytest.raises(ValueError, match="envelope"):
            engine.buir_bwd(torch.ones(1), *tabs, W, b, ids, ids)
        with pytest.raises(ValueError, match="envelope"):
            engine.buir_query(tabs[0], W, b, ids)
        with pytest.raises(ValueError, match="envelope"):
            engine.buir_scores(torch.zeros(3, d), torch.zeros(3), tabs[2], torch.zeros(3, 4, dtype=torch.int64))
        with pytest.raises(ValueError, match="envelope"):
            hnn.buir_loss(*tabs, W, b, ids, ids)
    tabs = [torch.zeros(5, 64) for _ in range(4)]
    with pytest.raises(ValueError, match="envelope"):
        engine.buir_fwd(*tabs, torch.zeros(64, 64), torch.zeros(64), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"weight \[d, d\]"):
        engine.buir_fwd(*tabs, torch.zeros(32, 64), torch.zeros(64), ids, ids)
    with pytest.raises(ValueError, match="one positive item per row"):
        engine.buir_fwd(*tabs, torch.zeros(64, 64), torch.zeros(64), ids, torch.zeros(3, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="differ in shape"):
        engine.ema_update(torch.zeros(4, 64), torch.zeros(5, 64), torch.zeros(4, 64), torch.zeros(4, 64), 0.9)
    with pytest.raises(ValueError, match="GPU"):      # inside the envelope: the only thing missing is the device
        engine.buir_fwd(*tabs, torch.zeros(64, 64), torch.zeros(64), ids, ids)


def test_dataset_kind_and_empty_negative_lists():
    from models.general.BUIR import BUIR
    from rechorus_amd import pipeline
    assert pipeline.dataset_kind(object.__new__(BUIR.Dataset)) == "general_unsampled"
    ds = object.__new__(BUIR.Dataset)
    ds.data = {"user_id": np.array([1, 2, 3]), "item_id": np.array([4, 5, 6])}
    ds.actions_before_epoch()
    assert ds.data["neg_items"] == [[], [], []]


def test_model_refuses_the_cpu_and_a_loss_on_the_prediction_is_impossible():
    import torch
    _, m = _model("buir_d16_sgd_b1")
    with pytest.raises(RuntimeError, match="GPU only"):
        m({"user_id": torch.tensor([1]), "item_id": torch.tensor([[2]]), "batch_size": 1, "phase": "train"})
    src = open(os.path.join(ROOT, "rechorus_amd", "nn.py")).read()
    assert "ctx.mark_non_differentiable(pred)" in src


def test_buir_kernels_use_no_float_atomics_and_keep_the_ema_unfused():
    src = open(os.path.join(ROOT, "rechorus_amd", "csrc", "buir.hip")).read()
    assert not re.search(r"atomic\w*\s*\(|__hip_atomic|__atomic", src)
    ema = src[src.index("void buir_ema_kernel"):src.index("// the one statement of the envelope")]
    assert "#pragma clang fp contract(off)" in ema and "fmaf" not in ema


def test_no_torch_normalize_or_linear_on_the_buir_path():
    for rel in ("rechorus_amd/rechorus/models/buir_model.py", "rechorus_amd/rechorus/helpers/BUIRRunner.py"):
        text = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"F\.normalize|F\.linear|functional", text), rel
