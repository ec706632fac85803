"""CPU: ComiRec's host side against the reference's goldens (tests/golden/make_golden_comirec.py) -- the float64 restatement of
forward, hard selection and hand-derived backward (tests/comirec_np.py) against the reference and against torch autograd, the
model file's class lookup, flags, state_dict keys and shape envelope, and the device pipeline's dataset kind.  No kernel runs.

Tolerances: the goldens are float32 results of the reference, the restatement is float64: 2e-5 of the tensor's largest entry.
The gradient of W2's bias is exactly 0 in exact arithmetic (a softmax is invariant to a shift of its row), the reference's
value is pure round-off: it gets an absolute floor of 1e-5 of W2's largest weight gradient; the other attention-path gradients
get one of 1e-6 of the batch's largest gradient entry (grad_floor: they are exact zeros at L = 1)."""
import argparse
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
import comirec_np  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

CASES = golden_cases("comirec_")
GEN = os.path.join(ROOT, "tests", "golden", "make_golden_comirec.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden import REF_SRC  # noqa: E402   (where the generator imports the reference from)

from comirec_np import PARAM_KEYS, TOL, golden_grads, golden_params, grad_floor, rel_err  # noqa: E402


def _args(**kw):
    a = dict(device="cpu", model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=64, attn_size=8, K=2, add_pos=1,
             history_max=20)
    a.update(kw)
    return SimpleNamespace(**a)


def test_golden_cases_exist_and_fit_the_size_limit():
    assert len(CASES) == 5, CASES
    shapes = set()
    for c in CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", c + ".npz")) <= 512 << 10
        g = load_golden(c)
        n_items, d, A, K, L, B, C, add_pos, seed = (int(x) for x in g["meta"])
        shapes.add((d, A, K, L, B, add_pos, str(g["opt"])))
        valid = (g["hist"] > 0).sum(1)
        assert set(np.unique(g["lengths"]).tolist()) == {1, min(2, L), max(L - 1, 1), L} or B < 4
        # the tie condition the generator asserted: no row with two or more valid positions is left out of a comparison
        if K >= 2:
            assert (g["gap"][valid >= 2] >= 1e-3 * np.abs(g["target_pred"]).max()).all()
            assert (g["gap"][valid == 1] == 0).all()      # one position: K bitwise-equal interests
    assert shapes == {(64, 8, 4, 20, 77, 1, "Adam"), (32, 4, 2, 7, 160, 0, "SGD"), (128, 16, 8, 50, 33, 1, "Adagrad"),
                      (4, 1, 1, 1, 3, 1, "SGD"), (64, 8, 4, 20, 1, 1, "Adam")}
    g = load_golden("comirec_d32_a4_k2_l7_sgd_b160")
    assert ((g["hist"] > 0).sum(1) == 0).sum() == 1 and (~g["keep"]).sum() == 1          # the all-padding row
    g = load_golden("comirec_d64_a8_k4_l20_adam_b77")
    h = g["hist"]
    assert ((h[:, 0] > 0) & (h[:, 1] == 0) & (h[:, 2] > 0)).any()                          # a zero id between two valid ones


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
    P = golden_params(g)
    r = comirec_np.train_grads(P, g["hist"], g["lengths"], g["item_id"])
    assert rel_err(r["interests"], g["interests"]) <= TOL
    multi = (g["hist"] > 0).sum(1) >= 2
    assert np.array_equal(r["sel"][multi], g["sel"][multi])
    # rows with one valid position: K equal interests, any selection gives the reference's prediction and gradients
    assert rel_err(r["pred"], g["pred"]) <= TOL
    assert abs(r["loss"] - float(g["loss"])) <= TOL * max(1.0, abs(float(g["loss"])))
    for k, name in PARAM_KEYS.items():
        if P[k] is None:
            continue
        assert rel_err(r["grads"][k], g["G_" + name], grad_floor(golden_grads(g), k)) <= TOL, (case, k)
    ev = comirec_np.eval_forward(golden_params(g, "P2_"), g["eval_hist"], g["eval_lengths"], g["eval_iid"])
    assert rel_err(ev, g["eval_pred"]) <= TOL


@pytest.mark.parametrize("case", CASES)
def test_single_position_rows_do_not_depend_on_the_selection(case):
    g = load_golden(case)
    K = int(g["meta"][3])
    P = golden_params(g)
    base = comirec_np.train_grads(P, g["hist"], g["lengths"], g["item_id"])
    single = (g["hist"] > 0).sum(1) <= 1
    other = np.where(single, (base["sel"] + 1) % K, base["sel"])
    alt = comirec_np.train_grads(P, g["hist"], g["lengths"], g["item_id"], sel=other)
    assert rel_err(alt["pred"], base["pred"]) <= 1e-12
    for k in PARAM_KEYS:
        if P[k] is not None and k not in ("W2", "b2"):      # (which ROW of W2 receives the round-off-sized share does change)
            assert rel_err(alt["grads"][k], base["grads"][k]) <= 1e-9, (case, k)
    if K >= 2 and single.any():
        # W2 / b2 of such a row: ds = a (e - c) with one position, a = 1 and e = c: exactly nothing
        f = base["fwd"]
        assert np.abs(f["a"][single].sum(-1) - 1.0).max() <= 1e-12 or ((g["hist"] > 0).sum(1) == 0).any()


def _torch_forward(tp, hist, lengths, item_id, sel):
    import torch
    valid = hist > 0
    h = tp["I"][hist]
    x = h
    if tp["Pos"] is not None:
        x = h + tp["Pos"][(lengths[:, None] - torch.arange(hist.shape[1])[None, :]) * valid]
    s = torch.tanh(x @ tp["W1"].T + tp["b1"]) @ tp["W2"].T + tp["b2"]
    s = s.masked_fill(~valid[:, :, None], -np.inf).transpose(1, 2)
    a = torch.softmax(s, dim=-1)                       # per-row maximum: the shift-invariant form of the reference's line
    a = a.masked_fill(torch.isnan(a), 0.0)
    interests = (h[:, None, :, :] * a[:, :, :, None]).sum(-2)
    user = interests[torch.arange(hist.shape[0]), sel]
    return (user[:, None, :] * tp["I"][item_id]).sum(-1)


@pytest.mark.parametrize("B,L,d,A,K,add_pos", [(6, 5, 8, 3, 3, 1), (9, 4, 4, 1, 2, 0), (4, 1, 12, 5, 4, 1)])
def test_backward_agrees_with_autograd_in_float64(B, L, d, A, K, add_pos):
    import torch
    rng = np.random.default_rng(B * 100 + L)
    n_items = 15
    P = {"I": rng.normal(0, 0.5, (n_items, d)), "Pos": rng.normal(0, 0.5, (L + 1, d)) if add_pos else None,
         "W1": rng.normal(0, 0.5, (A, d)), "b1": rng.normal(0, 0.5, A), "W2": rng.normal(0, 0.5, (K, A)), "b2": rng.normal(0, 0.5, K)}
    lengths = rng.integers(1, L + 1, B)
    hist = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        hist[b, :lengths[b]] = rng.integers(1, n_items, lengths[b])
    if L >= 3:
        lengths[0], hist[0, :3] = 3, (4, 0, 5)
    item_id = rng.integers(1, n_items, (B, 4))
    r = comirec_np.train_grads(P, hist, lengths, item_id)
    tp = {k: (None if v is None else torch.tensor(v, dtype=torch.float64, requires_grad=True)) for k, v in P.items()}
    pred = _torch_forward(tp, torch.from_numpy(hist), torch.from_numpy(lengths), torch.from_numpy(item_id), torch.from_numpy(r["sel"]))
    assert rel_err(pred.detach().numpy(), r["pred"]) <= 1e-12
    pos, neg = pred[:, 0], pred[:, 1:]
    w = (neg - neg.max()).softmax(dim=1)
    loss = -(((pos[:, None] - neg).sigmoid() * w).sum(dim=1)).log().mean()
    loss.backward()
    assert abs(loss.item() - r["loss"]) <= 1e-12
    for k in P:
        if P[k] is not None:
            # L = 1 and the bias of W2: exact zeros on one side, float64 round-off on the other
            floor = 0.0 if k == "I" else float(np.abs(r["grads"]["I"]).max())
            assert rel_err(r["grads"][k], tp[k].grad.numpy(), floor) <= 1e-10, k


def test_class_lookup_flags_and_log_args():
    import main
    cls = main.find_class("model", ("ComiRec", ""))
    assert cls.__name__ == "ComiRec" and cls.reader == "SeqReader" and cls.runner == "BaseRunner"
    assert cls.extra_log_args == ["emb_size", "attn_size", "K"]
    # column 0 is the selection's target: the runner must shuffle the candidates as the reference's does
    assert not getattr(cls, "candidate_permutation_equivariant", False)
    assert not hasattr(cls, "hip_train_step") and not hasattr(cls, "full_catalogue_vectors")
    d, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
    assert (d.emb_size, d.attn_size, d.K, d.add_pos, d.history_max, d.num_neg, d.test_all) == (64, 8, 2, 1, 20, 1, 0)
    a, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args(["--attn_size", "4", "--K", "6", "--add_pos", "0"])
    assert (a.attn_size, a.K, a.add_pos) == (4, 6, 0)


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="the reference exists in the build container only")
def test_flags_and_defaults_equal_the_reference():
    code = ("import sys, argparse, json, numpy as np\n"
            "for n, t in (('object', object), ('int', int), ('float', float), ('bool', bool)):\n"
            "    hasattr(np, n) or setattr(np, n, t)\n"
            "sys.path.insert(0, sys.argv[1])\n"
            "from models.sequential.ComiRec import ComiRec as M\n"
            "a, _ = M.parse_model_args(argparse.ArgumentParser()).parse_known_args([])\n"
            "print(json.dumps([sorted(vars(a).items()), M.reader, M.runner, M.extra_log_args]))\n")
    import json
    outs = []
    for src in (REF_SRC, PLUGIN):
        p = subprocess.run([sys.executable, "-c", code, src], check=True, capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=ROOT))
        outs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_match_the_reference(case):
    from models.sequential.ComiRec import ComiRec
    g = load_golden(case)
    n_items, d, A, K, L, B, C, add_pos, seed = (int(x) for x in g["meta"])
    m = ComiRec(_args(emb_size=d, attn_size=A, K=K, add_pos=add_pos, history_max=L), SimpleNamespace(n_users=5, n_items=n_items))
    want = ["W1.bias", "W1.weight", "W2.bias", "W2.weight", "i_embeddings.weight"] + (["p_embeddings.weight"] if add_pos else [])
    assert sorted(m.state_dict().keys()) == sorted(g["state_keys"].tolist()) == want
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == g["P0_" + k.replace(".", "__")].shape, k
    # BaseModel.init_weights: N(0, 0.01) weights and biases
    assert 0.005 < float(m.i_embeddings.weight.std()) < 0.02 and float(m.W1.bias.abs().max()) < 0.1


def test_dataset_kind_is_sequential():
    from models.BaseModel import SequentialModel
    from models.sequential.ComiRec import ComiRec
    from rechorus_amd import pipeline
    assert ComiRec.Dataset is SequentialModel.Dataset
    assert pipeline.dataset_kind(object.__new__(ComiRec.Dataset)) == "sequential"


@pytest.mark.parametrize("flags", [dict(emb_size=6), dict(emb_size=260), dict(K=0), dict(history_max=0), dict(attn_size=65),
                                   dict(K=17), dict(history_max=257)])
def test_envelope_raises_in_init(flags):
    from models.sequential.ComiRec import ComiRec
    with pytest.raises(ValueError, match="envelope"):
        ComiRec(_args(**flags), SimpleNamespace(n_users=5, n_items=6))


def test_check_shape_reports_the_envelope():
    from rechorus_amd import _lib, engine
    lib = _lib.load()
    for shape in ((4, 1, 1, 1), (256, 64, 16, 256), (4, 64, 16, 256), (256, 1, 1, 1), (64, 8, 4, 20), (36, 5, 3, 256)):
        assert lib.rc_comirec_check_shape(*shape) == _lib.RC_OK, shape
        assert lib.rc_comirec_workspace_bytes(*shape, 4099) > 0
        engine.comirec_check_shape(*shape)
    for shape in ((6, 8, 4, 20), (260, 8, 4, 20), (64, 8, 0, 20), (64, 8, 4, 0), (0, 8, 4, 20), (64, 0, 4, 20), (64, 65, 4, 20),
                  (64, 8, 17, 20), (64, 8, 4, 257)):
        assert lib.rc_comirec_check_shape(*shape) == -4, shape      # RC_ERR_UNSUPPORTED
        msg = lib.rc_last_error_string()
        assert b"outside the envelope" in msg and ("emb_size=%d attn_size=%d K=%d history_max=%d" % shape).encode() in msg
        assert lib.rc_comirec_workspace_bytes(*shape, 64) == 0
        with pytest.raises(ValueError, match="envelope"):
            engine.comirec_check_shape(*shape)


def test_entry_points_refuse_bad_calls_without_a_gpu():
    import ctypes as C
    from rechorus_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(256)

    def fwd(d=64, tgt=p, sel=p, user=p, item=p, B=8):
        return lib.rc_comirec_fwd(item, 100, p, 21, p, p, p, p, p, p, tgt, B, 20, d, 8, 4, p, p, sel, user, None)
    assert fwd(d=30) == -4 and b"outside the envelope" in lib.rc_last_error_string()
    assert fwd(item=None) == -1 and b"null pointer" in lib.rc_last_error_string()
    assert fwd(tgt=None) == -1 and b"come together" in lib.rc_last_error_string()
    assert fwd(B=0) == -1 and b"batch" in lib.rc_last_error_string()
    bwd = lambda ws_bytes, g_x=p: lib.rc_comirec_bwd(p, 100, p, 21, p, p, p, p, p, p, p, p, p, 8, 20, 64, 8, 4, p, g_x, p, p, p, p, p,
                                                      ws_bytes, None)
    assert bwd(16) == -2 and b"workspace 16 <" in lib.rc_last_error_string()
    assert bwd(1 << 30, g_x=None) == -1 and b"g_x comes with the position table" in lib.rc_last_error_string()
    assert lib.rc_comirec_score_max(p, p, 100, p, 8, 0, 64, 4, p, None) == -1 and b"candidate count" in lib.rc_last_error_string()
    assert lib.rc_comirec_score_max(p, p, 100, p, 8, 100, 64, 17, p, None) == -4


def test_engine_wrappers_raise_without_touching_the_gpu():
    import torch
    from rechorus_amd import engine, nn as hnn
    z = torch.zeros
    with pytest.raises(ValueError, match="envelope"):
        engine.comirec_fwd(z(9, 6), None, z(8, 6), z(8), z(4, 8), z(4), z(3, 20, dtype=torch.int64), z(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="lengths"):
        engine.comirec_fwd(z(9, 64), None, z(8, 64), z(8), z(4, 8), z(4), z(3, 20, dtype=torch.int64), z(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="candidates"):
        engine.comirec_score_max(z(3, 4, 64), z(9, 64), z(2, 5, dtype=torch.int64))
    w = torch.zeros(8, 64, requires_grad=True)
    with pytest.raises(RuntimeError, match="no backward"):
        hnn.comirec_scores(z(9, 64), None, w, z(8), z(4, 8), z(4), z(3, 20, dtype=torch.int64), z(3, dtype=torch.int64),
                           z(3, 5, dtype=torch.int64))


def test_comirec_kernels_use_no_float_atomics():
    src = open(os.path.join(ROOT, "rechorus_amd", "csrc", "comirec.hip")).read()
    assert not re.search(r"atomic\w*\s*\(|__hip_atomic|__atomic", src)
