"""CPU: AutoInt's host side against the reference's goldens (tests/golden/make_golden_autoint.py) -- the goldens themselves (size,
the two conditions that make them exercise the attention path, a bit-identical rerun of the generator), the float64 restatement of
the layer and its hand-derived backward (tests/autoint_np.py) against the reference and against torch autograd, the model file's
class lookup, flags, state_dict keys, initial parameters under the same seed, its torch path on the CPU (prediction, loss,
gradients, both optimizer trajectories), the shape envelope and the device pipeline's dataset kind.  No kernel runs.

Tolerances: the goldens are float32 results of the reference; the restatement is float64 and the model file's CPU path float32 torch
ops in another order: 2e-5 of the tensor's largest entry.  Where a golden stores the reference's own fp32-vs-float64 deviation for a
tensor and it exceeds 1e-5, the bound is twice that deviation (autoint_np.bound_for).  Gradients that are exactly zero in exact
arithmetic are compared no finer than 1e-6 of the batch's largest gradient entry (autoint_np.grad_floor)."""
import argparse
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT, assert_update_close, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden import REF_SRC  # noqa: E402   (where the generator imports the reference from)

import autoint_np as anp  # noqa: E402
from autoint_np import TOL, rel_err  # noqa: E402

CASES = golden_cases("autoint_")
GEN = os.path.join(ROOT, "tests", "golden", "make_golden_autoint.py")
ATTENTION_PATH = ("autoint_attentions.", "residual_embeddings.", "deep_layers.")


def _args(**kw):
    a = dict(device="cpu", model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=64, attention_size=32, num_heads=1,
             num_layers=1, layers="[64]", loss_n="BCE")
    a.update(kw)
    return SimpleNamespace(**a)


def _corpus(n_side=6):
    names = ["u_f%d_c" % i for i in range(n_side)]
    fmax = dict({n: 5 for n in names}, user_id=7, item_id=9)
    return SimpleNamespace(n_users=7, n_items=9, user_feature_names=names, item_feature_names=[], situation_feature_names=[],
                           feature_max=fmax)


def test_golden_cases_exist_fit_the_size_limit_and_exercise_the_attention_path():
    assert len(CASES) == 5, CASES
    shapes = set()
    for c in CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", c + ".npz")) <= 512 << 10, c
        g = load_golden(c)
        m = anp.meta(g)
        F = len(m["fields"])
        shapes.add((m["ctr"], m["d"], m["A"], m["H"], m["L"], tuple(m["tower"]), m["B"], m["C"], F))
        for l in range(m["L"]):
            # in every layer at least half of the softmax rows are clearly non-uniform ...
            assert g["pmax%d" % l].shape == (m["B"], m["C"], m["H"], F)
            assert (g["pmax%d" % l] > anp.row_threshold(F)).mean() >= 0.5, (c, l)
            assert g["Y%d" % l].shape == (m["B"], m["C"], F, m["A"])
        # ... and between a quarter and three quarters of the last layer's outputs are positive
        assert 0.25 <= (g["Y%d" % (m["L"] - 1)] > 0).mean() <= 0.75, c
    assert shapes == {(True, 64, 32, 1, 1, (64,), 48, 1, 8), (True, 64, 32, 2, 2, (64, 32), 33, 1, 9),
                      (False, 16, 8, 4, 3, (32,), 24, 5, 7), (True, 128, 64, 8, 1, (), 3, 1, 3), (False, 8, 4, 4, 1, (), 1, 2, 2)}
    g = load_golden("autoint_mind_ctr_d64_a32_h1_l1")
    assert g["b1/c_day_f"].dtype == np.int64 and "Adam/overall_bias" in g and "SGD/overall_bias" in g
    g = load_golden("autoint_mindf_ctr_d64_a32_h2_l2")
    assert g["b1/c_day_f"].dtype == np.float64 and g["b1/i_age_f"].shape == (33, 1)
    assert "Adagrad/overall_bias" in load_golden("autoint_ctr_d128_a64_h8_l1_b3")


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="the reference exists in the build container only")
def test_generator_reruns_bit_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, GEN, "--out", str(tmp_path)], check=True, env=env, capture_output=True, timeout=900)
    for c in CASES:
        a, b = load_golden(c), np.load(os.path.join(str(tmp_path), c + ".npz"))
        assert sorted(a) == sorted(b.files)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (c, k)


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference(case):
    g = load_golden(case)
    m = anp.meta(g)
    P = anp.scaled_params(g)
    f = anp.model_forward(P, g, anp.batch(g, 1))
    for l in range(m["L"]):
        assert rel_err(f["Ys"][l], g["Y%d" % l]) <= TOL, (case, l)
    pred = 1.0 / (1.0 + np.exp(-f["raw"])) if m["ctr"] else f["raw"]
    assert rel_err(pred.reshape(g["pred"].shape), g["pred"]) <= anp.bound_for(g, "pred")[0]
    G = anp.attention_grads(P, g, anp.batch(g, 1), anp.graw_from_gpred(g))
    checked = 0
    for k in anp.state_keys(g):
        if k.startswith(ATTENTION_PATH):
            assert rel_err(G[k], g["G/" + k], anp.grad_floor(g)) <= anp.bound_for(g, k)[0], (case, k)
            checked += 1
    assert checked == 5 * m["L"] + 2 * (len(m["tower"]) + 1)


def _torch_layer(X, Wq, Wk, Wv, Wr, br, H):
    import torch
    N, F, _ = X.shape
    A = Wq.shape[0]
    split = lambda t: t.view(N, F, H, A // H).transpose(1, 2)
    q, k, v = split(X @ Wq.T), split(X @ Wk.T), split(X @ Wv.T)
    p = (q @ k.transpose(-2, -1) / (A // H) ** 0.5).softmax(dim=-1)
    return ((p @ v).transpose(1, 2).reshape(N, F, A) + X @ Wr.T + br).relu()


@pytest.mark.parametrize("N,F,Din,A,H", [(3, 2, 4, 4, 4), (5, 7, 8, 8, 1), (2, 9, 12, 6, 3), (4, 3, 16, 8, 2)])
def test_backward_agrees_with_autograd_in_float64(N, F, Din, A, H):
    import torch
    prob = anp.random_layer(N, F, Din, A, H, seed=N * 100 + F)
    X, Wq, Wk, Wv, Wr, br, dY = (np.asarray(a, dtype=np.float64) for a in prob)
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (X, Wq, Wk, Wv, Wr, br)]
    Y = _torch_layer(*t, H)
    assert rel_err(anp.layer_forward(X, Wq, Wk, Wv, Wr, br, H), Y.detach().numpy()) <= 1e-12
    Y.backward(torch.from_numpy(dY))
    r = anp.layer_backward(X, Wq, Wk, Wv, Wr, br, H, dY)
    for name, tt in zip(("dX", "dWq", "dWk", "dWv", "dWr", "dbr"), t):
        assert rel_err(r[name], tt.grad.numpy()) <= 1e-10, name


def test_class_lookup_flags_and_log_args():
    import main
    ctr, topk = main.find_class("model", ("AutoInt", "CTR")), main.find_class("model", ("AutoInt", "TopK"))
    assert (ctr.__name__, ctr.reader, ctr.runner) == ("AutoIntCTR", "ContextReader", "CTRRunner")
    assert (topk.__name__, topk.reader, topk.runner) == ("AutoIntTopK", "ContextReader", "BaseRunner")
    assert ctr.__module__ == topk.__module__ == "models.autoint_model"
    for cls in (ctr, topk):
        assert cls.extra_log_args == ["emb_size", "layers", "num_layers", "num_heads", "loss_n"]
        a, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
        assert (a.emb_size, a.attention_size, a.num_heads, a.num_layers, a.layers) == (64, 32, 1, 1, "[64]")
    assert ctr.parse_model_args(argparse.ArgumentParser()).parse_known_args([])[0].loss_n == "BCE"
    assert topk.parse_model_args(argparse.ArgumentParser()).parse_known_args([])[0].loss_n == "BPR"
    a, _ = ctr.parse_model_args(argparse.ArgumentParser()).parse_known_args(["--attention_size", "16", "--num_heads", "4", "--num_layers", "3"])
    assert (a.attention_size, a.num_heads, a.num_layers) == (16, 4, 3)


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="the reference exists in the build container only")
def test_flags_and_defaults_equal_the_reference():
    code = ("import sys, argparse, json, numpy as np\n"
            "for n, t in (('object', object), ('int', int), ('float', float), ('bool', bool)):\n"
            "    hasattr(np, n) or setattr(np, n, t)\n"
            "sys.path.insert(0, sys.argv[1])\n"
            "from models.context.AutoInt import AutoIntCTR, AutoIntTopK\n"
            "out = []\n"
            "for M in (AutoIntCTR, AutoIntTopK):\n"
            "    a, _ = M.parse_model_args(argparse.ArgumentParser()).parse_known_args([])\n"
            "    out.append([sorted(vars(a).items()), M.reader, M.runner, M.extra_log_args])\n"
            "print(json.dumps(out))\n")
    import json
    outs = []
    for src in (REF_SRC, PLUGIN):
        p = subprocess.run([sys.executable, "-c", code, src], check=True, capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=ROOT))
        outs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]


@pytest.mark.parametrize("case", CASES)
def test_state_dict_and_initial_parameters_equal_the_golden(case):
    import torch
    g = load_golden(case)
    m = anp.meta(g)
    torch.manual_seed(m["seed"])
    model = anp.build_model(g, "cpu", params={})       # nothing loaded: what the constructor leaves under the golden's seed
    sd = model.state_dict()
    assert list(sd.keys()) == anp.state_keys(g)
    for l in range(m["L"]):
        assert "autoint_attentions.%d.q_linear.weight" % l in sd and "residual_embeddings.%d.bias" % l in sd
        assert "autoint_attentions.%d.q_linear.bias" % l not in sd
    I0 = anp.initial_params(g)
    for k, v in sd.items():
        assert tuple(v.shape) == I0[k].shape == g["G/" + k].shape, k
        assert v.numpy().tobytes() == I0[k].tobytes(), (case, k)      # bit-equal: same modules, same creation order, one init pass
        if "I0sha/" + k in g:      # the case that stores the SHA-256 of the reference's tensors instead of the tensors
            import hashlib
            assert hashlib.sha256(v.numpy().tobytes()).hexdigest() == str(g["I0sha/" + k]), (case, k)


def test_stored_initial_parameters_equal_the_seeded_restatement():
    """one golden leaves I0 out for size and autoint_np.init_from_seed regenerates it; where I0 is stored the two must agree"""
    stored = 0
    for case in CASES:
        g = load_golden(case)
        if "I0/overall_bias" in g:
            stored += 1
            for k, v in anp.init_from_seed(g).items():
                assert v.tobytes() == g["I0/" + k].tobytes(), (case, k)
    assert stored == 4


@pytest.mark.parametrize("case", CASES)
def test_model_file_on_the_cpu_reproduces_the_reference(case):
    import torch
    g = load_golden(case)
    m = anp.meta(g)
    model = anp.build_model(g, "cpu")
    model.train()
    fd = anp.feed(g, 1, "cpu")
    with torch.no_grad():
        X, _ = model._get_embeddings_FM(fd)
        for l, Y in enumerate(model.interacting_layers(X)):
            assert rel_err(Y.numpy(), g["Y%d" % l]) <= TOL, (case, l)
    out = model(fd)
    loss = anp.torch_loss(g, out)
    loss.backward()
    assert rel_err(out["prediction"].detach().numpy().reshape(g["pred"].shape), g["pred"]) <= anp.bound_for(g, "pred")[0]
    assert abs(loss.item() - float(g["loss"])) <= TOL * max(1.0, abs(float(g["loss"])))
    for k, p in model.named_parameters():
        assert rel_err(p.grad.numpy(), g["G/" + k], anp.grad_floor(g)) <= anp.bound_for(g, k)[0], (case, k)

    P0 = anp.scaled_params(g)
    for opt in ("Adam", "SGD", "Adagrad"):
        if opt + "_hyper" not in g:
            continue
        lr, l2 = (float(x) for x in g[opt + "_hyper"])
        m2 = anp.build_model(g, "cpu")
        m2.train()
        optim = getattr(torch.optim, opt)(m2.customize_parameters(), lr=lr, weight_decay=l2)      # helpers/BaseRunner.py:96-101
        for step in (1, 2):
            optim.zero_grad()
            ls = anp.torch_loss(g, m2(anp.feed(g, step, "cpu")))
            ls.backward()
            optim.step()
            want = float(g[opt + "_losses"][step - 1])
            assert abs(ls.item() - want) <= TOL * max(1.0, abs(want)), (case, opt, step)
        extra = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
        for k, v in m2.state_dict().items():
            assert_update_close(v.numpy(), P0[k], g["%s/%s" % (opt, k)], what=f"{case} {opt} {k}", extra_atol=2 * extra,
                                outlier_atol=2 * lr)


@pytest.mark.parametrize("flags,n_side", [(dict(attention_size=2), 6), (dict(attention_size=68), 6), (dict(num_heads=3), 6),
                                          (dict(emb_size=132), 6), (dict(emb_size=6), 6), (dict(), 31), (dict(num_heads=0), 6)])
def test_envelope_raises_in_init(flags, n_side):
    from models.context.AutoInt import AutoIntCTR, AutoIntTopK
    for cls in (AutoIntCTR, AutoIntTopK):
        with pytest.raises(ValueError, match="envelope"):
            cls(_args(**flags), _corpus(n_side))
    AutoIntCTR(_args(attention_size=64, num_heads=64, emb_size=128, num_layers=2), _corpus(30))      # the far corner is inside


def test_check_shape_and_entry_points_refuse_bad_calls_without_a_gpu():
    import ctypes as C
    from rechorus_amd import _lib, engine
    lib = _lib.load()
    for shape in ((2, 4, 4, 4), (32, 128, 64, 64), (8, 64, 32, 1), (9, 36, 6, 3), (32, 128, 64, 1), (2, 128, 64, 8)):
        assert lib.rc_autoint_check_shape(*shape) == _lib.RC_OK, shape
        assert lib.rc_autoint_workspace_bytes(4099, *shape) > 0
    for shape in ((1, 64, 32, 1), (33, 64, 32, 1), (8, 62, 32, 1), (8, 132, 32, 1), (8, 64, 2, 1), (8, 64, 68, 1), (8, 64, 32, 3),
                  (8, 64, 32, 0)):
        assert lib.rc_autoint_check_shape(*shape) == -4, shape      # RC_ERR_UNSUPPORTED
        assert b"outside the envelope" in lib.rc_last_error_string()
        assert lib.rc_autoint_workspace_bytes(64, *shape) == 0
        with pytest.raises(ValueError, match="envelope"):
            engine.autoint_check_shape(*shape)
    p = C.c_void_p(256)      # non-null and aligned; never dereferenced: every call below is refused before any launch
    q = C.c_void_p(260)

    def fwd(X=p, N=10, F=8, br=p, Y=p):
        return lib.rc_autoint_layer_fwd(X, p, p, p, p, br, N, F, 64, 32, 1, Y, None)

    def bwd(ws=p, ws_bytes=1 << 30, dY=p, N=10, H=1, dX=p):
        return lib.rc_autoint_layer_bwd(p, p, p, p, p, p, dY, N, 8, 64, 32, H, ws, ws_bytes, dX, p, p, p, p, p, None)
    table = [(lambda: fwd(X=None), -1, b"null pointer"), (lambda: fwd(br=None), -1, b"null pointer"), (lambda: fwd(Y=q), -1, b"16-byte"),
             (lambda: fwd(N=0), -4, b"instances"), (lambda: fwd(F=40), -4, b"outside the envelope"),
             (lambda: bwd(dY=None), -1, b"null pointer"), (lambda: bwd(ws=None), -1, b"workspace"), (lambda: bwd(ws_bytes=16), -2, b"workspace of 16"),
             (lambda: bwd(H=5), -4, b"outside the envelope"), (lambda: bwd(dX=q), -1, b"16-byte"), (lambda: bwd(N=1 << 25), -4, b"instances")]
    for i, (call, code, text) in enumerate(table):
        got = call()
        msg = lib.rc_last_error_string()
        assert got == code and text in msg and msg.startswith(b"rc_autoint_layer_"), (i, got, msg)


def test_engine_and_autograd_wrappers_raise_without_touching_the_gpu():
    import torch
    from rechorus_amd import engine, nn as hnn
    z = torch.zeros
    with pytest.raises(ValueError, match="envelope"):
        engine.autoint_layer_fwd(z(3, 40, 64), z(32, 64), z(32, 64), z(32, 64), z(32, 64), z(32), 1)
    with pytest.raises(ValueError, match="Wk must be"):
        engine.autoint_layer_fwd(z(3, 8, 64), z(32, 64), z(16, 64), z(32, 64), z(32, 64), z(32), 1)
    w = torch.zeros(32, 64, requires_grad=True)
    with pytest.raises(RuntimeError, match="no backward"):
        hnn.autoint_layer_eval(z(3, 8, 64), w, z(32, 64), z(32, 64), z(32, 64), z(32), 1)


def test_dataset_kinds():
    from models.context.AutoInt import AutoIntCTR, AutoIntTopK
    from rechorus_amd import pipeline
    assert pipeline.dataset_kind(object.__new__(AutoIntCTR.Dataset)) == "ctr"
    assert pipeline.dataset_kind(object.__new__(AutoIntTopK.Dataset)) == "context"


def test_autoint_kernels_use_no_float_atomics():
    import re
    src = open(os.path.join(ROOT, "rechorus_amd", "csrc", "autoint.hip")).read()
    assert not re.search(r"atomic\w*\s*\(|__hip_atomic|__atomic", src)
