"""CPU: DCNv2's host side against the reference's goldens (tests/golden/make_golden_dcnv2.py) -- the goldens themselves (size, the
conditions that make them exercise both tanh stages and the gate), the float64 restatement of both cross networks, the head and the
hand-derived backward of the mixed layer (tests/dcnv2_np.py) against the reference and against central differences, the model file's
class lookup, flags, state_dict keys and initial parameters under the same seed, the refusals at construction and of the entry points,
and the norm term of the loss.  No kernel runs.

Tolerances: the larger of 2e-5 and 4 x the golden's dev/<key> (the reference's own fp32 deviation from float64), as
largest |difference| / largest |reference entry| (dcnv2_np.bound_for); gradients no finer than 1e-6 of the batch's largest gradient
entry; the golden's zero_grad_keys (exactly zero in exact arithmetic) absolutely, at 1e-5 of the largest gradient entry."""
import argparse
import ctypes as C
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

import dcnv2_np as dnp  # noqa: E402
from dcnv2_np import rel_err  # noqa: E402

CASES = [c for c in golden_cases("dcnv2_") if c != "dcnv2_layer_dev"]
MIXED = [c for c in CASES if "_mix_" in c]


def _args(**kw):
    a = dict(device="cpu", model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=4, layers="[8]", cross_layer_num=2,
             reg_weight=2.0, mixed=1, structure="parallel", low_rank=4, expert_num=2, loss_n="BCE")
    a.update(kw)
    return SimpleNamespace(**a)


def _corpus(n_side=0):
    names = ["u_f%d_c" % i for i in range(n_side)]
    fmax = dict({n: 5 for n in names}, user_id=7, item_id=9)
    return SimpleNamespace(n_users=7, n_items=9, user_feature_names=names, item_feature_names=[], situation_feature_names=[],
                           feature_max=fmax)


def test_golden_cases_exist_fit_the_size_limit_and_cover_the_table():
    assert len(CASES) == 6, CASES
    shapes = set()
    for c in CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", c + ".npz")) <= 512 << 10, c
        m = dnp.meta(load_golden(c))
        shapes.add((m["ctr"], m["mixed"], m["stacked"], m["d"], len(m["fields"]), m["r"] if m["mixed"] else 0, m["E"] if m["mixed"] else 0,
                    m["L"], m["B"], m["C"]))
    assert shapes == {(1, 1, 1, 16, 8, 8, 2, 3, 33, 1), (0, 1, 0, 8, 3, 4, 1, 4, 5, 5), (1, 1, 0, 64, 8, 64, 2, 2, 3, 1),
                      (0, 1, 1, 4, 2, 12, 4, 1, 2, 2), (1, 0, 0, 8, 8, 0, 0, 3, 17, 1), (0, 0, 1, 16, 3, 0, 0, 2, 4, 4)}
    assert load_golden(CASES[0])["b1/c_day_f"].dtype == np.int64          # the numeric field of the MIND set


@pytest.mark.parametrize("case", MIXED)
def test_stored_parameters_exercise_both_tanh_stages_and_the_gate(case):
    """the generator's assertions, on the stored data: median |p| and median |q| in [0.3, 2.0] in every (layer, expert); for E >= 2 at
    least half of the rows with a largest gate probability above 0.6 and every expert's mean gate probability above 1 / (4 E)"""
    g = load_golden(case)
    m = dnp.meta(g)
    model, P0 = dnp.scaled_model(g, "cpu")
    f = dnp.model_forward(P0, g, dnp.batch(g, 1))
    xs = [f["x0"]] + f["xs"]
    Wg = np.concatenate([P0["gating.%d.weight" % e] for e in range(m["E"])], 0)
    bg = np.concatenate([P0["gating.%d.bias" % e] for e in range(m["E"])], 0)
    for l in range(m["L"]):
        _, d = dnp.mix_layer_forward(xs[0], xs[l], P0["cross_layer_u.%d" % l], P0["cross_layer_v.%d" % l], P0["cross_layer_c.%d" % l],
                                     P0["bias.%d" % l], Wg, bg, details=True)
        for e in range(m["E"]):
            mp, mq = np.median(np.abs(d["p"][:, e])), np.median(np.abs(d["q"][:, e]))
            assert 0.3 <= mp <= 2.0 and 0.3 <= mq <= 2.0, (case, l, e, mp, mq)
        if m["E"] >= 2:
            assert (d["g"].max(1) > 0.6).mean() >= 0.5, (case, l)
            assert d["g"].mean(0).min() > 1.0 / (4 * m["E"]), (case, l, d["g"].mean(0))


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference(case):
    g = load_golden(case)
    m = dnp.meta(g)
    _, P0 = dnp.scaled_model(g, "cpu")
    f = dnp.model_forward(P0, g, dnp.batch(g, 1), with_grads=True)
    for l in range(m["L"]):
        assert rel_err(f["xs"][l], g["X%d" % l]) <= dnp.bound_for(g, "X%d" % l)[0], (case, l)
    assert rel_err(f["pred"].reshape(g["pred"].shape), g["pred"]) <= dnp.bound_for(g, "pred")[0]
    assert abs(f["loss"] - float(g["loss"])) <= dnp.bound_for(g, "loss")[0] * abs(float(g["loss"]))
    zero, gmax = set(str(k) for k in g["zero_grad_keys"]), dnp.grad_floor(g) * 1e6
    keys = [k for k in g if k.startswith("G/")]
    assert sorted(k[2:] for k in keys) == sorted(f["G"])
    for k in keys:
        want, got = dnp.stored(g, "", k, f["G"][k[2:]])
        if k[2:] in zero:
            assert np.abs(got).max() <= 1e-5 * gmax and np.abs(want).max() <= 1e-5 * gmax, (case, k)
            continue
        assert rel_err(got, want, dnp.grad_floor(g)) <= dnp.bound_for(g, k)[0], (case, k)


@pytest.mark.parametrize("N,D,r,E,zero_row", [(3, 8, 4, 1, None), (4, 12, 8, 2, 1), (2, 8, 12, 4, None), (5, 24, 4, 3, 0)])
def test_closed_form_backward_agrees_with_central_differences(N, D, r, E, zero_row):
    prob = [np.asarray(a, np.float64) for a in dnp.random_layer(N, D, r, E, seed=10 * N + E, zero_row=zero_row)]
    dXn, args = prob[8], prob[:8]
    got = dnp.mix_layer_backward(dXn, *args)
    order = ("dX0", "dXl", "dU", "dV", "dC", "dbias", "dWg", "dbg")
    h = 1e-6
    rng = np.random.default_rng(0)
    for idx, name in enumerate(order):
        a = args[idx]
        flat = a.reshape(-1)
        picks = rng.choice(flat.size, size=min(flat.size, 12), replace=False)
        if zero_row is not None and idx < 2:
            picks = np.concatenate([picks, [zero_row * D, zero_row * D + D - 1]])      # elements of the row of zeros
        for i in picks:
            keep = flat[i]
            flat[i] = keep + h
            up = (dnp.mix_layer_forward(*args) * dXn).sum()
            flat[i] = keep - h
            dn = (dnp.mix_layer_forward(*args) * dXn).sum()
            flat[i] = keep
            num = (up - dn) / (2 * h)
            assert abs(num - got[name].reshape(-1)[i]) <= 1e-6 * max(1.0, np.abs(got[name]).max()), (name, i, num, got[name].reshape(-1)[i])
    if E == 1:      # the softmax over one expert is identically 1: the gate's gradient is an exact zero
        assert (got["dWg"] == 0).all() and (got["dbg"] == 0).all()
    if zero_row is not None:      # x_0 = 0 switches the row's cross term off: only the straight-through term reaches x_l
        assert (got["dXl"][zero_row] == dXn[zero_row]).all()


def test_class_lookup_flags_and_log_args():
    import main
    ctr, topk = main.find_class("model", ("DCNv2", "CTR")), main.find_class("model", ("DCNv2", "TopK"))
    assert (ctr.__name__, ctr.reader, ctr.runner) == ("DCNv2CTR", "ContextReader", "CTRRunner")
    assert (topk.__name__, topk.reader, topk.runner) == ("DCNv2TopK", "ContextReader", "BaseRunner")
    assert ctr.__module__ == topk.__module__ == "models.dcnv2_model"
    for cls, loss_n in ((ctr, "BCE"), (topk, "BPR")):
        assert cls.extra_log_args == ["emb_size", "loss_n", "cross_layer_num"]
        a, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
        assert (a.emb_size, a.layers, a.cross_layer_num, a.reg_weight) == (64, "[64]", 6, 2.0)
        assert (a.mixed, a.structure, a.low_rank, a.expert_num, a.loss_n) == (1, "parallel", 64, 2, loss_n)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_and_initial_parameters_match_the_reference(case):
    g = load_golden(case)
    model = dnp.build_model(g)
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in g["state_keys"]]
    m = dnp.meta(g)
    assert tuple(sd["bias.0"].shape) == (m["d"] * len(m["fields"]), 1)
    for k, v in sd.items():
        if "I0/" + k in g:
            assert v.numpy().tobytes() == g["I0/" + k].tobytes(), (case, k)
        else:
            assert hashlib.sha256(v.numpy().tobytes()).hexdigest() == str(g["I0sha/" + k]), (case, k)
    expect = {"context_embedding.user_id.weight", "bias.0", "deep_layers.mlp.0.weight", "predict_layer.weight"}
    expect |= ({"cross_layer_u.0", "cross_layer_v.0", "cross_layer_c.0", "gating.0.weight", "gating.0.bias"} if m["mixed"]
               else {"cross_layer_w2.0"})
    assert expect <= set(sd)
    assert ("cross_layer_w2.0" in sd) != ("cross_layer_u.0" in sd)


@pytest.mark.parametrize("kw,text", [
    (dict(emb_size=3), "width=6"), (dict(emb_size=514), "width=1028"), (dict(low_rank=2), "low_rank=2"),
    (dict(low_rank=132), "low_rank=132"), (dict(low_rank=6), "low_rank=6"), (dict(expert_num=0), "expert_num=0"),
    (dict(expert_num=5), "expert_num=5"), (dict(structure="foo"), "structure")])
def test_construction_refuses_what_the_kernels_do_not_cover(kw, text):
    from models.context.DCNv2 import DCNv2CTR, DCNv2TopK
    for cls in (DCNv2CTR, DCNv2TopK):
        with pytest.raises(ValueError, match=text):
            cls(_args(**kw), _corpus())
    if "structure" not in kw:      # the envelope is the mixed kernels': the plain network is not held to it
        DCNv2CTR(_args(mixed=0, **kw), _corpus())


def test_envelope_edges_construct_and_a_cpu_forward_raises():
    import torch
    from models.context.DCNv2 import DCNv2TopK
    for kw in (dict(emb_size=4), dict(emb_size=512, low_rank=128, expert_num=4, cross_layer_num=1), dict(low_rank=4, expert_num=1)):
        DCNv2TopK(_args(loss_n="BPR", **kw), _corpus())
    model = DCNv2TopK(_args(loss_n="BPR"), _corpus())
    with pytest.raises(RuntimeError, match="GPU only"):
        model({"user_id": torch.zeros(2, dtype=torch.int64), "item_id": torch.zeros(2, 2, dtype=torch.int64)})


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from rechorus_amd import _lib, engine
    lib = _lib.load()
    p, q = C.c_void_p(256), C.c_void_p(260)      # non-null; never dereferenced; q is not 16-byte aligned
    N, D, r, E = 10, 24, 8, 2
    assert lib.rc_dcnv2_check_shape(D, r, E) == 0 and lib.rc_dcnv2_check_shape(8, 4, 1) == 0 and lib.rc_dcnv2_check_shape(1024, 128, 4) == 0
    for bad in ((6, 8, 2), (1028, 8, 2), (4, 8, 2), (24, 2, 2), (24, 132, 2), (24, 6, 2), (24, 8, 0), (24, 8, 5)):
        assert lib.rc_dcnv2_check_shape(*bad) == -4, bad
        assert lib.rc_last_error_string().startswith(b"rc_dcnv2_check_shape: outside the envelope")
        with pytest.raises(ValueError, match="DCNv2 on the HIP engine"):
            engine.dcnv2_check_shape(*bad)

    def fwd(x0=p, bias=p, out=p, n=N, d=D, e=E):
        return lib.rc_dcnv2_mix_layer_fwd(x0, p, p, p, p, bias, p, p, n, d, r, e, out, None)

    def bwd(dxn=p, ws=p, nbytes=0, dx0=p, dbg=p, n=N, rr=r):
        return lib.rc_dcnv2_mix_layer_bwd(dxn, p, p, p, p, p, p, p, p, n, D, rr, E, ws, nbytes, p, dx0, p, p, p, p, p, dbg, None)
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    table = [(lambda: fwd(x0=None), INVALID, b"null pointer"), (lambda: fwd(bias=None), INVALID, b"null pointer"),
             (lambda: fwd(out=None), INVALID, b"null pointer"), (lambda: fwd(out=q), INVALID, b"16-byte aligned"),
             (lambda: fwd(n=0), UNSUPPORTED, b"rows"), (lambda: fwd(d=6), UNSUPPORTED, b"envelope"), (lambda: fwd(e=5), UNSUPPORTED, b"envelope"),
             (lambda: bwd(dxn=None), INVALID, b"null pointer"), (lambda: bwd(dbg=None), INVALID, b"null pointer"),
             (lambda: bwd(dx0=q), INVALID, b"16-byte aligned"), (lambda: bwd(ws=None), INVALID, b"workspace must be"),
             (lambda: bwd(ws=q), INVALID, b"workspace must be"), (lambda: bwd(n=-1), UNSUPPORTED, b"rows"),
             (lambda: bwd(rr=6), UNSUPPORTED, b"envelope"),
             # everything that inspects only the arguments comes before the workspace-size check: ws_bytes = 0 here
             (bwd, WORKSPACE, b"workspace of 0 bytes")]
    for i, (call, code, text) in enumerate(table):
        got = call()
        msg = lib.rc_last_error_string()
        assert got == code, (i, got, msg)
        assert msg.startswith(b"rc_dcnv2_mix_layer_") and text in msg, (i, msg)


def test_backward_workspace_saturates():
    """the number of partials is bounded independently of N: the size stops growing once N passes 256 row tiles"""
    from rechorus_amd import _lib
    ws = _lib.load().rc_dcnv2_mix_layer_bwd_workspace_bytes
    per = lambda D, r, E: (E * (2 * D * r + r * r) + D + E * D + E + 63) // 64 * 256
    assert ws(1, 512, 64, 2) == per(512, 64, 2) and ws(33, 512, 64, 2) == 3 * per(512, 64, 2)
    big = [ws(n, 512, 64, 2) for n in (1 << 14, 1 << 17, 1 << 20, 1 << 24)]
    assert len(set(big)) == 1 and big[0] == min(256, (128 << 20) // per(512, 64, 2)) * per(512, 64, 2)
    assert ws(1 << 20, 1024, 128, 4) == ((128 << 20) // per(1024, 128, 4)) * per(1024, 128, 4) <= 128 << 20
    assert ws(0, 512, 64, 2) == 0 and ws(10, 6, 64, 2) == 0


def test_the_plain_network_adds_the_norm_term_and_the_mixed_one_does_not(monkeypatch):
    import torch
    from models.BaseContextModel import ContextCTRModel
    from models.context.DCNv2 import DCNv2CTR
    monkeypatch.setattr(ContextCTRModel, "loss", lambda self, out: out["prediction"].sum() * 0 + 0.25)
    torch.manual_seed(0)
    plain = DCNv2CTR(_args(mixed=0, reg_weight=0.5), _corpus())
    want = 0.25 + 0.5 * sum(float(W.detach().double().norm(2)) for W in plain.cross_layer_w2)      # the norm, not its square
    out = {"prediction": torch.zeros(3)}
    assert abs(float(plain.loss(out)) - want) <= 1e-5 * want
    assert abs(want - 0.25) > 1.0
    mixed = DCNv2CTR(_args(mixed=1, reg_weight=0.5), _corpus())
    assert float(mixed.loss(out)) == 0.25
