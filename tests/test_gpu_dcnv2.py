"""GPU: DCNv2 on the HIP engine (rc_dcnv2_mix_layer_fwd / _bwd) against the reference's goldens
(tests/golden/make_golden_dcnv2.py) and the float64 restatement (tests/dcnv2_np.py): the layer node on the edge grid of row counts
and shapes with dX0_part and dXl checked separately, weight gradients over several workgroups and over more tiles than workgroups,
bit-identical reruns, the evaluation form, exact-zero gate gradients with one expert; all six model cases on init, every layer's
x_l, prediction, loss, every gradient and two optimizer steps; a demo-shape stack against float64 torch on the device; the four
demo flag sets through the CLI.

Tolerances: the project's rule, nothing new -- each comparison is held to the larger of 2e-5 and 4 x the golden's stored dev/<key>
(the reference's own fp32 deviation from float64, dcnv2_np.bound_for), as largest |difference| / largest |reference entry|;
the random layer problems (dcnv2_np.LAYER_PROBLEMS, the demo-shape stack) are regenerated from their seeds and have their deviations
STORED in tests/golden/dcnv2_layer_dev.npz by the same generator (the reference's expression in fp32 torch ops against float64); no
bound is computed at test time.  The largest stored figures are gate bias gradients (1.6e-4 at N = 65, D = 24, E = 2): their
entries sum to zero and nearly cancel over the rows, for the reference as for the kernels; every other tensor's is below 2e-6.  The optimizer-step comparison passes
outlier_atol = 2 lr under Adam / Adagrad as tests/test_gpu_autoint.py does for two compounded steps: an element whose gradient is
round-off (|g| ~ eps) takes a step of up to lr per step in a direction the round-off decides, in the reference as well.  Gradients are compared no finer than 1e-6 of the batch's
largest gradient entry; the golden's zero_grad_keys (exactly zero in exact arithmetic: the bias in front of BatchNorm1d, the output
bias under BPR) are bounded absolutely at 1e-5 of the largest gradient entry, and under Adam / Adagrad their steps by 2.5 lr.  Each
comparison prints its bound and the largest error it saw (DCNV2_TOL lines, run with -s; tools/dcnv2_tolerance_report.py folds that
output into profiles/dcnv2_tolerances.txt)."""
import argparse
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_update_close, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)
import dcnv2_np as dnp  # noqa: E402
from dcnv2_np import GRAD_NAMES, TOL, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [c for c in golden_cases("dcnv2_") if c != "dcnv2_layer_dev"]
DEVS = load_golden("dcnv2_layer_dev")      # the stored fp32 deviations of the random layer problems (make_golden_dcnv2.py)


def _check(got, want, what, bound=TOL, why="the cap", floor=0.0):
    if torch.is_tensor(got):
        got = got.detach().cpu().numpy()
    err = rel_err(np.asarray(got).reshape(np.shape(want)), want, floor)
    print(f"DCNV2_TOL {what}: {err:.3e} (allowed {bound:.3g}: {why})")
    assert err <= bound, f"{what}: largest error / largest entry {err:.3e} > {bound:g}"
    return err


def _run_layer(prob, cuda, workspace=None):
    from rechorus_amd import engine
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in prob]
    Xn = engine.dcnv2_mix_layer_fwd(*t[:8])
    grads = engine.dcnv2_mix_layer_bwd(t[8], *t[:8], workspace=workspace)
    return t, Xn, grads


def _check_layer(prob_id, cuda, workspace=None):
    """prob_id: an entry of dnp.LAYER_PROBLEMS; its data from the seed, its bounds from the stored deviations"""
    N, D, r, E, seed, zero_row = prob_id
    key, what = dnp.layer_key(*prob_id), f"N={N} D={D} r={r} E={E}"
    prob = dnp.random_layer(N, D, r, E, seed=seed, zero_row=zero_row)
    _, Xn, grads = _run_layer(prob, cuda, workspace)
    fwd, want = dnp.mix_layer_forward(*prob[:8]), dnp.mix_layer_backward(prob[8], *prob[:8])
    _check(Xn, fwd, what + " Xnext", *dnp.stored_bound(DEVS, key + "/Xnext"))
    for name, got in zip(GRAD_NAMES, grads):      # dXl and dX0_part are two of the eight, each against its own reference
        _check(got, want[name], f"{what} {name}", *dnp.stored_bound(DEVS, f"{key}/{name}"))
    return grads


# ---- the layer node against float64 -------------------------------------------------------------------------------------------------
def _problems(pick):
    found = [p for p in dnp.LAYER_PROBLEMS if pick(p)]
    assert found
    return found


@pytest.mark.parametrize("D,r,E", dnp.EDGE_SHAPES)
def test_layer_kernels_on_the_edge_grid(D, r, E, cuda):
    from rechorus_amd import engine
    ws = engine.DCNv2Workspace()
    probs = _problems(lambda p: p[1:4] == (D, r, E) and p[0] in dnp.EDGE_ROWS)
    assert [p[0] for p in probs] == list(dnp.EDGE_ROWS)      # 257 rows: 17 workgroups' partials in the weight gradients; 63: a row of zeros
    for p in probs:
        grads = _check_layer(p, cuda, ws)
        if E == 1:      # the softmax over one expert is identically 1
            assert (grads[6] == 0).all() and (grads[7] == 0).all()


def test_layer_kernels_at_the_envelope_ceiling(cuda):
    _check_layer(_problems(lambda p: p[:4] == (70, 1024, 128, 4))[0], cuda)


@pytest.mark.parametrize("N,D,r,E", [(4200, 36, 4, 2), (8200, 64, 16, 2), (16400, 20, 8, 1)])
def test_more_tiles_than_workgroups_at_every_tile_height(N, D, r, E, cuda):
    """16, 32 and 64 rows a tile (the height grows once the batch fills 256 workgroups): 263, 257 and 257 tiles on 256 workgroups, so
    some workgroups add a second tile to their weight-gradient partial"""
    _check_layer(_problems(lambda p: p[:4] == (N, D, r, E))[0], cuda)


def test_reruns_are_bit_identical_inputs_stay_unchanged_and_eval_equals_training(cuda):
    from rechorus_amd import nn as hnn
    for shape in ((4200, 36, 4, 2), (257, 512, 64, 2), (65, 132, 36, 3)):
        prob = dnp.random_layer(*shape, seed=11)
        runs = []
        for _ in range(2):
            t, Xn, grads = _run_layer(prob, cuda)
            runs.append([x.cpu().numpy().copy() for x in (Xn,) + tuple(grads)])
            for a, b in zip(t, prob):
                assert a.cpu().numpy().tobytes() == b.tobytes(), shape
        for a, b in zip(*runs):
            assert a.tobytes() == b.tobytes(), shape
        t = [x.clone().requires_grad_(True) for x in t[:8]]
        train = hnn.dcnv2_mix_layer(*t)
        with pytest.raises(RuntimeError, match="no backward"):
            hnn.dcnv2_mix_layer_eval(*t)
        with torch.no_grad():
            ev = hnn.dcnv2_mix_layer_eval(*t)
        assert train.requires_grad and not ev.requires_grad
        assert ev.cpu().numpy().tobytes() == train.detach().cpu().numpy().tobytes() == runs[0][0].tobytes(), shape


def test_demo_shape_stack_against_float64_torch_on_the_device(cuda):
    from rechorus_amd import engine, nn as hnn
    N, D, r, E, L = (dnp.STACK[k] for k in ("N", "D", "r", "E", "L"))
    data, dY = dnp.stack_problem()
    leaves = [torch.from_numpy(a).to(cuda).requires_grad_(True) for a in data]
    dY = torch.from_numpy(dY).to(cuda)
    x0, Wg, bg = leaves[:3]
    ws, xl = engine.DCNv2Workspace(), x0
    for l in range(L):
        xl = hnn.dcnv2_mix_layer(x0, xl, *leaves[3 + 4 * l: 7 + 4 * l], Wg, bg, ws)
    xl.backward(dY)
    got = [xl.detach()] + [t.grad for t in leaves]
    want = dnp.torch_stack([t.detach().double().requires_grad_(True) for t in leaves], L, dY)
    for name, a, b in zip(dnp.STACK_NAMES, got, want):
        _check(a, b.cpu().numpy(), f"demo stack N={N} D={D} r={r} E={E} L={L} {name}", *dnp.stored_bound(DEVS, "stack/" + name))


# ---- the model file against the reference's goldens ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_model_matches_the_reference_golden(case, cuda):
    g = load_golden(case)
    m = dnp.meta(g)
    model, P0 = dnp.scaled_model(g, cuda)
    model.train()
    fd = dnp.feed(g, 1, cuda)
    with torch.no_grad():
        B, Cn = fd["item_id"].shape
        xs = model.cross_layers(model._fields(fd, Cn).reshape(B * Cn, -1))
    for l, x in enumerate(xs):
        _check(x, g["X%d" % l], f"{case} X{l}", *dnp.bound_for(g, "X%d" % l))
    out = model(fd)
    loss = model.loss(out)
    loss.backward()
    torch.cuda.synchronize()
    _check(out["prediction"], g["pred"], case + " pred", *dnp.bound_for(g, "pred"))
    _check(np.array([loss.item()]), np.array([float(g["loss"])]), case + " loss", *dnp.bound_for(g, "loss"))
    zero, gmax = set(str(k) for k in g["zero_grad_keys"]), 1e6 * dnp.grad_floor(g)
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(v is not None for v in grads.values()) and sorted(grads) == sorted(k[2:] for k in g if k.startswith("G/"))
    for k, got in grads.items():
        want, got = dnp.stored(g, "G/", k, got.cpu().numpy())
        if k in zero:
            assert float(np.abs(got).max()) <= 1e-5 * gmax, (case, k)
            continue
        bound, why = dnp.bound_for(g, "G/" + k)
        _check(got, want, f"{case} grad {k}", bound, why, floor=dnp.grad_floor(g))
    if m["mixed"] and m["E"] == 1:      # as in the reference: an exact zero, not None
        assert (grads["gating.0.weight"] == 0).all() and (grads["gating.0.bias"] == 0).all()
        assert (g["G/gating.0.weight"] == 0).all() and (g["G/gating.0.bias"] == 0).all()


@pytest.mark.parametrize("case", CASES)
def test_two_optimizer_steps_match_the_reference_golden(case, cuda, tmp_path):
    from helpers.BaseRunner import BaseRunner
    g = load_golden(case)
    opt = [k[:-6] for k in g if k.endswith("_hyper")][0]
    lr, l2 = (float(x) for x in g[opt + "_hyper"])
    model, P0 = dnp.scaled_model(g, cuda)
    model.train()
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.optimizer, a.lr, a.l2, a.train, a.log_file = opt, lr, l2, 1, str(tmp_path / "log.txt")
    model.optimizer = BaseRunner(a)._build_optimizer(model)
    losses = []
    for n in (1, 2):
        model.optimizer.zero_grad()
        ls = model.loss(model(dnp.feed(g, n, cuda)))
        ls.backward()
        model.optimizer.step()
        losses.append(ls.item())
    torch.cuda.synchronize()
    print(f"DCNV2_LOSSES {case} {opt}: {losses} (reference {g[opt + '_losses'].tolist()})")
    np.testing.assert_allclose(losses, g[opt + "_losses"], rtol=TOL)
    zero = set(str(k) for k in g["zero_grad_keys"])
    adaptive = opt in ("Adam", "Adagrad")
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(g["%s/%s" % (opt, k)]) == 2
            continue
        want, got = dnp.stored(g, opt + "/", k, v.cpu().numpy())
        start = dnp.stored(g, opt + "/", k, P0[k])[1]
        if k in zero:
            # the gradient is round-off around an exact zero: Adam / Adagrad normalise it to a step of about lr in a direction the
            # round-off decides, in the reference as well -- only the size of the move is held
            assert float(np.abs(got - start).max()) <= (2.5 * lr if adaptive else 1e-5) + 1e-7, (case, k)
            continue
        extra = 1e-3 * lr if adaptive else 0.0
        if adaptive and k.endswith(".running_mean") and "deep_layers.mlp.%d.bias" % (int(k.split(".")[2]) - 1) in zero:
            extra = 0.1 * 2.5 * lr      # the batch mean contains the bias in front, which the first step moved by about lr
        assert_update_close(got, start, want, what=f"{case} {opt} {k}", extra_atol=extra, outlier_atol=2 * lr if adaptive else 0.0)


def test_a_stack_issues_one_forward_and_one_backward_call_per_layer(cuda, monkeypatch):
    from rechorus_amd import _lib
    g = load_golden("dcnv2_a_ctr_mix_stacked_d16_r8_e2_l3")
    model, _ = dnp.scaled_model(g, cuda)
    model.train()
    calls, inner = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name) or inner(name, *a))
    out = model(dnp.feed(g, 1, cuda))
    assert [c for c in calls if c.startswith("rc_dcnv2")] == ["rc_dcnv2_mix_layer_fwd"] * 3, calls
    del calls[:]
    model.loss(out).backward()
    assert [c for c in calls if c.startswith("rc_dcnv2")] == ["rc_dcnv2_mix_layer_bwd"] * 3, calls
    model.eval()
    pred = model(dnp.feed(g, 1, cuda))["prediction"]
    assert not pred.requires_grad


# ---- CLI: the four demo flag sets ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx_root(tmp_path_factory):
    from synth_data import make_context_dataset
    root = str(tmp_path_factory.mktemp("dcnv2_data"))
    make_context_dataset(root, "ctr", n_users=200, n_items=100, per_user=12, ctr=True, seed=3, numeric=True)
    make_context_dataset(root, "topk", n_users=200, n_items=100, per_user=10, ctr=False, seed=4)
    return root


@pytest.mark.parametrize("mode,mixed,structure,experts,layers", [("CTR", 1, "stacked", 2, 3), ("TopK", 1, "parallel", 1, 4),
                                                                 ("CTR", 0, "parallel", 2, 3), ("TopK", 0, "stacked", 2, 2)])
def test_cli_trains_and_evaluates_the_demo_flag_sets(mode, mixed, structure, experts, layers, ctx_root, tmp_path, cuda, monkeypatch):
    import main
    from rechorus_amd import nn as hnn
    fused, fwd0, ev0 = [], hnn.dcnv2_mix_layer, hnn.dcnv2_mix_layer_eval
    monkeypatch.setattr(hnn, "dcnv2_mix_layer", lambda *a, **k: fused.append("train") or fwd0(*a, **k))
    monkeypatch.setattr(hnn, "dcnv2_mix_layer_eval", lambda *a, **k: fused.append("eval") or ev0(*a, **k))
    log = str(tmp_path / "run.txt")
    task = (["--model_mode", "CTR", "--loss_n", "BCE", "--dataset", "ctr", "--metric", "AUC,ACC", "--include_situation_features", "1"]
            if mode == "CTR" else ["--model_mode", "TopK", "--dataset", "topk", "--num_neg", "2", "--topk", "5,10"])
    res = main.run(["--model_name", "DCNv2", "--emb_size", "16", "--layers", "[16]", "--cross_layer_num", str(layers), "--mixed", str(mixed),
                    "--structure", structure, "--low_rank", "8", "--expert_num", str(experts), "--reg_weight", "0.01", "--lr", "5e-3",
                    "--l2", "0", "--path", ctx_root + "/", "--epoch", "1", "--batch_size", "256", "--num_workers", "0",
                    "--regenerate", "1", "--include_item_features", "1", "--include_user_features", "1", "--log_file", log,
                    "--model_path", str(tmp_path / "m.pt"), "--save_final_results", "0"] + task)
    found = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", open(log).read())
    assert found and np.isfinite(float(found.group(1))), open(log).read()[-2000:]
    assert ("AUC" if mode == "CTR" else "HR@5") in res["test"]
    assert ("train" in fused and "eval" in fused) == bool(mixed), fused
