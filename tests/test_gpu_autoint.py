"""GPU: AutoInt on the HIP engine (rc_autoint_layer_fwd / _bwd) against the reference's goldens
(tests/golden/make_golden_autoint.py) and the float64 restatement (tests/autoint_np.py): every layer's output, prediction, loss,
every parameter gradient and two optimizer steps of each golden through the model file; the layer kernels at every tile edge, field
count, width and head split of the grid below; a saturating softmax and an all-negative pre-activation; bit-identical reruns,
untouched inputs, the launch count of a stack, the evaluation forward, the refusals of the entry points and the CLI with graph
replay on and off.

Tolerances: 2e-5 of the tensor's largest entry (the project's cap).  Where a golden stores the reference's own fp32-vs-float64
deviation for a tensor and it exceeds 1e-5, that tensor's bound is twice the stored deviation (autoint_np.bound_for says so in the
printed line).  A gradient that is exactly zero in exact arithmetic is compared no finer than 1e-6 of the batch's largest gradient
entry (autoint_np.grad_floor); under Adam / Adagrad such a gradient is normalised to a step of up to lr in either direction, in the
reference as well, so those tensors' and the named bias elements' steps are only bounded (2.5 lr).  Each comparison prints its bound and the largest error it saw
(AUTOINT_TOL lines, run with -s; tools/autoint_tolerance_report.py folds that output into profiles/autoint_tolerances.txt)."""
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
import autoint_np as anp  # noqa: E402
from autoint_np import TOL, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = golden_cases("autoint_")
GRAD_NAMES = ("dX", "dWq", "dWk", "dWv", "dWr", "dbr")


def _check(got, want, what, bound=TOL, floor=0.0, why="the cap"):
    if torch.is_tensor(got):
        got = got.detach().cpu().numpy()
    err = rel_err(np.asarray(got).reshape(np.shape(want)), want, floor)
    print(f"AUTOINT_TOL {what}: {err:.3e} (allowed {bound:.3g}: {why})")
    assert err <= bound, f"{what}: largest error / largest entry {err:.3e} > {bound:g}"
    return err


def _runner(opt, lr, l2, ctr):
    from helpers.BaseRunner import BaseRunner
    from helpers.CTRRunner import CTRRunner
    cls = CTRRunner if ctr else BaseRunner
    a, _ = cls.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.train, a.log_file = 1, "/tmp/rechorus_amd_test/log.txt"
    a.optimizer, a.lr, a.l2, a.graph, a.engine = opt, lr, l2, 0, "dense"
    return cls(a)


def _zero_in_exact_arithmetic(g, key):
    """under BPR the gradients of a row's candidates sum to zero, so whatever shifts every candidate of a row alike has an exactly
    zero gradient: overall_bias, the tower's output bias, the first-order weights of the per-row fields"""
    if anp.meta(g)["ctr"]:
        return False
    if key == "overall_bias" or (key.startswith("deep_layers.") and key.endswith(".bias") and g["G/" + key].size == 1):
        return True
    return key.startswith("linear_embedding.") and anp.batch(g, 1)[key.split(".")[1]].ndim == 1


@pytest.mark.parametrize("case", CASES)
def test_golden_case(case, cuda):
    g = load_golden(case)
    m = anp.meta(g)
    model = anp.build_model(g, cuda)
    model.train()
    fd = anp.feed(g, 1, cuda)
    with torch.no_grad():
        X, _ = model._get_embeddings_FM(fd)
        for l, Y in enumerate(model.interacting_layers(X)):
            _check(Y, g["Y%d" % l], f"{case} Y{l}")
    out = model(fd)
    assert ("loss" in out) == m["ctr"]          # CTR training: the head's terms, the sigmoid and BCE are one kernel
    loss = model.loss(out)
    loss.backward()
    _check(out["prediction"], g["pred"], case + " pred", *anp.bound_for(g, "pred")[:1], why=anp.bound_for(g, "pred")[1])
    assert abs(loss.item() - float(g["loss"])) <= TOL * max(1.0, abs(float(g["loss"]))), (case, loss.item(), float(g["loss"]))
    for k, p in model.named_parameters():
        bound, why = anp.bound_for(g, k)
        _check(p.grad, g["G/" + k], f"{case} grad {k}", bound, anp.grad_floor(g), why)

    P0 = anp.scaled_params(g)
    for opt in ("Adam", "SGD", "Adagrad"):
        if opt + "_hyper" not in g:
            continue
        lr, l2 = (float(x) for x in g[opt + "_hyper"])
        m2 = anp.build_model(g, cuda)
        m2.optimizer = _runner(opt, lr, l2, m["ctr"])._build_optimizer(m2)
        m2.train()
        adaptive = opt in ("Adam", "Adagrad")
        extra = 1e-3 * lr if adaptive else 0.0      # per step taken (conftest.assert_update_close)
        # Adam / Adagrad normalise a gradient element that is round-off around an exact zero to a step of up to lr in a direction the
        # round-off decides.  Only elements without weight decay can be such: a weight's gradient has l2 * p (about 2e-5 here) added
        # to it.  They are named: |g| < 1e-7 in the reference's own autograd, an exact 0 included (the one-row TopK golden's two
        # candidates carry BPR gradients +x and -x, so dbr cancels to EXACTLY 0 in the reference and to round-off here), in the
        # parameters of the no-decay group (with l2 = 0: in every dense parameter).  Their steps are bounded by 2.5 lr, as
        # test_gpu_deepfm.py bounds them; every other element is compared.
        def ill_of(k):
            table = k.split(".")[0] in ("context_embedding", "linear_embedding")
            if not adaptive or table or (l2 > 0 and "bias" not in k):
                return None
            return np.abs(g["G/" + k]) < 1e-7
        ill = {k: ill_of(k) for k in P0}
        free = [k for k in P0 if not (adaptive and _zero_in_exact_arithmetic(g, k))]
        n_ill = sum(int(ill[k].sum()) for k in free if ill[k] is not None)
        first_step_stored = "%s/s1/overall_bias" % opt in g

        def compare(ref, start, steps, tag):
            for k, v in m2.state_dict().items():
                got = v.detach().cpu().numpy()
                if k not in free:
                    assert np.abs(got - P0[k]).max() <= 2.5 * lr, (case, opt, tag, k)
                    continue
                assert_update_close(got, start[k], ref[k], what=f"{case} {opt} {tag} {k}", extra_atol=steps * extra,
                                    outlier_atol=steps * lr, exclude=ill[k])
                if ill[k] is not None and ill[k].any():
                    assert np.abs(got - start[k])[ill[k]].max() <= 2.5 * lr, (case, opt, tag, k)
        losses = []
        S1 = {k: g["%s/s1/%s" % (opt, k)] for k in P0} if first_step_stored else None
        for step in (1, 2):
            m2.optimizer.zero_grad()
            ls = m2.loss(m2(anp.feed(g, step, cuda)))
            ls.backward()
            m2.optimizer.step()
            losses.append(ls.item())
            if step == 1 and first_step_stored:
                # the two TopK goldens store the first step as well: it is compared on its own, and the named elements are then set
                # to the reference's values, so that the second step starts where the reference's did and is compared in full
                # (comparing two compounded steps would let those elements' arbitrary directions leak into every other element)
                compare(S1, P0, 1, "step 1")
                with torch.no_grad():
                    for k, v in m2.state_dict().items():
                        mask = np.ones(P0[k].shape, dtype=bool) if k not in free else ill[k]
                        if mask is not None and mask.any():
                            v[torch.from_numpy(mask).to(cuda)] = torch.from_numpy(S1[k][mask]).to(cuda)
        print(f"AUTOINT_LOSSES {case} {opt}: {losses} (reference {g[opt + '_losses'].tolist()}; {n_ill} ill-conditioned elements)")
        final = {k: g["%s/%s" % (opt, k)] for k in P0}
        if first_step_stored:
            compare(final, S1, 1, "step 2")
        else:
            compare(final, P0, 2, "two steps")
        for step, (ls, want) in enumerate(zip(losses, g[opt + "_losses"].tolist()), 1):
            assert abs(ls - want) <= TOL * max(1.0, abs(want)), (case, opt, step, ls, want)


# ---- the layer kernels against float64 ----------------------------------------------------------------------------------------------
# (6, 3): attention_size no multiple of 4 -- the stacked weight block padded per part, the scalar Y store, the partial G fill
FS, DINS, HEADS = (2, 3, 7, 8, 9, 32), (8, 36, 64, 128), ((4, 4), (8, 1), (32, 1), (32, 2), (64, 8), (6, 3))


def tile_edge_counts(F):
    """1, 3, one tile's instance count - 1 / exactly / + 1 for each of the three tile heights (128, 64 and 32 stacked rows: which one a
    shape runs at depends on what fits the LDS, and differs between forward and backward), and 257: several tiles per workgroup"""
    ns = {1, 3, 257}
    for rows in (128, 64, 32):
        ti = rows // F
        ns.update(n for n in (ti - 1, ti, ti + 1) if n >= 1)
    return sorted(ns)


def layer_problem(N, F, Din, A, H, seed, **kw):
    """random_layer plus its float64 results; asserts the two conditions the goldens meet (unless the case is a degenerate one)"""
    prob = anp.random_layer(N, F, Din, A, H, seed, **kw)
    Y, f = anp.layer_forward(*prob[:6], H, details=True)
    return prob, Y, f["P"]


def _run_layer(prob, H, cuda, workspace=None):
    from rechorus_amd import engine
    t = [torch.from_numpy(a).to(cuda) for a in prob]
    Y = engine.autoint_layer_fwd(*t[:6], H)
    grads = engine.autoint_layer_bwd(*t[:5], Y, t[6], H, workspace=workspace)
    return t, Y, grads


@pytest.mark.parametrize("A,H", HEADS)
@pytest.mark.parametrize("Din", DINS)
@pytest.mark.parametrize("F", FS)
def test_layer_kernels_against_float64(F, Din, A, H, cuda):
    from rechorus_amd import engine
    ws = engine.AutoIntWorkspace()
    for N in tile_edge_counts(F):
        what = f"N={N} F={F} Din={Din} A={A} H={H}"
        prob, Yw, P = layer_problem(N, F, Din, A, H, seed=1000 * F + Din + A + H + N)
        if N * F >= 64:      # enough rows for the shares to mean something
            assert (P.max(-1) > anp.row_threshold(F)).mean() >= 0.5, what
            assert 0.25 <= (Yw > 0).mean() <= 0.75, what
        _, Y, grads = _run_layer(prob, H, cuda, ws)
        _check(Y, Yw, what + " Y")
        want = anp.layer_backward(*prob[:6], H, prob[6])
        for name, got in zip(GRAD_NAMES, grads):
            _check(got, want[name], f"{what} {name}")


def test_capped_grid_walks_several_tiles_per_workgroup(cuda):
    # 4 instances per tile at F = 32: 2,053 instances are 514 tiles on the 512 workgroups the grid is capped at
    N, F, Din, A, H = 2053, 32, 8, 4, 4
    prob, Yw, _ = layer_problem(N, F, Din, A, H, seed=5)
    _, Y, grads = _run_layer(prob, H, cuda)
    _check(Y, Yw, "capped grid Y")
    want = anp.layer_backward(*prob[:6], H, prob[6])
    for name, got in zip(GRAD_NAMES, grads):
        _check(got, want[name], f"capped grid {name}")


def test_saturating_softmax(cuda):
    N, F, Din, A, H = 300, 8, 64, 32, 2
    prob, Yw, P = layer_problem(N, F, Din, A, H, seed=6, score_std=20.0)
    S = anp.layer_forward(*prob[:6], H, details=True)[1]["S"]
    spread = float(np.median(S.max(-1) - S.min(-1)))
    assert 40.0 <= spread <= 90.0, spread            # about 60: most rows are one-hot to fp32
    assert (P.max(-1) > 0.999).mean() > 0.5
    _, Y, grads = _run_layer(prob, H, cuda)
    assert torch.isfinite(Y).all()
    _check(Y, Yw, "saturating softmax Y")
    want = anp.layer_backward(*prob[:6], H, prob[6])
    for name, got in zip(GRAD_NAMES, grads):
        assert torch.isfinite(got).all(), name
        _check(got, want[name], f"saturating softmax {name}")


def test_all_negative_pre_activations_give_exact_zeros(cuda):
    N, F, Din, A, H = 70, 7, 36, 8, 1
    prob, Yw, _ = layer_problem(N, F, Din, A, H, seed=7, relu_shift=-1.0e3)
    assert (Yw == 0).all()
    _, Y, grads = _run_layer(prob, H, cuda)
    assert (Y == 0).all()
    for name, got in zip(GRAD_NAMES, grads):
        assert (got == 0).all(), name               # dZ = dY * (Y > 0) = 0: every product behind it is an exact zero


def test_reruns_are_bit_identical_and_inputs_stay_unchanged(cuda):
    for shape in ((2053, 32, 8, 4, 4), (4099, 8, 64, 32, 1), (257, 9, 36, 64, 8)):
        prob, _, _ = layer_problem(*shape, seed=11)
        H = shape[4]
        runs = []
        for _ in range(2):
            t, Y, grads = _run_layer(prob, H, cuda)
            runs.append([x.cpu().numpy().copy() for x in (Y,) + tuple(grads)])
            for a, b in zip(t, prob):      # X, the weights, the bias and dY after forward and backward
                assert a.cpu().numpy().tobytes() == b.tobytes(), shape
        for a, b in zip(*runs):
            assert a.tobytes() == b.tobytes(), shape


def test_a_stack_issues_one_forward_and_one_backward_call_per_layer(cuda, monkeypatch):
    from rechorus_amd import _lib
    g = load_golden("autoint_topk_d16_a8_h4_l3_k4")
    model = anp.build_model(g, cuda)
    model.train()
    fd = anp.feed(g, 1, cuda)
    calls, inner = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name) or inner(name, *a))
    out = model(fd)
    fwd = [c for c in calls if c.startswith("rc_autoint")]
    assert fwd == ["rc_autoint_layer_fwd"] * 3, calls
    del calls[:]
    model.loss(out).backward()
    assert [c for c in calls if c.startswith("rc_autoint")] == ["rc_autoint_layer_bwd"] * 3, calls


def test_evaluation_forward(cuda):
    from rechorus_amd import nn as hnn
    g = load_golden("autoint_topk_d16_a8_h4_l3_k4")
    m = anp.meta(g)
    model = anp.build_model(g, cuda)
    att, res = model.autoint_attentions[0], model.residual_embeddings[0]
    X = torch.zeros(2, 1, len(m["fields"]), m["d"], device=cuda)
    with pytest.raises(RuntimeError, match="no backward"):
        hnn.autoint_layer_eval(X, att.q_linear.weight, att.k_linear.weight, att.v_linear.weight, res.weight, res.bias, m["H"])
    # --test_all style: 100 candidates per row, item-side fields per candidate
    rng = np.random.default_rng(3)
    b = {k: v.copy() for k, v in anp.batch(g, 1).items()}
    B, C = m["B"], 100
    b["item_id"] = rng.integers(1, m["n_items"], (B, C)).astype(np.int64)
    for f in m["fields"]:
        if b[f].ndim == 2 and f != "item_id":
            b[f] = rng.integers(0, int(g["feature_max"][m["fields"].index(f)]), (B, C)).astype(np.int64)
    fd = {k: torch.from_numpy(v).to(cuda) for k, v in b.items()}
    fd.update(batch_size=B, phase="test")
    model.eval()
    pred = model(fd)["prediction"]                  # the model's evaluation forward needs no torch.no_grad() around it
    assert not pred.requires_grad and pred.shape == (B, C)
    _check(pred, anp.model_forward(anp.scaled_params(g), g, b)["raw"], "evaluation forward, 100 candidates")


def test_entry_points_refuse_bad_arguments_by_return_code(cuda):
    import ctypes as C
    from rechorus_amd import _lib
    lib = _lib.load()
    N, F, d, A, H = 10, 8, 64, 32, 1
    z = lambda *s: torch.zeros(*s, device=cuda)
    X, W, br, Y = z(N, F, d), z(A, d), z(A), torch.full((N, F, A), 7.0, device=cuda)
    dX, dW, db = torch.full((N, F, d), 7.0, device=cuda), torch.full((A, d), 7.0, device=cuda), torch.full((A,), 7.0, device=cuda)
    ws = torch.zeros(lib.rc_autoint_workspace_bytes(N, F, d, A, H), dtype=torch.uint8, device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(x=p(X), br_=p(br), n=N, f=F, h=H, y=p(Y)):
        return lib.rc_autoint_layer_fwd(x, p(W), p(W), p(W), p(W), br_, n, f, d, A, h, y, st)

    def bwd(wsp=p(ws), nbytes=ws.numel(), dy=p(Y), n=N, h=H, dx=p(dX)):
        return lib.rc_autoint_layer_bwd(p(X), p(W), p(W), p(W), p(W), p(Y), dy, n, F, d, A, h, wsp, nbytes, dx, p(dW), p(dW), p(dW), p(dW),
                                        p(db), st)
    for call, code in ((lambda: fwd(x=None), -1), (lambda: fwd(br_=None), -1), (lambda: fwd(y=None), -1), (lambda: fwd(n=0), -4),
                       (lambda: fwd(f=33), -4), (lambda: fwd(h=5), -4), (lambda: fwd(y=C.c_void_p(Y.data_ptr() + 4)), -1),
                       (lambda: bwd(wsp=None), -1), (lambda: bwd(nbytes=ws.numel() - 256), -2), (lambda: bwd(dy=None), -1),
                       (lambda: bwd(h=3), -4), (lambda: bwd(n=-1), -4), (lambda: bwd(dx=None), -1)):
        assert call() == code, lib.rc_last_error_string()
        assert lib.rc_last_error_string().startswith(b"rc_autoint_layer_")
    torch.cuda.synchronize()
    for t in (Y, dX, dW, db):
        assert (t == 7.0).all()                     # nothing was launched
    assert fwd() == 0 and bwd() == 0


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx_root(tmp_path_factory):
    from synth_data import make_context_dataset
    root = str(tmp_path_factory.mktemp("autoint_data"))
    make_context_dataset(root, "ctr", n_users=300, n_items=150, per_user=20, ctr=True, seed=3, numeric=True)
    make_context_dataset(root, "topk", n_users=300, n_items=150, per_user=12, ctr=False, seed=4)
    return root


@pytest.mark.parametrize("mode", ["CTR", "TopK"])
def test_cli_trains_one_epoch_with_graph_replay_on_and_off(mode, ctx_root, tmp_path, cuda, monkeypatch):
    import main
    from rechorus_amd import graph as hgraph, nn as hnn
    replays, fused = [], []
    run0, fwd0 = hgraph.GraphedStep.run, hnn.autoint_layer
    monkeypatch.setattr(hgraph.GraphedStep, "run", lambda self, b: replays.append(1) or run0(self, b))
    monkeypatch.setattr(hnn, "autoint_layer", lambda *a, **k: fused.append(1) or fwd0(*a, **k))
    losses = {}
    for graph in ("1", "0"):
        log = str(tmp_path / ("log" + graph) / "run.txt")
        task = (["--model_mode", "CTR", "--loss_n", "BCE", "--dataset", "ctr", "--metric", "AUC,ACC", "--include_situation_features", "1"]
                if mode == "CTR" else ["--model_mode", "TopK", "--dataset", "topk", "--num_neg", "2", "--topk", "5,10"])
        n_replays = len(replays)
        res = main.run(["--model_name", "AutoInt", "--emb_size", "16", "--attention_size", "8", "--num_heads", "2", "--num_layers", "2",
                        "--layers", "[16]", "--lr", "5e-3", "--l2", "0", "--path", ctx_root + "/", "--epoch", "1", "--batch_size", "256",
                        "--num_workers", "0", "--regenerate", "1", "--include_item_features", "1", "--include_user_features", "1",
                        "--graph", graph, "--log_file", log, "--model_path", str(tmp_path / ("m" + graph + ".pt")),
                        "--save_final_results", "0"] + task)
        text = open(log).read()
        found = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", text)
        assert found and np.isfinite(float(found.group(1))), text[-2000:]
        losses[graph] = found.group(1)
        assert ("AUC" if mode == "CTR" else "HR@5") in res["test"]
        if mode == "CTR":
            assert (len(replays) > n_replays) == (graph == "1")      # the CTR step replays from a hipGraph when asked to
        else:
            # AutoIntTopK, like DeepFMTopK, does not declare candidate_permutation_equivariant: BaseRunner shuffles its candidate
            # columns on the host and never replays it, so both runs are eager and the equal losses show a repeatable step only
            assert len(replays) == n_replays
    assert fused and losses["1"] == losses["0"], losses
