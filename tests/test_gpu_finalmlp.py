"""GPU: FinalMLP on the HIP engine (csrc/finalmlp.hip) against the float64 restatement (tests/finalmlp_np.py) and the goldens of the
reference (tests/golden/make_golden_finalmlp.py).  Every comparison is |error| <= 2e-5 of the tensor's largest entry
(conftest.assert_close with rtol = 0, which also puts it on the tolerance record); a backward is checked with the ReLU / dropout mask
read from the kernel's own output, after asserting that this mask differs from float64's only where the float64 pre-activation is
round-off (within 1e-5 of the layer's largest)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)
import finalmlp_np as fnp  # noqa: E402
from finalmlp_np import TOL  # noqa: E402

pytestmark = pytest.mark.gpu


def _close(got, want, what, floor=0.0):
    if torch.is_tensor(got):
        got = got.detach().cpu().numpy()
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    print(f"FINALMLP_TOL {what}: {fnp.rel_err(got, want, floor):.3e}")
    assert_close(got, want, rtol=0.0, atol_scale=TOL, what=what, abs_floor=floor)


def _scalar(got, want, what):
    """a loss: |error| <= 2e-5 max(1, |want|), on the tolerance record like every tensor"""
    assert_close(np.array([got]), np.array([want]), rtol=TOL, atol_scale=0.0, what=what, abs_floor=TOL * max(0.0, 1.0 - abs(want)))


def _stream(rng, D, G, H, rows, logit_sd=1.5):
    return [rng.standard_normal((rows, G)).astype(np.float32), (rng.standard_normal((D, G)) * logit_sd / np.sqrt(G)).astype(np.float32),
            (0.5 * rng.standard_normal(D)).astype(np.float32), (rng.standard_normal((H, D)) / np.sqrt(D)).astype(np.float32),
            (0.5 * rng.standard_normal(H)).astype(np.float32)]


def _rows(kind, N, C):
    return {"1": 1, "B": N // C, "N": N}[kind]


def _dev(arrs, cuda):
    return [torch.from_numpy(a).to(cuda) for a in arrs]


def _gate_case(cuda, N, C, D, G, H, kinds, p=(0.0, 0.0), seed=0):
    from rechorus_amd import engine
    rng = np.random.default_rng(1000 * N + D + seed)
    X = rng.standard_normal((N, D)).astype(np.float32)
    st = [_stream(rng, D, G[s], H[s], _rows(kinds[s], N, C)) for s in (0, 1)]
    dA = [rng.standard_normal((N, H[s])).astype(np.float32) for s in (0, 1)]
    Xd, std, dAd = torch.from_numpy(X).to(cuda), [_dev(s, cuda) for s in st], _dev(dA, cuda)
    seeds = [torch.tensor([12345 + 7 * s + seed], dtype=torch.int64, device=cuda) for s in (0, 1)]
    full = [tuple(std[s]) + (p[s], seeds[s] if p[s] > 0 else None, 100 + s) for s in (0, 1)]
    return engine, X, st, dA, Xd, std, dAd, full


def _check_gate(cuda, N, C, D, G, H, kinds, p=(0.0, 0.0), tag=""):
    engine, X, st, dA, Xd, std, dAd, full = _gate_case(cuda, N, C, D, G, H, kinds, p)
    keep = [t.clone() for t in [Xd] + std[0] + std[1]]
    A = engine.finalmlp_gate_fwd(Xd, C, full[0], full[1])
    masks = []
    for s in (0, 1):
        g, pre = fnp.gate_fwd(X, st[s], C)
        got = A[s].cpu().numpy().astype(np.float64)
        scale = 1.0 / (1.0 - p[s])
        on = got != 0.0
        if p[s] == 0.0:
            _close(got, np.maximum(pre, 0.0), f"{tag} A{s + 1}")
            flipped = on != (pre > 0.0)
            assert np.abs(pre[flipped]).max(initial=0.0) <= 1e-5 * np.abs(pre).max(), (tag, s, int(flipped.sum()))
        else:
            # every element is 0 or relu(pre) / (1 - p); the dropped share of the positive ones within 5 binomial standard deviations
            _close(np.where(on, got, 0.0), np.where(on, np.maximum(pre, 0.0) * scale, 0.0), f"{tag} A{s + 1} kept")
            assert not (on & (pre < -1e-5 * np.abs(pre).max())).any()
            pos = pre > 1e-5 * np.abs(pre).max()
            n, dropped = int(pos.sum()), int((pos & ~on).sum())
            if n:
                assert abs(dropped - p[s] * n) <= 5.0 * np.sqrt(n * p[s] * (1.0 - p[s])) + 1.0, (tag, s, dropped, n)
        masks.append(on * scale)
    dX, g1, g2 = engine.finalmlp_gate_bwd(Xd, C, full[0], full[1], A[0], dAd[0], A[1], dAd[1])
    want_dX = 0.0
    for s, grads in ((0, g1), (1, g2)):
        dXs, *want = fnp.gate_bwd(X, st[s], C, masks[s], dA[s])
        want_dX = want_dX + dXs
        for name, got, w in zip(("dZin", "dWg", "dbg", "dW", "db"), grads, want):
            _close(got, w, f"{tag} {name}{s + 1}")
    _close(dX, want_dX, f"{tag} dX")
    for t, k in zip([Xd] + std[0] + std[1], keep):
        assert torch.equal(t, k), "an input was written"
    return engine, Xd, full, A, dAd, (dX, g1, g2)


# N x D x G x H x gate rows: every value of the grids at least once, the edges paired (1 with the widest, 4,099 with the widest, ...).
# 256 gate inputs and a 256-wide first layer in ONE stream are outside the envelope (the backward's LDS); they sit in different streams
GATE_GRID = [
    (1, 1, 12, (4, 4), (4, 36), "11"),
    (1, 1, 520, (256, 4), (4, 256), "11"),
    (31, 1, 36, (20, 4), (36, 4), "1N"),
    (33, 1, 96, (64, 20), (64, 36), "N1"),
    (33, 3, 36, (20, 20), (36, 64), "BB"),
    (127, 1, 512, (64, 64), (64, 256), "N1"),
    (129, 1, 520, (256, 4), (36, 64), "1N"),
    (1000, 4, 96, (20, 256), (256, 4), "BN"),
    (1000, 4, 12, (4, 64), (4, 256), "1B"),
    (4099, 1, 12, (256, 64), (36, 4), "N1"),
    (4099, 1, 520, (64, 256), (256, 36), "N1"),
    # more tiles than the forward's 1,024 workgroups (32-row tiles at these gate widths): the grid-stride loop over tiles, its
    # barrier, the accumulators' re-initialisation and the reuse of the LDS from tile to tile
    (32801, 1, 12, (256, 256), (36, 4), "N1"),
]


@pytest.mark.parametrize("N,C,D,G,H,kinds", GATE_GRID)
def test_gate_kernels(cuda, N, C, D, G, H, kinds):
    _check_gate(cuda, N, C, D, G, H, kinds, tag=f"gate N={N} D={D} G={G} H={H} {kinds}")


@pytest.mark.parametrize("p", [0.3, 0.5])
def test_gate_dropout(cuda, p):
    engine, Xd, full, A, dAd, _ = _check_gate(cuda, 1000, 4, 96, (20, 64), (64, 36), "BN", p=(p, p), tag=f"dropout p={p}")
    full2 = [f[:6] + (f[6] + 1, f[7]) for f in full]      # bumped seeds: another mask
    A2 = engine.finalmlp_gate_fwd(Xd, 4, full2[0], full2[1])
    assert not torch.equal(A[0], A2[0]) and not torch.equal(A[1], A2[1])
    A3 = engine.finalmlp_gate_fwd(Xd, 4, full[0], full[1])
    assert torch.equal(A[0], A3[0]) and torch.equal(A[1], A3[1])


def test_gate_saturated(cuda):
    """logits of +-30 (the bias; Zin is ordinary, Wg tiny): g in {0, 2} to fp32, and a finite dz that is zero to round-off, seen in
    every gradient dz feeds: dbg, dWg = dz^T Zin and dZin = dz Wg (one gate row per instance)"""
    from rechorus_amd import engine
    N, D, G, H = 64, 36, 4, 8
    rng = np.random.default_rng(5)
    Xn = rng.standard_normal((N, D)).astype(np.float32)
    X = torch.from_numpy(Xn).to(cuda)
    streams, host = [], []
    for s in (0, 1):
        bg = np.where(rng.random(D) < 0.5, -30.0, 30.0).astype(np.float32)
        st = [rng.standard_normal((N, G)).astype(np.float32), (1e-3 * rng.standard_normal((D, G))).astype(np.float32), bg,
              (rng.standard_normal((H, D)) / 6).astype(np.float32), np.zeros(H, np.float32)]
        host.append(st)
        streams.append(tuple(_dev(st, cuda)) + (0.0, None, 0))
    A1, A2 = engine.finalmlp_gate_fwd(X, 1, *streams)
    dAn = [rng.standard_normal((N, H)).astype(np.float32) for _ in (0, 1)]
    dA = _dev(dAn, cuda)
    dX, g1, g2 = engine.finalmlp_gate_bwd(X, 1, *streams, A1, dA[0], A2, dA[1])
    assert torch.isfinite(dX).all()
    want_dX = 0.0
    for s, (grads, A) in enumerate(((g1, A1), (g2, A2))):
        gate, pre = fnp.gate_fwd(Xn, host[s], 1)
        assert np.minimum(np.abs(gate), np.abs(gate - 2.0)).max() < 1e-10
        _close(A, np.maximum(pre, 0.0), f"saturated A{s + 1}")
        dXs, dZin, dWg, dbg, dW, db = fnp.gate_bwd(Xn, host[s], 1, (A.cpu().numpy() != 0).astype(np.float64), dAn[s])
        want_dX = want_dX + dXs
        for t in grads:
            assert torch.isfinite(t).all()
        # dz = P X g (1 - g / 2) is at most |P X| 2 e^-30 = 1.9e-13 |P X|: zero against the other gradients' scale
        scale = float(np.abs(dW).max())
        for name, t in zip(("dZin", "dWg", "dbg"), grads[:3]):
            assert t.abs().max().item() <= 1e-9 * scale, (name, t.abs().max().item())
        _close(grads[3], dW, f"saturated dW{s + 1}")
        _close(grads[4], db, f"saturated db{s + 1}")
    _close(dX, want_dX, "saturated dX")


FUSION_GRID = [(4, 4, 1), (4, 4, 4), (12, 20, 4), (12, 36, 3), (64, 64, 2), (64, 256, 1), (256, 256, 4)]


def _fusion_case(cuda, N, H1, H2, h):
    rng = np.random.default_rng(N + 31 * H1 + H2 + h)
    ar = [rng.standard_normal((N, H1)), rng.standard_normal((N, H2)), rng.standard_normal((h * (H1 // h) * (H2 // h), 1)) / np.sqrt(H1 * H2 / h),
          rng.standard_normal((1, H1)) / np.sqrt(H1), rng.standard_normal(1), rng.standard_normal((1, H2)) / np.sqrt(H2), rng.standard_normal(1),
          rng.standard_normal(N)]
    ar = [a.astype(np.float32) for a in ar]
    return ar, _dev(ar, cuda)


@pytest.mark.parametrize("H1,H2,h", FUSION_GRID)
@pytest.mark.parametrize("N", [1, 33, 129, 4099])
def test_fusion_kernels(cuda, N, H1, H2, h):
    from rechorus_amd import engine
    (x, y, wxy, wx, bx, wy, by, dout), dev = _fusion_case(cuda, N, H1, H2, h)
    keep = [t.clone() for t in dev]
    tag = f"fusion N={N} ({H1}, {H2}, {h})"
    out = engine.finalmlp_fusion_fwd(*dev[:7], h)
    # (the output is a sum of three terms of either sign: the bound is against the largest of them, not their sum)
    lin, bil = fnp.fusion_terms(x, y, wxy, wx, wy, h)
    want = fnp.fusion_fwd(x, y, wxy, wx, bx, wy, by, h)
    _close(out, want, tag + " out", floor=TOL * max(np.abs(lin).max(), np.abs(bil).max()))
    got = engine.finalmlp_fusion_bwd(dev[0], dev[1], dev[2], dev[3], dev[5], dev[7], h)
    for name, g, w in zip(("dx", "dy", "dw_xy", "dw_x", "db_x", "dw_y", "db_y"), got, fnp.fusion_bwd(x, y, wxy, wx, wy, dout, h)):
        _close(g, w, f"{tag} {name}")
    for t, k in zip(dev, keep):
        assert torch.equal(t, k), "an input was written"


def test_entry_points(cuda):
    """bit-identical reruns of both backwards, the evaluation entries against the training forward, no graph on the evaluation path,
    the refusals"""
    from rechorus_amd import engine, nn as hnn, _lib
    engine_, X, st, dA, Xd, std, dAd, full = _gate_case(cuda, 1000, 4, 96, (20, 64), (64, 36), "BN")
    A = engine.finalmlp_gate_fwd(Xd, 4, *full)
    ws = engine.FinalMLPWorkspace()
    r1 = engine.finalmlp_gate_bwd(Xd, 4, *full, A[0], dAd[0], A[1], dAd[1], workspace=ws)
    r2 = engine.finalmlp_gate_bwd(Xd, 4, *full, A[0], dAd[0], A[1], dAd[1], workspace=ws)
    for a, b in zip([r1[0], *r1[1], *r1[2]], [r2[0], *r2[1], *r2[2]]):
        assert torch.equal(a, b)
    params = [t.clone().requires_grad_(True) for t in [Xd] + std[0] + std[1]]
    A_tr = hnn.finalmlp_gate(params[0], 4, tuple(params[1:6]), tuple(params[6:11]), workspace=ws)
    assert A_tr[0].requires_grad and torch.equal(A_tr[0], A[0]) and torch.equal(A_tr[1], A[1])
    (A_tr[0] * dAd[0]).sum().add((A_tr[1] * dAd[1]).sum()).backward()
    for p_, want in zip(params, [r1[0], *r1[1], *r1[2]]):
        assert torch.equal(p_.grad, want)
    with pytest.raises(RuntimeError):
        hnn.finalmlp_gate_eval(params[0], 4, tuple(params[1:6]), tuple(params[6:11]))
    with torch.no_grad():
        A_ev = hnn.finalmlp_gate_eval(params[0], 4, tuple(params[1:6]), tuple(params[6:11]))
    assert not A_ev[0].requires_grad and A_ev[0].grad_fn is None and torch.equal(A_ev[0], A[0]) and torch.equal(A_ev[1], A[1])

    (x, y, wxy, wx, bx, wy, by, dout), dev = _fusion_case(cuda, 1000, 64, 256, 1)
    out = engine.finalmlp_fusion_fwd(*dev[:7], 1)
    b1 = engine.finalmlp_fusion_bwd(dev[0], dev[1], dev[2], dev[3], dev[5], dev[7], 1, workspace=ws)
    b2 = engine.finalmlp_fusion_bwd(dev[0], dev[1], dev[2], dev[3], dev[5], dev[7], 1, workspace=ws)
    for a, b in zip(b1, b2):
        assert torch.equal(a, b)
    fp = [t.clone().requires_grad_(True) for t in dev[:7]]
    o_tr = hnn.finalmlp_fusion(*fp, 1, workspace=ws)
    assert torch.equal(o_tr, out)
    (o_tr * dev[7]).sum().backward()
    for p_, want in zip(fp, (b1[0], b1[1], b1[2], b1[3], b1[4], b1[5], b1[6])):
        assert torch.equal(p_.grad.reshape(-1), want.reshape(-1))
    with pytest.raises(RuntimeError):
        hnn.finalmlp_fusion_eval(*fp, 1)
    with torch.no_grad():
        o_ev = hnn.finalmlp_fusion_eval(*fp, 1)
    assert o_ev.grad_fn is None and torch.equal(o_ev, out)

    # refusals: the widths of one stream beyond the backward's LDS, a width off the grid of 4, a head count that does not divide,
    # a gate with a row count that is none of the three, CPU tensors
    bad = _stream(np.random.default_rng(0), 96, 256, 256, 1)
    with pytest.raises(_lib.RechorusHipError, match="LDS"):
        engine.finalmlp_gate_bwd(Xd, 4, tuple(_dev(bad, cuda)) + (0.0, None, 0), full[1], torch.zeros(1000, 256, device=cuda),
                                 torch.zeros(1000, 256, device=cuda), A[1], dAd[1])
    odd = _stream(np.random.default_rng(0), 96, 6, 8, 1)
    with pytest.raises(_lib.RechorusHipError, match="envelope"):
        engine.finalmlp_gate_fwd(Xd, 4, tuple(_dev(odd, cuda)) + (0.0, None, 0), full[1])
    with pytest.raises(ValueError):
        engine.finalmlp_gate_fwd(Xd, 4, tuple(_dev(_stream(np.random.default_rng(0), 96, 8, 8, 7), cuda)) + (0.0, None, 0), full[1])
    with pytest.raises(ValueError, match="num_heads"):
        engine.finalmlp_fusion_fwd(*dev[:7], 3)
    with pytest.raises(ValueError):
        engine.finalmlp_gate_fwd(Xd.cpu(), 4, *full)
    with pytest.raises(ValueError, match="dropout"):
        engine.finalmlp_gate_fwd(Xd, 4, full[0][:5] + (0.5, None, 0), full[1])


# ---- the model file ---------------------------------------------------------------------------------------------------------------------
import argparse  # noqa: E402
import re  # noqa: E402

from conftest import assert_update_close, golden_cases, load_golden  # noqa: E402

CASES = golden_cases("finalmlp_")


def _runner(opt, lr, l2, ctr):
    from helpers.BaseRunner import BaseRunner
    from helpers.CTRRunner import CTRRunner
    cls = CTRRunner if ctr else BaseRunner
    a, _ = cls.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.train, a.log_file = 1, "/tmp/rechorus_amd_test/log.txt"
    a.optimizer, a.lr, a.l2, a.graph, a.engine = opt, lr, l2, 0, "dense"
    return cls(a)


def _zero_in_exact_arithmetic(cfg, key):
    """under BPR the gradients of a row's candidates sum to zero, so whatever shifts every candidate of a row alike has an exactly zero
    gradient: the fusion's two biases"""
    return (not cfg["ctr"]) and key in ("fusion_module.w_x.bias", "fusion_module.w_y.bias")


def _first_layer_outputs(model, fd):
    """A_1, A_2 through the evaluation entry of the gate kernel, on the model's own parameters"""
    from rechorus_amd import nn as hnn
    n_cand = fd["item_id"].shape[1]
    with torch.no_grad():
        flat = model._flat_fields(fd, n_cand)
        if not model.use_fs:
            x2 = flat.reshape(-1, flat.shape[-1])
            return [hnn.linear(x2, b.mlp[0].weight, b.mlp[0].bias, relu=True) for b in (model.mlp1, model.mlp2)]
        st1, st2 = (model._stream_spec(s, fd, n_cand, False)[0] for s in (1, 2))
        return hnn.finalmlp_gate_eval(flat, n_cand, st1, st2)


@pytest.mark.parametrize("case", CASES)
def test_golden_case(case, cuda):
    g = load_golden(case)
    cfg = fnp.config(g)
    model = fnp.build_model(g, cuda)
    model.train()
    fd = fnp.feed(g, 1, cuda)
    for s, A in enumerate(_first_layer_outputs(model, fd), 1):
        _close(A, g["A%d" % s], f"{case} A{s}")
    out = model(fd)
    loss = model.loss(out)
    loss.backward()
    _close(out["prediction"], g["pred"], case + " pred")
    _scalar(loss.item(), float(g["loss"]), case + " loss")
    floor = fnp.grad_floor(g)
    for k, p in model.named_parameters():
        # |error| <= bound * max(largest entry, floor): conftest.assert_close with rtol = 0 and the floor's share as abs_floor
        bound, why = fnp.bound_for(g, k)
        want = g["G/" + k].astype(np.float64)
        err = fnp.rel_err(p.grad.cpu().numpy(), want, floor)
        print(f"FINALMLP_TOL {case} grad {k}: {err:.3e} (allowed {bound:.3g}: {why})")
        assert_close(p.grad.cpu().numpy(), want, rtol=0.0, atol_scale=bound, what=f"{case} grad {k}",
                     abs_floor=bound * max(0.0, floor - float(np.abs(want).max())), loose=None if bound <= TOL else why)

    P0 = fnp.params(g)
    for opt in ("Adam", "SGD"):
        if opt + "_hyper" not in g:
            continue
        lr, l2 = (float(x) for x in g[opt + "_hyper"])
        m2 = fnp.build_model(g, cuda)
        m2.optimizer = _runner(opt, lr, l2, cfg["ctr"])._build_optimizer(m2)
        m2.train()
        adaptive = opt == "Adam"
        extra = 1e-3 * lr if adaptive else 0.0      # per step taken (conftest.assert_update_close)

        # Adam normalises a gradient element that is round-off around an exact zero to a step of up to lr in a direction the round-off
        # decides.  Only elements without weight decay can be such (a weight's gradient has l2 * p added).  They are named: |g| < 1e-7
        # in the reference's own autograd, in the dense no-decay parameters; their steps are bounded by 2.5 lr, every other element
        # is compared.
        def ill_of(k):
            if not adaptive or k.startswith("embedding_dict.") or "ctx_emb" in k and "bias" not in k or (l2 > 0 and "bias" not in k):
                return None
            return np.abs(g["G/" + k]) < 1e-7
        ill = {k: ill_of(k) for k in P0}
        free = [k for k in P0 if not (adaptive and _zero_in_exact_arithmetic(cfg, k))]
        losses = []
        for step in (1, 2):
            m2.optimizer.zero_grad()
            ls = m2.loss(m2(fnp.feed(g, step, cuda)))
            ls.backward()
            m2.optimizer.step()
            losses.append(ls.item())
        print(f"FINALMLP_LOSSES {case} {opt}: {losses} (reference {g[opt + '_losses'].tolist()})")
        for k, v in m2.state_dict().items():
            got = v.detach().cpu().numpy()
            if k not in free:
                assert np.abs(got - P0[k]).max() <= 2.5 * lr, (case, opt, k)
                continue
            assert_update_close(got, P0[k], g["%s/%s" % (opt, k)], what=f"{case} {opt} {k}", extra_atol=2 * extra, outlier_atol=2 * lr,
                                exclude=ill[k])
            if ill[k] is not None and ill[k].any():
                assert np.abs(got - P0[k])[ill[k]].max() <= 2.5 * lr, (case, opt, k)
        for step, (ls, want) in enumerate(zip(losses, g[opt + "_losses"].tolist()), 1):
            _scalar(ls, want, f"{case} {opt} loss of step {step}")


def test_demo_widths_against_restatement(cuda):
    """F = 8, d = 64, fs [64], mlp1 [64], mlp2 [256], one head, the MIND demo's contexts, N = 1,024: the whole model against float64"""
    g = load_golden("finalmlp_mind_ctr_d8")
    cfg = fnp.config(g)
    from models.context.FinalMLP import FinalMLPCTR
    args, corpus = fnp.model_args(g, cuda, emb_size=64, mlp1_hidden_units="[64]", mlp2_hidden_units="[256]", fs_hidden_units="[64]")
    torch.manual_seed(5)
    model = FinalMLPCTR(args, corpus)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(20.0)
        for s in (1, 2):      # gate logits of order one, as the goldens' calibration leaves them
            last = [m for m in getattr(model.fs_module, "fs%d_gate" % s).mlp if isinstance(m, torch.nn.Linear)][-1]
            last.weight.mul_(4.0)
        model.fusion_module.w_xy.mul_(0.05)
    model = model.to(cuda).train()
    B = 1024
    rng = np.random.default_rng(8)
    fmax = cfg["feature_max"]
    b = {"user_id": rng.integers(1, fmax["user_id"], B), "item_id": rng.integers(1, fmax["item_id"], (B, 1)),
         "label": rng.integers(0, 2, (B, 1))}
    for f in cfg["sit"]:
        b[f] = rng.integers(0, fmax[f], B)
    for f in cfg["item"]:
        b[f] = rng.integers(0, fmax[f], (B, 1))
    fd = {k: torch.from_numpy(np.asarray(v, dtype=np.int64)).to(cuda) for k, v in b.items()}
    fd.update(batch_size=B, phase="train")
    P = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    fl = cfg["flags"]
    want = fnp.Model64(P, dict(context_features=cfg["context_features"], use_fs=1, num_heads=1, ctr=True,
                               fs1_context=fl["fs1_context"].split(","), fs2_context=fl["fs2_context"].split(","))).forward(b)
    g1 = want["gate1"]
    assert ((g1 < 0.5) | (g1 > 1.5)).mean() > 0.1, "the gates of this check are not all near 1"
    for s, A in enumerate(_first_layer_outputs(model, fd), 1):
        _close(A, want["A%d" % s].reshape(B, -1), f"demo widths A{s}")
    out = model(fd)
    _close(out["prediction"], want["prediction"], "demo widths prediction")
    p64 = np.clip(want["prediction"], 1e-12, 1 - 1e-12)
    y = b["label"].reshape(-1)
    loss64 = float(-(y * np.log(p64) + (1 - y) * np.log(1 - p64)).mean())
    loss = model.loss(out)
    _scalar(loss.item(), loss64, "demo widths loss")
    for p in model.parameters():
        p.grad = None
    # the backward of both kernels at these widths and N = 1,024, on the model's own tensors: the autograd nodes are intercepted, given
    # a known upstream gradient, and every gradient they return is held to the restatement (mask from the kernel's own A)
    from rechorus_amd import nn as hnn
    seen = {}
    gate0, fuse0 = hnn.finalmlp_gate, hnn.finalmlp_fusion

    def gate(X, n_cand, st1, st2, workspace=None):
        leaves = [t.detach().clone().requires_grad_(True) for t in (X,) + tuple(st1[:5]) + tuple(st2[:5])]
        A = gate0(leaves[0], n_cand, tuple(leaves[1:6]), tuple(leaves[6:11]), workspace=workspace)
        seen["gate"] = (leaves, A)
        return gate0(X, n_cand, st1, st2, workspace=workspace)

    def fusion(x, y, *par, workspace=None):
        leaves = [t.detach().clone().requires_grad_(True) for t in (x, y) + tuple(par[:5])]
        seen["fusion"] = (leaves, fuse0(*leaves, par[5], workspace=workspace))
        return fuse0(x, y, *par, workspace=workspace)
    hnn.finalmlp_gate, hnn.finalmlp_fusion = gate, fusion
    try:
        model.loss(model(fd)).backward()
    finally:
        hnn.finalmlp_gate, hnn.finalmlp_fusion = gate0, fuse0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    rng = np.random.default_rng(9)
    leaves, A = seen["gate"]
    dA = [rng.standard_normal(tuple(t.shape)).astype(np.float32) for t in A]
    torch.autograd.backward(list(A), _dev(dA, cuda))
    host = [t.detach().cpu().numpy() for t in leaves]
    want_dX = 0.0
    for s_ in (0, 1):
        st = host[1 + 5 * s_:6 + 5 * s_]
        _, pre = fnp.gate_fwd(host[0].reshape(B, -1), st, 1)
        on = A[s_].detach().cpu().numpy() != 0
        flipped = on != (pre > 0)
        assert np.abs(pre[flipped]).max(initial=0.0) <= 1e-5 * np.abs(pre).max()
        dXs, *wants = fnp.gate_bwd(host[0].reshape(B, -1), st, 1, on.astype(np.float64), dA[s_])
        want_dX = want_dX + dXs
        for name, t, w in zip(("dZin", "dWg", "dbg", "dW", "db"), leaves[1 + 5 * s_:6 + 5 * s_], wants):
            _close(t.grad, w, f"demo widths {name}{s_ + 1}")
    _close(leaves[0].grad, want_dX, "demo widths dX")
    leaves, o = seen["fusion"]
    dout = rng.standard_normal(B).astype(np.float32)
    o.backward(torch.from_numpy(dout).to(cuda).view(o.shape))
    host = [t.detach().cpu().numpy() for t in leaves]
    wants = fnp.fusion_bwd(host[0], host[1], host[2], host[3], host[5], dout, 1)
    for name, t, w in zip(("dx", "dy", "dw_xy", "dw_x", "db_x", "dw_y", "db_y"), [leaves[k] for k in (0, 1, 2, 3, 4, 5, 6)], wants):
        _close(t.grad, w, f"demo widths fusion {name}")


@pytest.fixture(scope="module")
def ctx_root(tmp_path_factory):
    from synth_data import make_context_dataset
    root = str(tmp_path_factory.mktemp("finalmlp_data"))
    make_context_dataset(root, "ctr", n_users=300, n_items=150, per_user=20, ctr=True, seed=3, numeric=True)
    make_context_dataset(root, "topk", n_users=300, n_items=150, per_user=12, ctr=False, seed=4)
    return root


@pytest.mark.parametrize("mode", ["CTR", "TopK"])
def test_cli_trains_one_epoch_with_graph_replay_on_and_off(mode, ctx_root, tmp_path, cuda, monkeypatch):
    import main
    from rechorus_amd import graph as hgraph, nn as hnn
    replays, fused = [], []
    run0, gate0, fuse0 = hgraph.GraphedStep.run, hnn.finalmlp_gate, hnn.finalmlp_fusion
    monkeypatch.setattr(hgraph.GraphedStep, "run", lambda self, b: replays.append(1) or run0(self, b))
    monkeypatch.setattr(hnn, "finalmlp_gate", lambda *a, **k: fused.append("gate") or gate0(*a, **k))
    monkeypatch.setattr(hnn, "finalmlp_fusion", lambda *a, **k: fused.append("fusion") or fuse0(*a, **k))
    losses = {}
    for graph in ("1", "0"):
        log = str(tmp_path / ("log" + graph) / "run.txt")
        task = (["--model_mode", "CTR", "--loss_n", "BCE", "--dataset", "ctr", "--metric", "AUC,ACC", "--fs1_context", "c_hour_c,c_weekday_c,c_day_f",
                 "--fs2_context", "i_category_c"]
                if mode == "CTR" else ["--model_mode", "TopK", "--dataset", "topk", "--num_neg", "2", "--topk", "5,10", "--fs2_context", "c_hour_c"])
        n_replays = len(replays)
        # both runs draw the same dropout seeds: the seed generator is the process's, re-seeded from --random_seed when first used
        monkeypatch.setattr(hnn, "_DROP_SEED_GEN", None)
        res = main.run(["--model_name", "FinalMLP", "--emb_size", "16", "--mlp1_hidden_units", "[16]", "--mlp2_hidden_units", "[32,16]",
                        "--fs_hidden_units", "[16]", "--num_heads", "2", "--mlp2_dropout", "0.2", "--lr", "5e-3", "--l2", "0",
                        "--path", ctx_root + "/", "--epoch", "1", "--batch_size", "256", "--num_workers", "0", "--regenerate", "1",
                        "--include_item_features", "1", "--include_situation_features", "1", "--graph", graph, "--log_file", log,
                        "--model_path", str(tmp_path / ("m" + graph + ".pt")), "--save_final_results", "0"] + task)
        text = open(log).read()
        found = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", text)
        assert found and np.isfinite(float(found.group(1))), text[-2000:]
        losses[graph] = found.group(1)
        assert ("AUC" if mode == "CTR" else "HR@5") in res["test"]
        if mode == "CTR":
            assert (len(replays) > n_replays) == (graph == "1")      # the CTR step replays from a hipGraph when asked to
    assert "gate" in fused and "fusion" in fused and losses["1"] == losses["0"], losses
