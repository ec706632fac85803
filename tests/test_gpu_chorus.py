"""GPU: Chorus's kernels, autograd node, trainer and model file against the float64 restatement (tests/chorus_np.py) and the
reference's own numbers (tests/golden/chorus_*.npz; per array the larger of 2e-5 and four times the reference's own float32-against-
float64 deviation recorded there).

Shapes are the smallest at which a lane, slot or segment mistake shows: ids are drawn from 7 users, 11 items and 5 categories, so
users, candidates and categories repeat across tuples, a candidate repeats inside a tuple, a negative equals the positive and row 0
and the last row occur; the intervals hold -1, exact zeros and a tuple without any; betas + 1 and sigmas + 1 sit below, on and above
the clamp, and small betas + 1 push an unclamped kernel value beyond +1 and beyond -1.  B runs on both sides of the front's tuples
per workgroup (rc_chorus_front_tuples_per_block; the front has one path for every C), n_occ on both sides of the category update's
piece size (rc_chorus_category_piece).  Only in-range ids are ever passed.

Tolerances (conftest.assert_close: |got - want| <= rtol |want| + atol_scale max|want|): scores 1e-5 / 1e-5, everything else at most
2e-5 / 2e-5, nothing excluded.  With the reason where a comparison has more:
  * the tables after an Adam / Adagrad step go through conftest.assert_update_close with extra_atol = 1e-3 lr, as every trainer test
    of the project: the step lr g / (sqrt(v) + eps) is ill-conditioned where |g| ~ eps;
  * sum_c gpred[b, c] is exactly 0 in exact arithmetic under the BPR loss, so ubgrad and user_bias's gradient are round-off on both
    sides: held to a floor of 2e-5 max|gpred| per tuple of the user, and user_bias after an Adam / Adagrad step to lr (the largest
    step those optimizers take).  The kernels behind them are compared tightly with gradients that are not round-off (the
    weighted-sum loss of the autograd test, the given gpred of the scores_bwd test).
"""
import argparse
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close, assert_update_close, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import chorus_np  # noqa: E402
from chorus_np import CAT_TABLES, PARAMS, STATE_KEYS  # noqa: E402
from slrc_data import make_kg_dataset  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

pytestmark = pytest.mark.gpu
N_USERS, N_ITEMS, N_CAT = 7, 11, 5
T2 = dict(rtol=2e-5, atol_scale=2e-5)
KINDS = {1: [0], 2: [0, 1], 3: [0, 1, 2], 8: [0, 1, 2, 0, 2, 1, 1, 2]}


def _kinds(R, rot=0):
    """every kind reaches every position over rot = 0, 1, 2"""
    return [(k + rot) % 3 for k in KINDS[R]]


def _problem(d, R, B, Cn, seed=0, n_cat=N_CAT):
    rng = np.random.default_rng(10000 * d + 1000 * R + 10 * B + Cn + seed)
    f = np.float32
    P = {"U": rng.normal(0, 0.3, (N_USERS, d)).astype(f), "I": rng.normal(0, 0.3, (N_ITEMS, d)).astype(f),
         "Rel": rng.normal(0, 0.3, (R, d)).astype(f), "w": rng.normal(0, 0.7, (1, d)).astype(f),
         "user_bias": rng.normal(0, 0.3, (N_USERS, 1)).astype(f), "item_bias": rng.normal(0, 0.3, (N_ITEMS, 1)).astype(f),
         "betas": rng.normal(0, 0.3, (n_cat, R)).astype(f), "sigmas": rng.normal(0, 0.2, (n_cat, R)).astype(f),
         "mus": rng.normal(0, 0.5, (n_cat, R)).astype(f)}
    if n_cat >= 5:
        P["betas"][0, 0], P["betas"][1, R - 1], P["betas"][2, 0] = -1.5, 9.0, 11.0       # betas + 1: below 1e-10, exactly 10, above 10
        P["sigmas"][3, 0], P["sigmas"][4, R - 1], P["sigmas"][2, R - 1] = -1.5, 9.0, 11.0
        P["betas"][3, R - 1] = -0.8                    # beta = 0.2: n(0; 0, 0.2) = 1.99 > 1 and -n(0; 0, 0.2) < -1, exp kernel 0.2 < 1
        P["betas"][4, 0] = 1.5                         # beta = 2.5: the exponential kernel at dt = 0 is 2.5 > 1
    uid = rng.integers(0, N_USERS, B).astype(np.int64)
    iid = rng.integers(0, N_ITEMS, (B, Cn)).astype(np.int64)
    cid = rng.integers(0, n_cat, (B, Cn)).astype(np.int64)
    if Cn >= 2:
        iid[0, 1] = iid[0, 0]                          # a negative equals the positive
    if Cn >= 3:
        iid[0, 2] = iid[0, 1]                          # a candidate repeats inside the tuple
    uid[0], iid[B - 1, 0], cid[B - 1, 0] = 0, 0, 0     # row 0 ...
    uid[B - 1], iid[0, Cn - 1], cid[0, Cn - 1] = N_USERS - 1, N_ITEMS - 1, n_cat - 1      # ... and the last row occur
    iv = np.where(rng.random((B, Cn, R)) < 0.35, -1.0, rng.uniform(0.0, 3.0, (B, Cn, R))).astype(f)
    iv[rng.random((B, Cn, R)) < 0.1] = 0.0             # intervals of exactly 0 (where the kernels peak)
    iv[0, 0, 0] = 0.0
    if B >= 2:
        iv[B - 1] = -1.0                               # a tuple without any interval
    return P, uid, iid, cid, iv


def _dev(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def _devP(dev, P):
    return _dev(dev, *(P[k] for k in PARAMS))


def _np(t):
    return t.detach().cpu().numpy()


def _check_front(d, R, B, Cn, kinds, gmf, dev, all_off=False):
    from rechorus_amd import engine
    P, uid, iid, cid, iv = _problem(d, R, B, max(Cn, 2))
    iid, cid, iv = (np.ascontiguousarray(x[:, :Cn]) for x in (iid, cid, iv))
    if all_off:
        iv[:] = -1.0
    tag = f"d={d} R={R} B={B} C={Cn} kinds={kinds} gmf={gmf}"
    want_pred = chorus_np.scores(P, uid, iid, cid, iv, kinds, gmf)
    # only the one-candidate tensor carries the floor (see _dot_magnitude); every other shape is held to the relative bound alone
    dot_floor = 1e-6 * _dot_magnitude(P, uid, iid, cid, iv, kinds, gmf) if B * Cn == 1 else 0.0
    dP, ids = _devP(dev, P), _dev(dev, uid, iid, cid, iv)
    assert_close(_np(engine.chorus_scores(dP, *ids, kinds, gmf)), want_pred, what=f"scores {tag}", abs_floor=dot_floor)
    # the backward for a given gradient that is not round-off anywhere
    gin = np.random.default_rng(Cn).normal(0, 1, (B, Cn)).astype(np.float32)
    kmax = max(np.abs(v).max() for v in chorus_np.kernels(chorus_np.f64(P), cid, iv, kinds)[2].values())
    _check_outputs(engine.chorus_scores_grads(dP, *ids, kinds, _dev(dev, gin)[0], gmf),
                   chorus_np.front_grads(P, uid, iid, cid, iv, kinds, gin, gmf), iv, gmf, "scores_bwd " + tag,
                   k_floor=dot_floor * np.abs(gin).max() * kmax)
    if Cn < 2:
        return
    want_lv, want_g = chorus_np.bpr(want_pred)
    want = chorus_np.front_grads(P, uid, iid, cid, iv, kinds, want_g, gmf)
    for want_p in (True, False):
        out = engine.chorus_fwd_bwd(dP, *ids, kinds, gmf, want_pred=want_p)
        if want_p:
            assert_close(_np(out["pred"]), want_pred, what=f"fwd_bwd pred {tag}", abs_floor=dot_floor)
        else:
            assert out["pred"] is None
        assert_close(_np(out["loss_vec"]), want_lv, what=f"loss_vec {tag}", **T2)
        assert_close(_np(out["gpred"]), want_g, what=f"gpred {tag}", **T2)
        _check_outputs(out, want, iv, gmf, "fwd_bwd " + tag, ub_floor=2e-5 * np.abs(want_g).max(),
                       k_floor=dot_floor * np.abs(want_g).max() * kmax)


def _dot_magnitude(P, uid, iid, cid, iv, kinds, gmf):
    """max over the candidates of sum_d |u'_d z_d|, the size of the terms a score's inner product adds up.  A float32 inner product
    of n <= 136 terms is exact to about sqrt(n) 2^-24 < 1e-6 of that sum, whatever the sum itself cancels to -- and with B = C = 1 the
    one score of the tensor IS such a cancelling sum, so max|want| is no scale for it.  At B = C = 1, and only there, the score and
    the kgrad row (g times <u', I[i]> + <u', Rel[r]> times a kernel derivative) carry this floor beside the relative tolerance."""
    Pd = chorus_np.f64(P)
    decay, _, _ = chorus_np.kernels(Pd, cid, iv, kinds)
    z = (1.0 + decay.sum(-1))[:, :, None] * Pd["I"][iid] + np.einsum("bcr,rd->bcd", decay, Pd["Rel"])
    up = Pd["U"][uid] * Pd["w"].reshape(-1) if gmf else Pd["U"][uid]
    return float(np.abs(up[:, None, :] * z).sum(-1).max())


def _check_outputs(out, want, iv, gmf, tag, ub_floor=None, k_floor=0.0):
    B, Cn, R = iv.shape
    for k in ("coef", "ugrad", "kgrad", "GRel") + (("gw", "uprime") if gmf else ()):
        assert_close(_np(out[k]), want[k], what=f"{k} {tag}", abs_floor=k_floor if k == "kgrad" else 0.0, **T2)
    if not gmf:
        assert out["gw"] is None and out["uprime"] is None
    if ub_floor is None:
        assert_close(_np(out["ubgrad"]), want["ubgrad"], what=f"ubgrad {tag}", **T2)
    else:
        assert_close(_np(out["ubgrad"]), np.zeros(B), what=f"ubgrad {tag}", abs_floor=ub_floor)     # exactly 0 in exact arithmetic
    masked = np.tile((iv < 0).reshape(B * Cn, R), (1, 3))                                          # [betas | sigmas | mus]
    assert not _np(out["kgrad"])[masked].any(), tag                                                # the mask gives exact zeros


@pytest.mark.parametrize("gmf", [False, True])
@pytest.mark.parametrize("d", [16, 32, 64, 128])
def test_scores_and_front_against_float64(d, gmf, cuda):
    from rechorus_amd import engine
    tpb = engine.chorus_front_tuples_per_block()
    assert tpb == 16
    for R in (1, 2, 3, 8):
        for B in (1, tpb - 1, tpb + 1):
            for Cn in (1, 2, 5, 100):
                for rot in ((0, 1, 2) if (B == tpb + 1 and Cn in (2, 5)) else (0,)):
                    _check_front(d, R, B, Cn, _kinds(R, rot), gmf, cuda)


@pytest.mark.parametrize("gmf", [False, True])
def test_front_with_the_whole_catalogue_and_without_any_interval(gmf, cuda):
    for d, R in ((16, 1), (64, 3), (128, 8)):
        _check_front(d, R, 3, 1031, _kinds(R), gmf, cuda)                    # --test_all
        _check_front(d, R, 5, 7, _kinds(R, 1), gmf, cuda, all_off=True)      # every decay is 0


def test_problem_reaches_both_clamps_of_the_kernel_value():
    """the fixture itself: unclamped kernel values beyond +1 and beyond -1, and parameters on every side of their clamp"""
    P, uid, iid, cid, iv = _problem(64, 3, 17, 100)
    for rot in (0, 1, 2):
        _, kappa, _ = chorus_np.kernels(chorus_np.f64(P), cid, iv, _kinds(3, rot))
        on = iv >= 0
        assert (kappa[on] > 1).any() and ((kappa[on] < -1).any() or rot == 1)
    xb = P["betas"] + 1
    assert (xb < 1e-10).any() and (xb == 10).any() and (xb > 10).any()


def _cat_keys(n, mode, rng):
    if mode == "one":
        return np.zeros(n, dtype=np.int64), 1
    if mode == "own":
        return rng.permutation(n).astype(np.int64), n
    n_cat = 37
    return np.minimum(rng.zipf(1.3, n) - 1, n_cat - 1).astype(np.int64), n_cat


@pytest.mark.parametrize("mode", ["one", "own", "zipf"])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_category_update_on_both_sides_of_the_piece_size(R, mode, cuda):
    from rechorus_amd import engine
    Pz = engine.chorus_category_piece()
    assert Pz == 1024
    for n in (1, Pz - 1, Pz, Pz + 1, 3 * Pz + 7):
        rng = np.random.default_rng(n + R)
        cid, n_cat = _cat_keys(n, mode, rng)
        kgrad = rng.normal(0, 1, (n, 3 * R)).astype(np.float32)
        want = np.zeros((n_cat, 3 * R))
        np.add.at(want, cid, kgrad.astype(np.float64))
        d_cid, d_k = _dev(cuda, cid, kgrad)
        keys, perm = engine.sort_ids(d_cid, n_cat)
        _, heads, n_heads = engine.segment_heads(keys, perm, want_single=False)
        runs = []
        for _ in range(2):
            dense = [torch.zeros((n_cat, R), device=cuda) for _ in CAT_TABLES]
            # the workspace at exactly its declared bytes
            ws = torch.empty(engine._lib.load().rc_chorus_category_update_workspace_bytes(n, n_cat, R), dtype=torch.uint8, device=cuda)
            engine.chorus_category_update(keys, perm, heads, n_heads, d_k, n_cat, dense_grad=dense, workspace_buf=ws)
            runs.append(torch.cat(dense, dim=1))
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))                   # bit-identical between two runs
        # a sum of up to 3,079 unit normals in fp32: 2e-5 of the largest entry covers its rounding (sqrt(n) 6e-8 |sum| << 2e-5 max)
        assert_close(_np(runs[0]), want, what=f"category dense n={n} R={R} {mode}", **T2)
        # the in-place form on zero tables with SGD, lr = 1, l2 = 0 is w = fma(-1, g, 0) = -g: the same sums, exactly (compared as
        # floats: a category outside the batch keeps +0 in both, and its negation is -0)
        W = [torch.zeros((n_cat, R), device=cuda) for _ in CAT_TABLES]
        engine.chorus_category_update(keys, perm, heads, n_heads, d_k, n_cat, hyper=engine.make_hyper("SGD", 1.0, 0.0), W=W)
        assert torch.equal(-torch.cat(W, dim=1), runs[0])
        # Adam with state, against float64 on the rows of the batch; rows outside it and their state stay untouched
        W0 = rng.normal(0, 0.3, (n_cat, 3 * R)).astype(np.float32)
        Wd = [t.contiguous() for t in _dev(cuda, W0)[0].split(R, dim=1)]
        m, v = [torch.zeros_like(t) for t in Wd], [torch.zeros_like(t) for t in Wd]
        engine.chorus_category_update(keys, perm, heads, n_heads, d_k, n_cat, hyper=engine.make_hyper("Adam", 1e-3, 1e-5, step=1), W=Wd,
                                      m=m, v=v)
        W1, _, _ = chorus_np.optimizer_rows(W0, want, cid, "Adam", 1e-3, 1e-5)
        assert_update_close(_np(torch.cat(Wd, dim=1)), W0, W1, what=f"category Adam n={n} {mode}", rtol=2e-5, extra_atol=1e-6, strict=True)
        out = np.setdiff1d(np.arange(n_cat), cid)
        if out.size:
            assert np.array_equal(_np(torch.cat(Wd, dim=1))[out].view(np.int32), W0[out].view(np.int32))
            assert not _np(torch.cat(m, dim=1))[out].any()


def test_category_update_refuses_a_partial_set_of_dense_gradients(cuda):
    from rechorus_amd import _lib, engine
    cid = torch.zeros(4, dtype=torch.int64, device=cuda)
    keys, perm = engine.sort_ids(cid, 1)
    _, heads, n_heads = engine.segment_heads(keys, perm, want_single=False)
    k = torch.zeros((4, 3), device=cuda)
    dense = [torch.zeros((1, 1), device=cuda), None, torch.zeros((1, 1), device=cuda)]
    with pytest.raises(_lib.RechorusHipError, match="all three dense gradients"):
        engine.chorus_category_update(keys, perm, heads, n_heads, k, 1, dense_grad=dense)


@pytest.mark.parametrize("gmf", [False, True])
@pytest.mark.parametrize("d,R,B,Cn", [(16, 1, 1, 2), (32, 3, 3, 5), (64, 3, 17, 100), (128, 8, 5, 33)])
def test_dense_gradients_of_the_autograd_node_against_float64(d, R, B, Cn, gmf, cuda):
    from rechorus_amd import nn as hnn
    P, uid, iid, cid, iv = _problem(d, R, B, Cn)
    kinds = _kinds(R)
    params = [t.requires_grad_(True) for t in _devP(cuda, P)]
    ids = _dev(cuda, uid, iid, cid, iv)
    loss = hnn.bpr_loss(hnn.chorus_scores(params, *ids, kinds, gmf))
    loss.backward()
    want_lv, want_g = chorus_np.bpr(chorus_np.scores(P, uid, iid, cid, iv, kinds, gmf))
    assert_close(loss.item(), want_lv.mean(), what="loss", **T2)

    def check(want, what, ub=False):
        for k, p in zip(PARAMS, params):
            if want[k] is None:
                assert p.grad is None, k          # the head does not read it: no gradient, as in the reference
                continue
            assert p.grad.shape == p.shape
            floor = 2e-5 * np.abs(want_g).max() * np.bincount(uid, minlength=N_USERS).max() if (ub and k == "user_bias") else 0.0
            assert_close(_np(p.grad), want[k].reshape(p.shape), what=f"dense grad {k} {what}", abs_floor=floor, **T2)
    check(chorus_np.dense_grads(P, uid, iid, cid, iv, kinds, want_g, gmf), f"d={d} R={R} B={B} C={Cn} gmf={gmf}", ub=True)
    for p in params:
        p.grad = None
    w = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (B, Cn)).astype(np.float32)).to(cuda)
    (hnn.chorus_scores(params, *ids, kinds, gmf) * w).sum().backward()
    check(chorus_np.dense_grads(P, uid, iid, cid, iv, kinds, _np(w), gmf), "(weighted sum)")


def _trainer(P, dev, kinds, gmf, opt, lr, l2, lr_scale):
    from rechorus_amd import engine
    tabs = dict(zip(PARAMS, _devP(dev, P)))
    return engine.ChorusTrainer(*(tabs[k] for k in PARAMS), kinds=kinds, gmf=gmf, opt=opt, lr=lr, l2=l2, lr_scale=lr_scale), tabs


ROWS = {"U": 0, "user_bias": 0, "I": 1, "item_bias": 1, "betas": 2, "mus": 2, "sigmas": 2}


@pytest.mark.parametrize("gmf", [False, True])
@pytest.mark.parametrize("opt,lr,l2", [("SGD", 0.5, 1e-4), ("Adam", 1e-3, 1e-6), ("Adagrad", 0.01, 1e-4)])
@pytest.mark.parametrize("d,R,B,Cn", [(16, 1, 1, 2), (64, 3, 17, 100), (128, 8, 5, 33), (32, 3, 3, 5)])
def test_trainer_step_against_float64(d, R, B, Cn, opt, lr, l2, gmf, cuda):
    P, uid, iid, cid, iv = _problem(d, R, B, Cn)
    kinds, lr_scale = _kinds(R), 0.1
    # rows outside the batch exist on every row-wise table: one user, one item and one category are taken out by hand
    uid[uid == 3], iid[iid == 5], cid[cid == 1] = 2, 4, 2
    tr, tabs = _trainer(P, cuda, kinds, gmf, opt, lr, l2, lr_scale)
    ids = _dev(cuda, uid, iid, cid, iv)
    before = {k: tabs[k].clone() for k in PARAMS}
    want, states = dict(P), None
    for step_no in (1, 2):
        loss = tr.step(*ids)
        gmax = np.abs(chorus_np.bpr(chorus_np.scores(want, uid, iid, cid, iv, kinds, gmf))[1]).max() * np.bincount(uid).max()
        want_loss, want_new, states = chorus_np.step(want, uid, iid, cid, iv, kinds, opt, lr, l2, lr_scale, gmf, states, step_no)
        assert loss.shape == (1,) and tr.hyper.step == tr.hyper_kg.step == tr.hyper_bias.step == step_no
        assert_close(loss.item(), want_loss, what=f"{opt} loss step {step_no}", **T2)
        for k in PARAMS:
            klr = lr_scale * lr if k in ("I", "Rel") else lr
            extra = 1e-3 * klr if opt in ("Adam", "Adagrad") else 0.0
            if k == "user_bias":      # a round-off gradient (module docstring)
                extra = lr * 2e-5 * gmax if opt == "SGD" else lr
            assert_update_close(_np(tabs[k]), np.asarray(want[k]), want_new[k], what=f"{opt} {k} step {step_no} gmf={gmf}", rtol=2e-5,
                                extra_atol=extra, strict=True)
            for name, idx in (("m", 0), ("v", 1)):
                st = tr.state[k].get(name)
                if st is not None and k != "user_bias" and states[k][idx] is not None:
                    assert_close(_np(st), states[k][idx], what=f"{opt} {k} {name} step {step_no}", **T2)
        # continue from the float64 parameters narrowed to fp32: step 2 checks one step from a non-zero state, not two compounded
        for k in PARAMS:
            tabs[k].copy_(torch.from_numpy(want_new[k].astype(np.float32)))
            for name, idx in (("m", 0), ("v", 1)):
                if tr.state[k].get(name) is not None and states[k][idx] is not None:
                    tr.state[k][name].copy_(torch.from_numpy(states[k][idx].astype(np.float32)))
        want = {k: want_new[k].astype(np.float32) for k in PARAMS}
    # rows of every row-wise table (and of its state) outside the batch are bit-unchanged; so is a parameter the head does not read
    for k, which in ROWS.items():
        out = np.setdiff1d(np.arange(P[k].shape[0]), (uid, iid, cid)[which])
        assert out.size > 0, k
        out = torch.from_numpy(out).to(cuda)
        assert torch.equal(tabs[k][out].view(torch.int32), before[k][out].view(torch.int32)), k
        for st in tr.state[k].values():
            assert not st[out].any(), k
    for k in (("user_bias", "item_bias") if gmf else ("w",)) + (() if 2 in kinds else ("sigmas", "mus")):
        assert torch.equal(tabs[k].view(torch.int32), before[k].view(torch.int32)), k


@pytest.mark.parametrize("gmf", [False, True])
@pytest.mark.parametrize("opt", ["SGD", "Adam", "Adagrad"])
def test_two_runs_of_the_step_are_bit_identical(opt, gmf, cuda):
    P, uid, iid, cid, iv = _problem(64, 3, 130, 64)
    cid[:, 1::3] = 2          # a category with thousands of occurrences: several pieces
    ids = _dev(cuda, uid, iid, cid, iv)
    runs = []
    for _ in range(2):
        tr, tabs = _trainer(P, cuda, _kinds(3), gmf, opt, 0.01, 1e-5, 0.1)
        losses = [tr.step(*ids).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs.append([tabs[k] for k in PARAMS] + losses + [s for k in PARAMS for s in tr.state[k].values()])
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("gmf", [False, True])
@pytest.mark.parametrize("d,R,B,Cn", [(32, 3, 3, 5), (64, 3, 130, 64), (128, 8, 2, 101)])
def test_rowwise_sgd_without_weight_decay_agrees_with_the_dense_path_on_every_row(d, R, B, Cn, gmf, cuda):
    from rechorus_amd import nn as hnn
    P, uid, iid, cid, iv = _problem(d, R, B, Cn)
    kinds, lr, lr_scale = _kinds(R), 0.5, 0.1
    ids = _dev(cuda, uid, iid, cid, iv)
    tr, tabs = _trainer(P, cuda, kinds, gmf, "SGD", lr, 0.0, lr_scale)
    loss_row = tr.step(*ids)
    params = [t.requires_grad_(True) for t in _devP(cuda, P)]
    loss_dense = hnn.bpr_loss(hnn.chorus_scores(params, *ids, kinds, gmf))
    loss_dense.backward()
    assert_close(loss_row.item(), loss_dense.item(), what="loss")
    gmax = float(np.abs(chorus_np.bpr(chorus_np.scores(P, uid, iid, cid, iv, kinds, gmf))[1]).max()) * np.bincount(uid).max()
    for k, p in zip(PARAMS, params):
        if p.grad is None:
            assert torch.equal(tabs[k], p.detach()), k
            continue
        dense = p.detach() - (lr_scale * lr if k in ("I", "Rel") else lr) * p.grad
        assert_update_close(_np(tabs[k]).reshape(-1, 1), _np(p).reshape(-1, 1), _np(dense).reshape(-1, 1), what=f"row-wise vs dense {k}",
                            rtol=2e-5, extra_atol=lr * 2e-5 * gmax if k == "user_bias" else 0.0, strict=True)


# ---- every golden through the kernels, the autograd node and the model file, both engines -------------------------------------------

def _gtol(g, key):
    """the larger of 2e-5 and 4x the reference's own fp32-against-float64 deviation recorded in the golden"""
    t = max(2e-5, 4.0 * float(g["dev_" + key])) if "dev_" + key in g else 2e-5
    return dict(rtol=t, atol_scale=t, loose="4x the reference's own fp32-against-float64 deviation" if t > 2e-5 else None)


def _golden_model(g, dev, tmp_path, monkeypatch, stage=2):
    import pandas as pd
    from models.sequential.Chorus import Chorus
    n_users, n_items, n_cat, d, R, B, K, seed, redraw, gmf = (int(x) for x in g["meta"])
    lr, l2, lr_scale = (float(x) for x in g["hyper"])
    src = tmp_path / "src"
    src.mkdir(exist_ok=True)
    monkeypatch.chdir(src)
    meta = {"item_id": np.arange(1, n_items)}
    if n_cat > 1:
        meta["i_category"] = np.arange(n_items - 1) % n_cat
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, item_relations=g["relations"].tolist(), item_meta_df=pd.DataFrame(meta),
                             dataset="golden", include_attr=0)
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=K, dropout=0, test_all=0, emb_size=d, history_max=20,
                           time_scalar=8640000, stage=1, base_method="GMF" if gmf else "BPR", category_col="i_category",
                           lr_scale=lr_scale, margin=1.0, lr=lr)
    if not (tmp_path / "model").exists():
        Chorus(args, corpus).save_model()
    args.stage = stage
    m = Chorus(args, corpus).to(dev)
    m.load_state_dict({STATE_KEYS[k]: torch.from_numpy(g[k + "0"]) for k in PARAMS})     # a reference state_dict loads
    return m


def _runner(opt, lr, l2):
    from helpers.BaseRunner import BaseRunner
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.train, a.log_file = 1, "/tmp/rechorus_amd_test/log.txt"
    a.optimizer, a.lr, a.l2, a.graph, a.engine = opt, lr, l2, 0, "dense"
    return BaseRunner(a)


@pytest.mark.parametrize("case", golden_cases("chorus_d"))
def test_golden_case(case, cuda, tmp_path, monkeypatch):
    g = load_golden(case)
    lr, l2, lr_scale = (float(x) for x in g["hyper"])
    opt, B, gmf = str(g["opt"]), int(g["meta"][5]), bool(g["meta"][9])
    uid, iid, cid, iv = _dev(cuda, g["uid"], g["iid"], g["cid"], g["intervals"])
    feed = {"user_id": uid, "item_id": iid, "category_id": cid, "relational_interval": iv, "batch_size": B, "phase": "train"}
    m = _golden_model(g, cuda, tmp_path, monkeypatch)
    m.train()
    out = m(feed)
    assert_close(_np(out["prediction"]), g["pred"], what=case + " pred", **_gtol(g, "pred"))
    loss = m.loss(out)
    loss.backward()
    assert_close(loss.item(), float(g["loss"]), what=case + " loss", **_gtol(g, "loss"))
    sd = dict(m.named_parameters())
    ub_floor = 1e-5 * np.abs(g["Gitem_bias"]).max() if not gmf else 0.0      # the generator's bound on the reference's own round-off
    for k, has in zip(PARAMS, g["has_grad"]):
        if not has:
            assert sd[STATE_KEYS[k]].grad is None, k
            continue
        assert_close(_np(sd[STATE_KEYS[k]].grad), g["G" + k], what=f"{case} G{k}", abs_floor=ub_floor if k == "user_bias" else 0.0,
                     **_gtol(g, "G" + k))

    def check_two_steps(model, what):
        got = model.state_dict()
        for k, has in zip(PARAMS, g["has_grad"]):
            W, W0, W2 = _np(got[STATE_KEYS[k]]), g[k + "0"], g[k + "2"]
            if not has:
                assert np.array_equal(W.view(np.int32), W0.view(np.int32)), (case, what, k)      # no gradient: left alone
                continue
            klr = lr_scale * lr if k in ("I", "Rel") else lr
            extra = 2e-3 * klr if opt in ("Adam", "Adagrad") else 0.0
            if k == "user_bias":      # round-off on BOTH sides (module docstring), two steps
                extra = 4 * lr * ub_floor if opt == "SGD" else 4 * lr
            assert_update_close(W, W0, W2, what=f"{case} {what} {k} after two steps", extra_atol=extra, strict=True,
                                rtol=max(2e-5, 4 * float(g["dev_" + k + "2"])) if "dev_" + k + "2" in g else 2e-5)
    # the dense path: the optimizer BaseRunner builds from customize_parameters, two steps
    m2 = _golden_model(g, cuda, tmp_path, monkeypatch)
    m2.optimizer = _runner(opt, lr, l2)._build_optimizer(m2)
    m2.train()
    for _ in range(2):
        m2.optimizer.zero_grad()
        m2.loss(m2(feed)).backward()
        m2.optimizer.step()
    check_two_steps(m2, "dense")
    # the row-wise path: its loss is the golden's; with SGD and l2 = 0 a row outside the batch does not move under torch.optim
    # either, so two row-wise steps are held to the golden itself
    m3 = _golden_model(g, cuda, tmp_path, monkeypatch)
    loss3 = m3.hip_train_step(feed, opt, lr, l2)
    assert_close(loss3.item(), float(g["loss"]), what=case + " row-wise loss", **_gtol(g, "loss"))
    if opt == "SGD" and l2 == 0.0:
        m3.hip_train_step(feed, opt, lr, l2)
        check_two_steps(m3, "row-wise")
    assert list(m3.state_dict().keys()) == g["state_keys"].tolist()      # ... and the reverse of loading: the reference's keys


def test_golden_stage1_case(cuda, tmp_path, monkeypatch):
    """the stage-1 batch through the model file: kg_forward on rc_cfkg_scores, Chorus.loss, both gradients, two steps of the optimizer
    BaseRunner builds; the row-wise step's loss"""
    from models.sequential.Chorus import Chorus
    import pandas as pd
    g = load_golden("chorus_kg_stage1")
    n_items, R, d, B, seed = (int(x) for x in g["meta"])
    lr, l2, margin = (float(x) for x in g["hyper"])
    opt = str(g["opt"])
    monkeypatch.chdir(tmp_path)
    corpus = SimpleNamespace(n_users=10, n_items=n_items, item_relations=["r_complement", "r_substitute"][:R - 1],
                             item_meta_df=pd.DataFrame({"item_id": np.arange(1, n_items)}), dataset="golden", include_attr=0)
    args = SimpleNamespace(device=cuda, model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=d, history_max=20,
                           time_scalar=8640000, stage=1, base_method="BPR", category_col="i_category", lr_scale=0.1, margin=margin, lr=lr)

    def build():
        m = Chorus(args, corpus).to(cuda)
        with torch.no_grad():
            m.i_embeddings.weight.copy_(torch.from_numpy(g["I0"]))
            m.r_embeddings.weight.copy_(torch.from_numpy(g["Rel0"]))
        return m
    head, tail, rel = _dev(cuda, g["head_id"], g["tail_id"], g["relation_id"])
    feed = {"head_id": head, "tail_id": tail, "relation_id": rel, "batch_size": B, "phase": "train"}
    m = build()
    out = m(feed)
    assert_close(_np(out["prediction"]), g["pred"], what="stage-1 pred")
    loss = m.loss(out)
    loss.backward()
    assert_close(loss.item(), float(g["loss"]), what="stage-1 loss", **T2)
    assert_close(_np(m.i_embeddings.weight.grad), g["GI"], what="stage-1 GI", **T2)
    assert_close(_np(m.r_embeddings.weight.grad), g["GRel"], what="stage-1 GRel", **T2)
    assert m.u_embeddings.weight.grad is None and m.betas.weight.grad is None
    m2 = build()
    m2.optimizer = _runner(opt, lr, l2)._build_optimizer(m2)
    m2.train()
    for tag in ("1", "2"):
        m2.optimizer.zero_grad()
        m2.loss(m2(feed)).backward()
        m2.optimizer.step()
        extra = 1e-3 * lr * int(tag)
        assert_update_close(_np(m2.i_embeddings.weight), g["I0"], g["I" + tag], what="stage-1 I step " + tag, rtol=2e-5, extra_atol=extra, strict=True)
        assert_update_close(_np(m2.r_embeddings.weight), g["Rel0"], g["Rel" + tag], what="stage-1 Rel step " + tag, rtol=2e-5, extra_atol=extra, strict=True)
    m3 = build()
    loss3 = m3.hip_train_step(feed, opt, lr, l2)
    assert_close(loss3.item(), float(g["loss"]), what="stage-1 row-wise loss", **T2)
    # Rel is updated densely: its first row-wise step is torch.optim's
    assert_update_close(_np(m3.r_embeddings.weight), g["Rel0"], g["Rel1"], what="stage-1 row-wise Rel", rtol=2e-5, extra_atol=1e-3 * lr, strict=True)


# ---- stage 1: the argument mapping onto rc_cfkg_fwd_bwd --------------------------------------------------------------------------------

def test_stage1_feed_through_the_cfkg_step_against_float64(cuda):
    """Chorus's feed (head_id = (t, t, t', t), tail_id = (h, h, h, h')) through engine.chorus_kg_feed and rc_cfkg_fwd_bwd: the loss is
    the MarginRankingLoss of the reference's four columns, and the gradient rows are those of autograd on the dense node"""
    from rechorus_amd import engine, nn as hnn
    rng = np.random.default_rng(3)
    d, R, B, margin = 32, 3, 37, 1.0
    I = rng.normal(0, 0.5, (N_ITEMS, d)).astype(np.float32)
    Rel = rng.normal(0, 0.5, (R, d)).astype(np.float32)
    h, t, hn, tn = (rng.integers(1, N_ITEMS, B).astype(np.int64) for _ in range(4))
    r = rng.integers(1, R, B).astype(np.int64)
    head_id = np.stack([t, t, tn, t], axis=1)       # the reference's feed_dict['head_id'] = its tail_id array
    tail_id = np.stack([h, h, h, hn], axis=1)
    rel_id = np.stack([r] * 4, axis=1)
    E, Rl = I.astype(np.float64), Rel.astype(np.float64)
    pred = -((E[head_id] + Rl[rel_id] - E[tail_id]) ** 2).sum(-1)
    want_loss = np.maximum(0.0, -(pred[:, :2].reshape(-1) - pred[:, 2:].reshape(-1)) + margin).mean()
    dI, dR, dh, dt_, dr = _dev(cuda, I, Rel, head_id, tail_id, rel_id)
    got = engine.cfkg_scores(dI, dR, dh, dt_, dr)
    assert_close(_np(got), pred, what="stage-1 scores")
    ch, ct = engine.chorus_kg_feed(dh, dt_)
    p4, lv, _, _ = engine.cfkg_fwd_bwd(dI, dR, ch[:, 0].contiguous(), ct[:, 0].contiguous(), ch[:, 3].contiguous(),
                                       ct[:, 2].contiguous(), dr[:, 0].contiguous(), margin)
    assert_close(engine.reduce_sum(lv, 1.0 / B).item(), want_loss, what="stage-1 loss", **T2)
    assert_close(_np(p4)[:, [0, 1, 3, 2]], pred, what="stage-1 pred, columns 2 and 3 swapped back")
    # one SGD step of the trainer against autograd on the dense node with the reference's loss
    Ip, Rp = dI.clone().requires_grad_(True), dR.clone().requires_grad_(True)
    pr = hnn.cfkg_scores(Ip, Rp, dh, dt_, dr)
    loss = torch.nn.MarginRankingLoss(margin=margin)(pr[:, :2].flatten(), pr[:, 2:].flatten(), torch.ones(2 * B, device=cuda))
    loss.backward()
    tr = engine.CfkgTrainer(dI, dR, margin=margin, opt="SGD", lr=0.5, l2=0.0)
    loss_row = tr.step(ch, ct, dr)
    assert_close(loss_row.item(), loss.item(), what="stage-1 row-wise loss")
    assert_update_close(_np(dI), I, _np(Ip.detach() - 0.5 * Ip.grad), what="stage-1 I", rtol=2e-5, strict=True)
    assert_update_close(_np(dR), Rel, _np(Rp.detach() - 0.5 * Rp.grad), what="stage-1 Rel", rtol=2e-5, strict=True)


# ---- the model file through main.py on a synthetic KGReader corpus: stage 1 writes the checkpoint stage 2 loads ----------------------

@pytest.fixture(scope="module")
def kg_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("chorus_data"))
    make_kg_dataset(root, "synth_kg", n_users=40, n_items=30, per_user=7, n_neg=20, seed=11)
    return root


@pytest.mark.parametrize("engine_flag,base,test_all", [("dense", "BPR", "0"), ("rowwise", "GMF", "1"), ("rowwise", "BPR", "0")])
def test_cli_trains_stage_1_then_stage_2(engine_flag, base, test_all, kg_root, tmp_path, cuda, monkeypatch):
    import main
    from rechorus_amd import engine
    src = tmp_path / "src"
    src.mkdir()
    monkeypatch.chdir(src)          # the pre-trained file goes to ../model/Chorus/, as in the reference
    kg_steps, steps, fwd = [], [], []
    kg0, step0, fwd0 = engine.CfkgTrainer.step, engine.ChorusTrainer.step, engine.chorus_scores

    def scores(P, uid, iid, cid, intervals, kinds, gmf=False):
        fwd.append((iid.shape[1], tuple(kinds), gmf, int(cid.max())))
        return fwd0(P, uid, iid, cid, intervals, kinds, gmf)
    monkeypatch.setattr(engine.CfkgTrainer, "step", lambda self, *a, **k: kg_steps.append(1) or kg0(self, *a, **k))
    monkeypatch.setattr(engine.ChorusTrainer, "step", lambda self, *a, **k: steps.append(1) or step0(self, *a, **k))
    monkeypatch.setattr(engine, "chorus_scores", scores)
    common = ["--model_name", "Chorus", "--emb_size", "64", "--margin", "1", "--history_max", "20", "--time_scalar", "100000",
              "--dataset", "synth_kg", "--path", kg_root + "/", "--epoch", "1", "--num_workers", "0", "--regenerate", "1",
              "--engine", engine_flag, "--num_neg", "4", "--topk", "5,10", "--save_final_results", "0", "--base_method", base]
    with pytest.raises(ValueError, match="--stage 1"):        # stage 2 before stage 1: the pre-trained file is missing
        main.run(common + ["--stage", "2", "--log_file", str(tmp_path / "log" / "s0.txt")])
    log1 = str(tmp_path / "log" / "s1.txt")
    main.run(common + ["--stage", "1", "--lr", "5e-4", "--l2", "1e-5", "--batch_size", "32", "--early_stop", "0", "--test_all", "0",
                       "--log_file", log1])
    ckpt = tmp_path / "model" / "Chorus" / "KG__synth_kg__emb_size=64__margin=1.0.pt"
    assert ckpt.exists(), os.listdir(tmp_path)
    sd1 = torch.load(str(ckpt), map_location="cpu")
    assert list(sd1.keys()) == [chorus_np.STATE_KEYS[k] for k in PARAMS]
    m1 = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", open(log1).read())
    assert m1 and np.isfinite(float(m1.group(1)))
    assert bool(kg_steps) == (engine_flag == "rowwise") and not steps
    fwd.clear()
    log2 = str(tmp_path / "log" / "s2.txt")
    res = main.run(common + ["--stage", "2", "--lr", "1e-3", "--l2", "0", "--lr_scale", "0.1", "--batch_size", "64", "--test_all",
                             test_all, "--log_file", log2, "--model_path", str(tmp_path / "m2.pt")])
    text = open(log2).read()
    m2 = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", text)
    assert m2 and np.isfinite(float(m2.group(1))), text[-2000:]
    hr = float(re.search(r"HR@5:([0-9.]+)", res["test"]).group(1))
    assert 0.0 <= hr <= 1.0 and "NDCG@10" in res["test"]
    assert bool(steps) == (engine_flag == "rowwise")           # the row-wise trainer trained, or the autograd node did
    assert (5 in {f[0] for f in fwd}) == (engine_flag == "dense")
    assert ({f[0] for f in fwd} - {5}) == ({31} if test_all == "1" else {21})      # evaluation went through rc_chorus_scores
    assert {f[1] for f in fwd} == {(0, 1, 2)} and {f[2] for f in fwd} == {base == "GMF"}   # r_complement, r_substitute
    assert max(f[3] for f in fwd) >= 1                          # the category column was read
