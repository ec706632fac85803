"""GPU: the fused BPRMF kernel's result does not depend on how a batch is cut into launches, bit for bit.  A wave reads its tuple's
ids once, coalesced (two registers per lane), and hands them to the lane-groups through an LDS strip (csrc/fused_body.hpp); the
persistent form of the kernel these tests were written for (a wave striding over the batch, the next tuple's ids fetched ahead) was
measured slower in the step and is not built, so W below is only the batch scale it would have had: the waves
the device holds of the d = 64, C = 100 SGD instantiation (768 workgroups of 4).

The same batch in chunks of 64 tuples is the reference.  The comparison is exact by construction: a singleton row is read by one
tuple only, and rows that occur several times are not written by this kernel.  `single` flags and the bitmap are those of the WHOLE
batch and inv_b is passed."""
import numpy as np
import pytest
import torch

import guarded as G
from conftest import assert_close, assert_update_close
from oracle import bprmf_oracle as O

pytestmark = pytest.mark.gpu

N_ITEMS, N_USERS, CHUNK, W = 20000, 500, 64, 3072
NAMES = ("pred", "loss_vec", "gpred", "ugrad", "I", "m", "v")


@pytest.fixture(scope="module")
def eng(cuda):
    from rechorus_amd import engine
    return engine


def _batch_sizes():
    """multiples of the resident waves and their neighbours: full and ragged last rounds of workgroups, odd batch sizes"""
    return {"W-1": W - 1, "W": W, "W+1": W + 1, "2W+5": 2 * W + 5, "3W+1": 3 * W + 1}


_problems = {}


def _problem(d, B, C, cuda):
    """(U, I, uid, iid, single, n_single) on the device, cached per shape and never written: a small hot set takes most positions
    (rows with many occurrences), every cold row is placed at most twice -- about a third of them once: the singletons"""
    key = (d, B, C)
    if key not in _problems:
        rng = np.random.default_rng(1000 * d + 10 * C + B % 7)
        n_hot = 2000
        U = rng.normal(0, 0.05, (N_USERS, d)).astype(np.float32)
        I = rng.normal(0, 0.05, (N_ITEMS, d)).astype(np.float32)
        uid = rng.integers(0, N_USERS, B).astype(np.int64)
        iid = rng.integers(0, n_hot, B * C).astype(np.int64)
        cold = rng.permutation(np.arange(n_hot, N_ITEMS))
        once, twice = cold[:6000], cold[6000:9000]
        pos = rng.permutation(B * C)[:min(B * C // 2, len(once) + 2 * len(twice))]
        ids = np.concatenate([once, twice, twice])[rng.permutation(len(once) + 2 * len(twice))][:len(pos)]
        iid[pos] = ids
        iid = iid.reshape(B, C)
        single = (np.bincount(iid.ravel(), minlength=N_ITEMS)[iid] == 1).astype(np.uint8)
        assert 0 < int(single.sum()) < B * C
        to = lambda a: torch.from_numpy(a).to(cuda)
        _problems[key] = (to(U), to(I), to(uid), to(iid), to(single), int(single.sum()))
    return _problems[key]


def _state(I, opt):
    m = torch.full_like(I, 0.25e-6) if opt in ("Adam", "Adagrad") else None
    v = torch.full_like(I, 1e-9) if opt == "Adam" else None
    return m, v


def _run(eng, prob, opt, how, a, b, state, B):
    """tuples [a, b) of the batch on the tables in `state` (I, m, v: updated in place) -> (pred, loss_vec, gpred, ugrad)"""
    U, _, uid, iid, single, _ = prob
    I, m, v = state[:3]
    if opt is None:
        return eng.bprmf_fwd_bwd(U, I, uid[a:b], iid[a:b], inv_b=1.0 / B, want_pred=True)
    h = eng.make_hyper(opt, lr=0.05, l2=1e-3, step=3)
    if how == "bitmap":
        return eng.bprmf_fwd_bwd_update(U, I, uid[a:b], iid[a:b], None, h, mI=m, vI=v, inv_b=1.0 / B, want_pred=True, multi=state[3])
    return eng.bprmf_fwd_bwd_update(U, I, uid[a:b], iid[a:b], single[a:b].reshape(-1), h, mI=m, vI=v, inv_b=1.0 / B, want_pred=True)


def _whole_and_chunked(eng, prob, opt, how, B):
    res = []
    for step in (B, CHUNK):
        I = prob[1].clone()
        state = (I, *_state(I, opt), eng.bucket_multi_bitmap(prob[3], N_ITEMS) if how == "bitmap" else None)
        outs = [_run(eng, prob, opt, how, a, min(a + step, B), state, B) for a in range(0, B, step)]
        res.append(tuple(torch.cat([o[k] for o in outs]) for k in range(4)) + state[:3])
    torch.cuda.synchronize()
    return res


def _assert_equal(whole, chunked, what):
    for nm, x, y in zip(NAMES, whole, chunked):
        if x is None:
            assert y is None
            continue
        if not torch.equal(x, y):
            diff = x != y
            raise AssertionError(f"{what}: {nm}: {int(diff.sum())} of {x.numel()} elements differ between the whole batch and chunks "
                                 f"of {CHUNK} tuples, max |diff| {(x - y).abs().max().item():.3e}, first at {torch.nonzero(diff)[0].tolist()}")


# d, C, which batch sizes
SHAPES = [(64, 100, ("W-1", "W", "W+1", "2W+5", "3W+1")),
          (64, 64, ("2W+5",)), (64, 65, ("2W+5",)), (64, 128, ("2W+5",)),     # C = 64: no second id register; 65: one candidate in it
          (32, 100, ("2W+5",)),
          (128, 100, ("2W+5",)),      # no register-resident kernel (d = 128: C <= 64): the update call refuses, fwd_bwd is generic
          (128, 64, ("2W+5",)),       # the widest d = 128 shape that has one
          (64, 2, ("2W+5",)), (64, 16, ("2W+5",))]                            # C = 2: two tuples per wave, ids loaded per lane-group
CASES = [(d, C, bn, opt, how) for d, C, bns in SHAPES for bn in bns
         for opt, how in ([("SGD", "bitmap"), ("SGD", "flags"), (None, "none")] +
                          ([(o, hw) for o in ("Adam", "Adagrad") for hw in ("bitmap", "flags")] if (d, C) == (64, 100) else []))]


@pytest.mark.parametrize("d,C,bn,opt,how", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_whole_batch_equals_chunks_of_64_bit_for_bit(d, C, bn, opt, how, cuda, eng):
    B = _batch_sizes()[bn]
    if not eng._lib.load().rc_bprmf_fused_supported(d, C) and opt is not None:
        with pytest.raises(eng._lib.RechorusHipError, match="no register-resident kernel"):
            _whole_and_chunked(eng, _problem(d, B, C, cuda), opt, how, B)
        return
    prob = _problem(d, B, C, cuda)
    whole, chunked = _whole_and_chunked(eng, prob, opt, how, B)
    _assert_equal(whole, chunked, f"d={d} C={C} B={B} {opt} {how}")
    if opt is not None:
        changed = int((whole[4] != prob[1]).any(dim=1).sum())
        assert 0 < changed <= prob[5], (changed, prob[5])      # singleton rows were updated, and nothing but singleton rows


@pytest.mark.parametrize("how", ["bitmap", "flags"])
def test_against_the_oracle(how, cuda, eng):
    """d = 64, C = 100, B = 2W + 5, SGD: every output and the updated singleton rows against oracle/bprmf_oracle.py"""
    d, C, opt = 64, 100, "SGD"
    B = 2 * W + 5
    prob = _problem(d, B, C, cuda)
    U, I0, uid, iid = (x.cpu().numpy() for x in prob[:4])
    Id = prob[1].clone()
    state = (Id, None, None, eng.bucket_multi_bitmap(prob[3], N_ITEMS) if how == "bitmap" else None)
    pred, loss_vec, gpred, ugrad = (x.cpu().numpy() for x in _run(eng, prob, opt, how, 0, B, state, B))
    want_pred = O.gather_dot(U, I0, uid, iid)
    assert_close(pred, want_pred, what="pred")
    rows, _, _, _ = O.bpr_loss_rows(want_pred)
    assert_close(loss_vec, rows, what="loss_vec")
    g = O.bpr_loss_grad(want_pred, 1.0 / B)
    assert_close(gpred, g, what="gpred")
    gu, gi = O.bprmf_row_grads(U, I0, uid, iid, g)
    assert_close(ugrad, gu, what="ugrad")
    single = prob[4].cpu().numpy().astype(bool)
    rows1 = iid[single]
    GI = np.zeros_like(I0)
    GI[rows1] = gi[single]
    Iref = I0.copy()
    O.opt_step_dense(Iref, GI, {}, opt, lr=0.05, l2=1e-3, step=3, rows=rows1)
    assert_update_close(Id.cpu().numpy(), I0, Iref, what="I (singleton rows)")


@pytest.mark.parametrize("opt,how", [("SGD", "bitmap"), ("Adam", "flags"), (None, "none")])
def test_ids_at_the_very_end_of_their_allocations(opt, how, cuda, eng):
    """B = 2W + 5 with uid and iid between guard bands: their last byte is followed by a band, and the clamped id loads of the last
    tuple (lanes past C) stay inside; the outputs equal the run with torch's slack behind the ids"""
    d, C = 64, 100
    B = 2 * W + 5
    prob = _problem(d, B, C, cuda)
    arena = G.Arena(cuda, 16 << 20)
    guarded_prob = (prob[0], prob[1], arena.put(prob[2], "uid"), arena.put(prob[3], "iid"), arena.put(prob[4], "single"), prob[5])
    res = []
    for p in (prob, guarded_prob):
        I = prob[1].clone()
        state = (I, *_state(I, opt), eng.bucket_multi_bitmap(prob[3], N_ITEMS) if how == "bitmap" else None)
        res.append(_run(eng, p, opt, how, 0, B, state, B) + state[:3])
    arena.check()
    _assert_equal(res[0], res[1], f"guarded ids, {opt} {how}")


@pytest.mark.parametrize("opt,how", [("SGD", "bitmap"), ("Adagrad", "flags")])
def test_two_runs_are_bit_identical(opt, how, cuda, eng):
    d, C = 64, 100
    B = 2 * W + 5
    prob = _problem(d, B, C, cuda)
    res = []
    for _ in range(2):
        I = prob[1].clone()
        state = (I, *_state(I, opt), eng.bucket_multi_bitmap(prob[3], N_ITEMS) if how == "bitmap" else None)
        res.append(_run(eng, prob, opt, how, 0, B, state, B) + state[:3])
    _assert_equal(res[0], res[1], f"two runs, {opt} {how}")
