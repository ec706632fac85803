"""GPU: the SGD row write-back stores a row only if the update changed a bit of it (csrc/opt_math.hpp, store_row4_changed: a
bitwise vote of the row's lane-group), in the fused BPRMF kernel's singleton loop and in every row body of csrc/plan_update.hip.
Skipping the store of a bit-identical row is exact, so the tables after a step must be what they were before this change, bit for
bit -- rows whose update is below half an ulp (unchanged, not written) and rows that move (written whole) side by side.

The expected tables do not come from the code under test.  gpred and ugrad are taken from rc_bprmf_fwd_bwd, the no-update entry
point; an occurrence's gradient row is gpred[b, c] * U[uid[b]] in float32 (users: ugrad[b]); a row's occurrences are summed in
float32 in the order the update kernels fix (ascending batch position up to 32 occurrences; above that in
chunks of 256, sixteen strided partial sums and a binary tree per chunk, the chunks the same way); and
w' = fma(-lr, fma(l2, w, g), w) with both fmas rounded ONCE to float32 (fma32 below, checked against fractions.Fraction without a
GPU).  The comparison is np.array_equal on the uint32 views.  Loss and gpred are held to oracle/bprmf_oracle.py as in the other
BPRMF tests.

Each route has learning rates at which the CPU expectation leaves between 25 % and 75 % of the touched item rows unchanged (asserted
on the expectation before the GPU result is looked at), and the two ends: lr = 0 (no row changes) and lr = 1 (every row does)."""
import fractions
import functools

import numpy as np
import pytest
import torch

from conftest import assert_close
from oracle import bprmf_oracle as O

F32 = np.float32
GPB = 16            # lane-groups per workgroup of the chunk kernels at d = 64 (256 threads / 16 lanes per row)
LONG, CHUNK = 32, 256   # csrc/plan.hpp: kPlanLongSeg, kPlanChunk


# ---- float32 arithmetic with one rounding ------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """round_to_float32(a * b + c) with a single rounding, element-wise on float32 arrays.  a * b is exact in float64 (48 bits);
    p + c is rounded to 53 bits with its error e recovered exactly (two-sum).  Rounding that sum to float32 is a second rounding,
    which differs from the single one only where the float64 sum lies exactly half-way between two float32 values while the exact
    sum does not (a float32 midpoint is a float64 number, so rounding to float64 cannot cross one): there e says on which side
    the exact value lies."""
    a, b, c = (np.asarray(x, dtype=F32).astype(np.float64) for x in np.broadcast_arrays(a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(F32)
    r64 = r.astype(np.float64)
    dist = s - r64
    toward = np.where(dist > 0, F32(np.inf), F32(-np.inf)).astype(F32)
    nb = np.nextafter(r, toward)
    tie = (dist != 0) & (np.abs(dist) * 2 == np.abs(nb.astype(np.float64) - r64))
    # a tie was resolved to even by the cast; the exact value is beyond the midpoint iff e points away from r
    flip = tie & (e != 0) & (np.sign(e) == np.sign(dist))
    return np.where(flip, nb, r).astype(F32)


def fma32_exact(a, b, c):
    """the same by rational arithmetic, one element (finite inputs)"""
    x = fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c))
    if x == 0:
        return fma32(a, b, c)[()]      # the sign of a zero sum is IEEE's, not a rational's
    lo = F32(float(x))                 # float(Fraction) rounds once to float64: a starting point only
    cands = [np.nextafter(lo, F32(-np.inf)), lo, np.nextafter(lo, F32(np.inf))]
    best = min(cands, key=lambda v: (abs(fractions.Fraction(float(v)) - x), int(v.view(np.uint32)) & 1))
    return best


def sgd32(w, g, lr, l2):
    """opt_elem<MODE_SGD>: g = fmaf(l2, w, g); w = fmaf(-lr, g, w)"""
    g = fma32(F32(l2), w, g)
    return fma32(F32(-lr), g, w)


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def test_fma32_rounds_once():
    """the helper the expectations stand on, against rational arithmetic: random operands, operands built so that the float64 sum is
    an exact float32 midpoint with a remainder on either side, signed zeros and denormals"""
    rng = np.random.default_rng(5)
    a = rng.normal(0, 1, 400).astype(F32)
    b = rng.normal(0, 1e-3, 400).astype(F32)
    c = rng.normal(0, 1, 400).astype(F32)
    # c with an odd last mantissa bit plus a product just below half an ulp of c: the product is half_ulp * (1 - 2^-46), the
    # float64 sum rounds up to the exact float32 midpoint, and a second rounding ties to even, away from c
    k = np.arange(100) % 50 - 10
    sign = np.where(np.arange(100) < 50, 1.0, -1.0)
    c2 = (sign * 2.0 ** k * (1 + (2 * rng.integers(0, 1 << 22, 100) + 1) * 2.0 ** -23)).astype(F32)
    a2 = (sign * 2.0 ** (k - 24) * (1 + 2.0 ** -23)).astype(F32)
    b2 = np.full(100, 1 - 2.0 ** -23, dtype=F32)
    den = np.array([1e-40, -3e-42, 1.4e-45, 0.0, -0.0], dtype=F32)
    A = np.concatenate([a, a2, np.array([-0.0, -0.0, 1e-3, 0.0, -0.0], dtype=F32)])
    Bv = np.concatenate([b, b2, np.array([2.5e-7, -2.5e-7, 1e-40, 3.0, 0.0], dtype=F32)])
    Cv = np.concatenate([c, c2, den])
    got = fma32(A, Bv, Cv)
    want = np.array([fma32_exact(x, y, z) for x, y, z in zip(A, Bv, Cv)], dtype=F32)
    assert np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))
    twice = (A.astype(np.float64) * Bv.astype(np.float64) + Cv.astype(np.float64)).astype(F32)
    assert (bits(twice) != bits(got)).sum() >= 90        # the midpoint cases do tell one rounding from two
    assert bits(fma32(F32(-0.0), F32(-1e-7), F32(-0.0)))[()] == 0 and bits(fma32(F32(-0.0), F32(1e-7), F32(-0.0)))[()] == 0x80000000


# ---- a row's occurrences summed in the kernels' order ---------------------------------------------------------------------------------

def _tree16(parts):
    """plan_tree_sum: part[g] += part[g + off], off = 8, 4, 2, 1"""
    parts = [p.copy() for p in parts]
    off = GPB // 2
    while off >= 1:
        for g in range(off):
            parts[g] = parts[g] + parts[g + off]
        off //= 2
    return parts[0]


def _strided_tree(vecs):
    """lane-group g adds elements g, g + 16, ... in ascending order to a zero, then the tree"""
    d = vecs.shape[1]
    parts = []
    for g in range(GPB):
        acc = np.zeros(d, dtype=F32)
        for v in vecs[g::GPB]:
            acc = acc + v
        parts.append(acc)
    return _tree16(parts)


def row_sum(vecs):
    """vecs [n, d] float32: the gradient rows of a row's occurrences in ascending batch position"""
    n = len(vecs)
    if n <= LONG:
        acc = vecs[0].copy()
        for v in vecs[1:]:
            acc = acc + v
        return acc
    partial = np.stack([_strided_tree(vecs[k:k + CHUNK]) for k in range(0, n, CHUNK)])
    return _strided_tree(partial)


def apply_rows(W, ids, grads, lr, l2):
    """W[row] <- sgd(W[row], sum of the row's gradient rows) for every row in ids; returns the distinct rows and their counts"""
    order = np.argsort(ids, kind="stable")
    rows, start, cnt = np.unique(ids[order], return_index=True, return_counts=True)
    summed = np.empty((len(rows), W.shape[1]), dtype=F32)
    one = cnt == 1
    summed[one] = grads[order[start[one]]]
    for k in np.flatnonzero(~one):
        summed[k] = row_sum(grads[order[start[k]:start[k] + cnt[k]]])
    W[rows] = sgd32(W[rows], summed, lr, l2)
    return rows, cnt


def unchanged_fraction(W, W0, rows):
    return float((bits(W[rows]) == bits(W0[rows])).all(axis=1).mean())


def _diff(name, got, want, W0):
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    if len(bad) == 0:
        return ""
    r = bad[0]
    moved = "changes" if (bits(want[r]) != bits(W0[r])).any() else "stays as it was"
    return (f"{name}: {len(bad)} rows differ from the expectation (first {bad[:8].tolist()}); row {r} {moved} in the expectation, "
            f"{int((bits(got[r]) != bits(want[r])).sum())} of its elements differ")


@pytest.fixture(scope="module")
def eng(cuda):
    from rechorus_amd import engine
    return engine


def _check_loss_side(U0, I0, uid, iid, gpred, inv_b):
    want_pred = O.gather_dot(U0, I0, uid, iid)
    assert_close(gpred, O.bpr_loss_grad(want_pred, inv_b), what="gpred")
    return float(O.bpr_loss_rows(want_pred)[0].sum(dtype=np.float64) * inv_b)


# ---- route 1: the fused kernel alone, one wave = one tuple --------------------------------------------------------------------------

N_FUSED_ITEMS, N_FUSED_USERS, B_FUSED = 4096, 64, 7


@functools.lru_cache(maxsize=None)
def _fused_problem(d, C):
    """tables and a batch in which every item row occurs once (B = 7: the last wave of the grid holds a clamped tuple where a wave
    holds more than one)"""
    rng = np.random.default_rng(100 * d + C)
    U = rng.normal(0, 0.01, (N_FUSED_USERS, d)).astype(F32)
    I = rng.normal(0, 0.01, (N_FUSED_ITEMS, d)).astype(F32)
    uid = rng.integers(0, N_FUSED_USERS, B_FUSED).astype(np.int64)
    iid = rng.permutation(N_FUSED_ITEMS)[:B_FUSED * C].reshape(B_FUSED, C).astype(np.int64)
    return U, I, uid, iid


def _place_rows(I, U, uid, iid):
    """hand-placed rows in tuple 2 (d = 64, C = 100; candidate c is slot c // 4 of lane-group c % 4):
       c = 6   all but one element are large (their update is far below half an ulp), one element of lane 5 is tiny and moves;
       c = 7   a row of -0.0 (at lr = 0 the elements with g * u < 0 become +0.0: equal as floats, other bits);
       c = 10  a row of denormals;
       c = 1, 5, 9, ..., 37  neighbouring slots of lane-group 1, alternately tiny rows (move) and large rows (stay)."""
    I = I.copy()
    t = 2
    I[iid[t, 6]] = F32(64.0)
    I[iid[t, 6], 4 * 5 + 2] = F32(1e-30)
    I[iid[t, 7]] = F32(-0.0)
    I[iid[t, 10]] = (np.arange(1, 65) * 1.4e-45).astype(F32) * np.where(np.arange(64) % 3 == 0, -1, 1).astype(F32)
    for k, c in enumerate(range(1, 40, 4)):
        I[iid[t, c]] = F32(1e-20) * (1 + np.arange(64, dtype=F32)) if k % 2 == 0 else F32(16.0) + np.arange(64, dtype=F32)
    return I


def _run_fused(eng, cuda, U0, I0, uid, iid, lr, l2, how):
    to = lambda a: torch.from_numpy(a).to(cuda)
    U, I, uidd, iidd = to(U0), to(I0), to(uid), to(iid)
    B, C = iid.shape
    _, _, gpred, _ = eng.bprmf_fwd_bwd(U, I, uidd, iidd, inv_b=1.0 / B, want_pred=False)
    gpred = gpred.cpu().numpy().reshape(B, C)
    h = eng.make_hyper("SGD", lr=lr, l2=l2, step=1)
    if how == "bitmap":
        out = eng.bprmf_fwd_bwd_update(U, I, uidd, iidd, None, h, inv_b=1.0 / B, multi=eng.bucket_multi_bitmap(iidd, I0.shape[0]))
    else:
        out = eng.bprmf_fwd_bwd_update(U, I, uidd, iidd, torch.ones(B * C, dtype=torch.uint8, device=cuda), h, inv_b=1.0 / B)
    torch.cuda.synchronize()
    return gpred, out[2].cpu().numpy().reshape(B, C), U.cpu().numpy(), I.cpu().numpy()


def _expect_fused(U0, I0, uid, iid, gpred, lr, l2):
    C = iid.shape[1]
    grads = gpred.reshape(-1, 1).astype(F32) * np.repeat(U0[uid], C, axis=0)
    I = I0.copy()
    rows, cnt = apply_rows(I, iid.ravel(), grads, lr, l2)
    assert (cnt == 1).all()
    return I, rows


# (d, C, lr, l2, how, unchanged rows in the expectation: None = not asserted, else (low, high))
FUSED_CASES = [
    (64, 100, 0.0, 0.0, "bitmap", (1.0, 1.0)), (64, 100, 1.0, 0.0, "bitmap", (0.0, 0.0)),
    (64, 100, 1e-6, 0.0, "bitmap", (0.25, 0.75)), (64, 100, 1e-6, 0.0, "flags", (0.25, 0.75)),
    (64, 100, 1e-6, 1e-4, "bitmap", (0.25, 0.75)), (64, 100, 3e-7, 0.0, "bitmap", None),
    (64, 5, 0.0, 0.0, "bitmap", (1.0, 1.0)), (64, 5, 1.0, 0.0, "bitmap", (0.0, 0.0)), (64, 5, 3e-8, 0.0, "bitmap", (0.25, 0.75)),
    (32, 100, 0.0, 0.0, "bitmap", (1.0, 1.0)), (32, 100, 1.0, 0.0, "bitmap", (0.0, 0.0)), (32, 100, 1.5e-6, 0.0, "bitmap", (0.25, 0.75)),
    (128, 64, 0.0, 0.0, "bitmap", (1.0, 1.0)), (128, 64, 1.0, 0.0, "bitmap", (0.0, 0.0)), (128, 64, 3e-7, 0.0, "bitmap", (0.25, 0.75)),
    (128, 64, 3e-7, 1e-4, "flags", None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("d,C,lr,l2,how,frac", FUSED_CASES, ids=[f"d{c[0]}-C{c[1]}-lr{c[2]:g}-l2_{c[3]:g}-{c[4]}" for c in FUSED_CASES])
def test_fused_kernel_singleton_rows(d, C, lr, l2, how, frac, cuda, eng):
    U0, I0, uid, iid = _fused_problem(d, C)
    gpred0, gpred, U, I = _run_fused(eng, cuda, U0, I0, uid, iid, lr, l2, how)
    _check_loss_side(U0, I0, uid, iid, gpred0, 1.0 / B_FUSED)
    want, rows = _expect_fused(U0, I0, uid, iid, gpred0, lr, l2)
    f = unchanged_fraction(want, I0, rows)
    print(f"d={d} C={C} lr={lr:g} l2={l2:g}: {f:.3f} of {len(rows)} touched rows unchanged in the expectation")
    if frac is not None:
        assert frac[0] <= f <= frac[1], f
    assert np.array_equal(bits(gpred), bits(gpred0)), "gpred of the update call differs from the no-update call's"
    assert np.array_equal(bits(U), bits(U0)), "the fused kernel does not write U"
    assert np.array_equal(bits(I), bits(want)), _diff("I", I, want, I0)


@pytest.mark.gpu
@pytest.mark.parametrize("lr", [0.0, 1e-9, 1.0])
def test_hand_placed_rows(lr, cuda, eng):
    d, C = 64, 100
    U0, I0, uid, iid = _fused_problem(d, C)
    I0 = _place_rows(I0, U0, uid, iid)
    gpred0, gpred, U, I = _run_fused(eng, cuda, U0, I0, uid, iid, lr, 0.0, "bitmap")
    want, rows = _expect_fused(U0, I0, uid, iid, gpred0, lr, 0.0)
    t = 2
    changed = lambda c: bits(want[iid[t, c]]) != bits(I0[iid[t, c]])
    if lr == 1e-9:
        assert changed(6).sum() == 1 and changed(6)[4 * 5 + 2], "one element of one lane moves"
        assert changed(10).all(), "every denormal moves"
        alt = [bool(changed(c).any()) for c in range(1, 40, 4)]
        assert alt == [k % 2 == 0 for k in range(10)], alt
        assert 0.5 < unchanged_fraction(want, I0, rows) < 1.0
    if lr == 0.0:
        neg0 = changed(7)
        assert 0 < neg0.sum() < d and np.array_equal(want[iid[t, 7]], I0[iid[t, 7]]), "-0.0 -> +0.0 where g * u < 0: equal floats, other bits"
        assert not changed(10).any() and not changed(6).any()
    assert np.array_equal(bits(gpred), bits(gpred0))
    assert np.array_equal(bits(I), bits(want)), _diff("I", I, want, I0)


# ---- route 2: the whole step through the bucket plan (B (C + 2) > 32,768) ---------------------------------------------------------------

B_PLAN, C_PLAN, D_PLAN, N_PLAN_USERS = 512, 100, 64, 3000


@functools.lru_cache(maxsize=None)
def _plan_problem(n_items):
    """n_items = 200,000: uniform ids, mostly single rows.  2,000: a skewed draw, rows from one occurrence to several hundred.
    Users: a few rows with 2, 3..32 and more than 32 occurrences."""
    rng = np.random.default_rng(n_items)
    U = rng.normal(0, 0.01, (N_PLAN_USERS, D_PLAN)).astype(F32)
    I = rng.normal(0, 0.01, (n_items, D_PLAN)).astype(F32)
    n = B_PLAN * C_PLAN
    if n_items >= 100_000:
        iid = rng.integers(0, n_items, n)
    else:
        p = 1.0 / (1.0 + np.arange(n_items)) ** 0.9
        iid = rng.permutation(n_items)[rng.choice(n_items, n, p=p / p.sum())]
    iid = iid.reshape(B_PLAN, C_PLAN).astype(np.int64)
    us = list(rng.permutation(N_PLAN_USERS))
    uid = [us.pop()] * 40 + [us.pop()] * 33 + [us.pop()] * 32 + [us.pop()] * 7 + [us.pop()] * 3
    for _ in range(20):
        uid += [us.pop()] * 2
    uid += [us.pop() for _ in range(B_PLAN - len(uid))]
    uid = np.array(uid, dtype=np.int64)[rng.permutation(B_PLAN)]
    return U, I, uid, iid


@functools.lru_cache(maxsize=None)
def _plan_gradients(n_items):
    """(gpred, ugrad) of rc_bprmf_fwd_bwd on the pre-step tables, on the host"""
    from rechorus_amd import engine
    dev = torch.device("cuda:0")
    U0, I0, uid, iid = _plan_problem(n_items)
    to = lambda a: torch.from_numpy(a).to(dev)
    _, _, gpred, ugrad = engine.bprmf_fwd_bwd(to(U0), to(I0), to(uid), to(iid), inv_b=1.0 / B_PLAN, want_pred=False)
    torch.cuda.synchronize()
    return gpred.cpu().numpy().reshape(B_PLAN, C_PLAN), ugrad.cpu().numpy()


def _step(n_items, opt, lr, l2, pipeline=0):
    from rechorus_amd import _lib, engine
    dev = torch.device("cuda:0")
    lib = _lib.load()
    assert lib.rc_bprmf_fused_supported(D_PLAN, C_PLAN) == 1
    assert lib.rc_bucket_plan_supported(B_PLAN * C_PLAN, B_PLAN, n_items, N_PLAN_USERS) == 1 and B_PLAN * (C_PLAN + 2) > 32768
    U0, I0, uid, iid = _plan_problem(n_items)
    U, I = torch.from_numpy(U0).to(dev), torch.from_numpy(I0).to(dev)
    prev = lib.rc_bprmf_step_pipeline(-1)
    try:
        lib.rc_bprmf_step_pipeline(pipeline)
        tr = engine.BprmfTrainer(U, I, opt=opt, lr=lr, l2=l2)
        loss = tr.step(torch.from_numpy(uid).to(dev), torch.from_numpy(iid).to(dev))
        torch.cuda.synchronize()
        out = (U.cpu().numpy(), I.cpu().numpy(), float(loss.item()),
               *(None if x is None else x.cpu().numpy() for x in (tr.mU, tr.vU, tr.mI, tr.vI)))
        del tr
    finally:
        lib.rc_bprmf_step_pipeline(prev)
    return out


# (items, lr, l2, unchanged item rows in the expectation)
PLAN_CASES = [
    (200_000, 0.0, 0.0, (1.0, 1.0)), (200_000, 1.0, 0.0, (0.0, 0.0)),
    (200_000, 1e-4, 0.0, (0.25, 0.75)), (200_000, 5e-5, 0.0, (0.25, 0.75)), (200_000, 1e-4, 1e-4, None),
    (2_000, 0.0, 0.0, (1.0, 1.0)), (2_000, 1.0, 0.0, (0.0, 0.0)),
    (2_000, 2e-5, 0.0, (0.25, 0.75)), (2_000, 1e-5, 1e-4, None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n_items,lr,l2,frac", PLAN_CASES, ids=[f"items{c[0]}-lr{c[1]:g}-l2_{c[2]:g}" for c in PLAN_CASES])
def test_step_through_the_bucket_plan(n_items, lr, l2, frac, cuda):
    U0, I0, uid, iid = _plan_problem(n_items)
    cnt_i = np.unique(iid, return_counts=True)[1]
    cnt_u = np.unique(uid, return_counts=True)[1]
    if n_items >= 100_000:
        assert (cnt_i == 1).mean() > 0.7
    else:
        assert min(((cnt_i >= 2) & (cnt_i <= 4)).sum(), ((cnt_i >= 5) & (cnt_i <= 32)).sum(), ((cnt_i > 32) & (cnt_i <= 256)).sum(),
                   (cnt_i > 256).sum(), (cnt_i == 1).sum()) >= 1
    assert {1, 2, 3, 7, 32, 33, 40} <= set(cnt_u.tolist())
    gpred, ugrad = _plan_gradients(n_items)
    want_loss = _check_loss_side(U0, I0, uid, iid, gpred, 1.0 / B_PLAN)
    grads = gpred.reshape(-1, 1).astype(F32) * np.repeat(U0[uid], C_PLAN, axis=0)
    Iw, Uw = I0.copy(), U0.copy()
    rows_i, _ = apply_rows(Iw, iid.ravel(), grads, lr, l2)
    rows_u, _ = apply_rows(Uw, uid, ugrad, lr, l2)
    f = unchanged_fraction(Iw, I0, rows_i)
    print(f"items={n_items} lr={lr:g} l2={l2:g}: {f:.3f} of {len(rows_i)} touched item rows, "
          f"{unchanged_fraction(Uw, U0, rows_u):.3f} of {len(rows_u)} user rows unchanged in the expectation")
    if frac is not None:
        assert frac[0] <= f <= frac[1], f
    U, I, loss = _step(n_items, "SGD", lr, l2)[:3]
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)
    assert np.array_equal(bits(I), bits(Iw)), _diff("I", I, Iw, I0)
    assert np.array_equal(bits(U), bits(Uw)), _diff("U", U, Uw, U0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_items", [200_000, 2_000])
@pytest.mark.parametrize("opt,lr", [("Adam", 1e-3), ("Adagrad", 0.01)])
def test_stateful_optimizers_equal_the_sort_pipeline(opt, lr, n_items, cuda):
    """the stateful paths store unconditionally as before: tables and optimizer state of the plan pipeline equal the sort pipeline's
    (csrc/seg_update.hip, which this change does not touch), bit for bit"""
    plan = _step(n_items, opt, lr, 1e-4, pipeline=0)
    sort = _step(n_items, opt, lr, 1e-4, pipeline=1)
    assert plan[2] == sort[2], "loss"
    for name, x, y in zip(("U", "I", "loss", "mU", "vU", "mI", "vI"), plan, sort):
        if name == "loss" or x is None:
            assert name == "loss" or y is None
            continue
        assert np.array_equal(bits(x), bits(y)), f"{name}: {int((bits(x) != bits(y)).any(axis=1).sum())} rows differ"
    U0, I0, _, _ = _plan_problem(n_items)
    assert not np.array_equal(plan[0], U0) and not np.array_equal(plan[1], I0)
