"""GPU parity of the BPRMF step's medium rows: item rows with 5..32 and user rows with 3..32 occurrences are listed by the bucket
plan (csrc/bucket_plan.hip, PC_MED) and updated by lane-groups of their own at the head of the two update launches
(csrc/plan_update.hip, plan_medium_body).  Crafted batches hold rows at every occurrence count at which the update takes another
path: 1 (fused kernel / listed single), 2..4 (index phase), 5..32 (medium), 33.. (chunks of 256: one, exactly one, two, three).

Checks per optimizer: (1) the float oracle of oracle/bprmf_oracle.py under conftest.assert_update_close, (2) bit-equality with the
sort pipeline on EVERY row of both tables (on the commit before the medium list the two pipelines agreed bit for bit on every row of
these batches, rows above 32 occurrences included, so the row set is the whole table), (3) two runs give the same bits, (4) two
consecutive steps with look-ahead (ticket hit, both plan slots and so both medium lists used) equal the same steps without."""
import functools

import numpy as np
import pytest
import torch

from conftest import assert_update_close
from oracle import bprmf_oracle as O

pytestmark = pytest.mark.gpu

B, C, N_ITEMS, N_USERS = 512, 100, 60_000, 5_000
ITEM_COUNTS = (1, 2, 3, 4, 5, 6, 8, 9, 16, 17, 31, 32, 33, 255, 256, 257, 600)
USER_COUNTS = (1, 2, 3, 5, 32, 33, 300)
ONE_TUPLE_N, SPREAD_N = 7, 10    # the medium row inside tuple 3; the medium row over the first and the last tuple (5 + 5)

# (d, opt, lr, l2)
CASES = [(64, "SGD", 0.05, 0.0), (64, "SGD", 0.05, 1e-3), (64, "Adam", 1e-3, 1e-4), (64, "Adagrad", 0.01, 1e-4),
         (16, "SGD", 0.05, 1e-3)]
# (d = 128 has no register-resident fused kernel at C = 100, so that shape takes the sort pipeline; the d = 128 instantiations run in
#  test_gpu_plan.py::test_train_step_plan_pipeline_equals_sort_pipeline at C = 40)


def medium_rows(uid, iid):
    ci = np.unique(iid, return_counts=True)[1]
    cu = np.unique(uid, return_counts=True)[1]
    return int(((ci > 4) & (ci <= 32)).sum()), int(((cu > 2) & (cu <= 32)).sum())


def list_fits(ids, n_medium, singles_listed):
    """csrc/plan.hpp PlanMedList: the medium entries grow downward from the end of the side's row-record array, which holds one
    record per position; the row records (from the front) and the medium entries must fit it together.  A medium row has at least
    3 occurrences, so there can be no more than n / 3 of them."""
    cnt = np.unique(ids, return_counts=True)[1]
    records = len(cnt) if singles_listed else int((cnt > 1).sum())
    return records + n_medium <= ids.size and n_medium <= ids.size // 3


def crafted_batch(seed):
    """ids from a seeded permutation: one row per count of ITEM_COUNTS / USER_COUNTS, the two placed medium rows, the rest of the
    batch filled with single rows, pairs and one triple"""
    rng = np.random.default_rng(seed)
    item_ids = iter(rng.permutation(np.arange(1, N_ITEMS)))
    n = B * C
    one_tuple_id, spread_id = next(item_ids), next(item_ids)
    flat = np.zeros(n, dtype=np.int64)
    cols = rng.permutation(C)
    placed = [3 * C + c for c in cols[:ONE_TUPLE_N]] + [c for c in cols[:SPREAD_N // 2]] + \
             [(B - 1) * C + c for c in cols[SPREAD_N // 2:SPREAD_N]]
    flat[placed[:ONE_TUPLE_N]] = one_tuple_id
    flat[placed[ONE_TUPLE_N:]] = spread_id
    rest = []
    for c in ITEM_COUNTS:
        rest += [next(item_ids)] * c
    left = n - len(placed) - len(rest)
    singles = 40_000
    pairs = (left - singles - 3) // 2
    singles = left - 3 - 2 * pairs
    rest += [next(item_ids)] * 3
    for _ in range(pairs):
        rest += [next(item_ids)] * 2
    rest += [next(item_ids) for _ in range(singles)]
    rest = np.array(rest, dtype=np.int64)
    free = np.setdiff1d(np.arange(n), np.array(placed))
    assert len(rest) == len(free)
    flat[free] = rest[rng.permutation(len(rest))]
    iid = flat.reshape(B, C)

    user_ids = iter(rng.permutation(np.arange(1, N_USERS)))
    us = []
    for c in USER_COUNTS:
        us += [next(user_ids)] * c
    left = B - len(us)
    pairs = 18
    for _ in range(pairs):
        us += [next(user_ids)] * 2
    us += [next(user_ids) for _ in range(left - 2 * pairs)]
    uid = np.array(us, dtype=np.int64)[rng.permutation(B)]
    assert uid.shape == (B,) and B * C + B > 32768       # above the small-step limit
    cnt = dict(zip(*np.unique(iid, return_counts=True)))
    assert cnt[one_tuple_id] == ONE_TUPLE_N and (iid[3] == one_tuple_id).sum() == ONE_TUPLE_N
    assert cnt[spread_id] == SPREAD_N and (iid[0] == spread_id).sum() == 5 and (iid[B - 1] == spread_id).sum() == 5
    assert set(ITEM_COUNTS) <= set(cnt.values()) and set(USER_COUNTS) <= set(np.unique(uid, return_counts=True)[1])
    return uid, iid


def capacity_batch(seed):
    """every item row exactly 5 occurrences, every user row exactly 3: the medium list at its fullest"""
    rng = np.random.default_rng(seed)
    b = 510
    iid = np.repeat(rng.permutation(np.arange(1, N_ITEMS))[:b * C // 5], 5)
    uid = np.repeat(rng.permutation(np.arange(1, N_USERS))[:b // 3], 3)
    return uid[rng.permutation(b)], iid[rng.permutation(b * C)].reshape(b, C)


def _tables(d):
    rng = np.random.default_rng(1000 + d)
    return (rng.normal(0, 0.01, size=(N_USERS, d)).astype(np.float32), rng.normal(0, 0.01, size=(N_ITEMS, d)).astype(np.float32))


def _steps(d, opt, lr, l2, batches, pipeline, ahead):
    """the batches through a fresh trainer -> (U, I, losses) after EACH step, on the host"""
    from rechorus_amd import _lib, engine
    dev = torch.device("cuda:0")
    lib = _lib.load()
    assert lib.rc_bprmf_fused_supported(d, C) == 1 and lib.rc_bucket_plan_supported(B * C, B, N_ITEMS, N_USERS) == 1    # the plan pipeline
    U0, I0 = _tables(d)
    U, I = torch.from_numpy(U0).to(dev), torch.from_numpy(I0).to(dev)
    dev_batches = [(torch.from_numpy(u).to(dev), torch.from_numpy(i).to(dev)) for u, i in batches]
    prev = lib.rc_bprmf_step_pipeline(-1)
    out = []
    try:
        lib.rc_bprmf_step_pipeline(pipeline)
        tr = engine.BprmfTrainer(U, I, opt=opt, lr=lr, l2=l2)
        for k, (u, i) in enumerate(dev_batches):
            nxt = dev_batches[k + 1] if ahead and k + 1 < len(dev_batches) else None
            if ahead and k > 0:
                # the ticket hit: the library uses the plan prepared beside the previous step iff every field it compares
                # (train_step.hip, ticket_matches) agrees with this call -- all of them are visible from here
                t, ws = tr._ticket, tr._workspace(*i.shape)
                assert t.generation != 0 and t.generation == tr._generation_of(u, i), "the batch was not announced"
                assert (t.ws, t.slot, t.device, t.B, t.C, t.d, t.n_users, t.n_items) == \
                       (ws.data_ptr(), k % 2, dev.index or 0, i.shape[0], i.shape[1], d, N_USERS, N_ITEMS), "ticket of another call"
                assert t.flavour == (1 if opt == "SGD" else 2)      # bitmap + multi-occurrence rows / every row listed
            loss = tr.step(u, i, next_batch=nxt)
            if ahead and k > 0:
                assert tr._ticket.generation == (0 if nxt is None else tr._gen), "the ticket was not taken"
            torch.cuda.synchronize()
            out.append((U.cpu().numpy().copy(), I.cpu().numpy().copy(), float(loss.item())))
        del tr
    finally:
        lib.rc_bprmf_step_pipeline(prev)
    return out


@functools.lru_cache(maxsize=None)
def _runs(case):
    d, opt, lr, l2 = CASES[case]
    batches = [crafted_batch(7), crafted_batch(8)]
    plan = _steps(d, opt, lr, l2, batches, 0, False)
    again = _steps(d, opt, lr, l2, batches[:1], 0, False)
    sort = _steps(d, opt, lr, l2, batches[:1], 1, False)
    ahead = _steps(d, opt, lr, l2, batches, 0, True)
    return batches, plan, again, sort, ahead


def _diff(name, x, y):
    bad = np.flatnonzero((x != y).any(axis=1))
    return f"{name}: {len(bad)} rows differ (first {bad[:8]}), max |diff| {np.abs(x - y).max():.3e}"


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"d{c[0]}-{c[1]}-l2_{c[3]:g}" for c in CASES])
class TestMediumRows:
    def test_matches_the_oracle(self, case, cuda):
        d, opt, lr, l2 = CASES[case]
        batches, plan, *_ = _runs(case)
        uid, iid = batches[0]
        n_mi, n_mu = medium_rows(uid, iid)
        assert n_mi >= 10 and n_mu >= 3 and list_fits(iid, n_mi, True) and list_fits(uid, n_mu, True)
        U0, I0 = _tables(d)
        Un, In = U0.copy(), I0.copy()
        want, _ = O.bprmf_train_step(Un, In, O.new_state(Un, opt), O.new_state(In, opt), uid, iid, opt=opt, lr=lr, l2=l2, step=1,
                                     rowwise=True)
        U, I, loss = plan[0]
        assert abs(loss - float(want)) <= 1e-5 * abs(float(want))
        ex = 0.0 if opt == "SGD" else 1e-3 * lr
        assert_update_close(U, U0, Un, what="U", extra_atol=ex)
        assert_update_close(I, I0, In, what="I", extra_atol=ex)
        assert not np.array_equal(I, I0) and not np.array_equal(U, U0)

    def test_equals_the_sort_pipeline_bit_for_bit(self, case, cuda):
        _, plan, _, sort, _ = _runs(case)
        assert plan[0][2] == sort[0][2], "loss"
        assert np.array_equal(plan[0][0], sort[0][0]), _diff("U", plan[0][0], sort[0][0])
        assert np.array_equal(plan[0][1], sort[0][1]), _diff("I", plan[0][1], sort[0][1])

    def test_two_runs_give_identical_bits(self, case, cuda):
        _, plan, again, _, _ = _runs(case)
        assert plan[0][2] == again[0][2]
        assert np.array_equal(plan[0][0], again[0][0]) and np.array_equal(plan[0][1], again[0][1])

    def test_look_ahead_equals_no_look_ahead(self, case, cuda):
        _, plan, _, _, ahead = _runs(case)
        for k in range(2):
            assert plan[k][2] == ahead[k][2], f"loss of step {k}"
            assert np.array_equal(plan[k][0], ahead[k][0]), _diff(f"U after step {k}", plan[k][0], ahead[k][0])
            assert np.array_equal(plan[k][1], ahead[k][1]), _diff(f"I after step {k}", plan[k][1], ahead[k][1])


@pytest.mark.parametrize("opt,lr,l2", [("SGD", 0.05, 1e-3), ("Adam", 1e-3, 1e-4)])
def test_medium_list_at_capacity(opt, lr, l2, cuda):
    """every listed row is medium, so the list is at its fullest: the counts against the room the list has (list_fits) on the CPU,
    then the step against the oracle and the sort pipeline (an entry dropped for want of room, or written over a row record, would
    leave a row without its update)"""
    d = 64
    uid, iid = capacity_batch(11)
    b = len(uid)
    assert b * C + b > 32768
    n_mi, n_mu = medium_rows(uid, iid)
    assert (n_mi, n_mu) == (b * C // 5, b // 3) and len(np.unique(iid)) == n_mi and len(np.unique(uid)) == n_mu
    assert list_fits(iid, n_mi, True) and list_fits(uid, n_mu, True)      # (Adam lists every row; SGD lists fewer)
    plan = _steps(d, opt, lr, l2, [(uid, iid)], 0, False)[0]
    sort = _steps(d, opt, lr, l2, [(uid, iid)], 1, False)[0]
    U0, I0 = _tables(d)
    Un, In = U0.copy(), I0.copy()
    O.bprmf_train_step(Un, In, O.new_state(Un, opt), O.new_state(In, opt), uid, iid, opt=opt, lr=lr, l2=l2, step=1, rowwise=True)
    ex = 0.0 if opt == "SGD" else 1e-3 * lr
    assert_update_close(plan[0], U0, Un, what="U", extra_atol=ex)
    assert_update_close(plan[1], I0, In, what="I", extra_atol=ex)
    assert np.array_equal(plan[0], sort[0]), _diff("U", plan[0], sort[0])
    assert np.array_equal(plan[1], sort[1]), _diff("I", plan[1], sort[1])
