"""GPU: the launch trace of the two Python trainers -- which entry point is called, in which order, on which of the trainer's streams.
_lib.call is wrapped (it still calls through) and every call is recorded as "entry point@ordinal of torch's current stream among the
trainer's streams" (0 = the caller's stream, 1 = trainer._side, 2 = NeumfTrainer._side2).  Each configuration's trace is compared with
a literal list.  The lists were produced by running this same test body on the commit BEFORE NeumfTrainer / SasrecTrainer were split
into named steps over one row-update marshaller; that change moved launches between functions and must not move one between streams,
reorder two, add or drop one.

NeuMF: d = 32, hidden 32, B = 64, C = 3, 50 users, 200 items, SGD, four steps; SASRec: d = 32, one block, 2 heads, history 8, B = 16,
C = 3, Adam, row-wise: 176 occurrences, so 20 items take the one-wave-per-row route (176 >= 8 * 20) and 400 items the sorted one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(cuda):
    from rechorus_amd import engine
    return engine


class Tracer:
    """_lib.call with a record of (entry point, stream ordinal) in front of it"""

    def __init__(self, lib, main):
        self.lib, self.inner, self.main, self.trainer, self.steps = lib, lib.call, main, None, []

    def __call__(self, name, *args):
        cur = torch.cuda.current_stream().cuda_stream
        streams = [self.main, self.trainer._side, getattr(self.trainer, "_side2", None)]     # (SasrecTrainer has one side stream)
        ordinal = [k for k, s in enumerate(streams) if s is not None and s.cuda_stream == cur]
        self.steps[-1].append("%s@%d" % (name, ordinal[0] if ordinal else -1))
        return self.inner(name, *args)

    def __enter__(self):
        self.lib.call = self
        return self

    def __exit__(self, *exc):
        self.lib.call = self.inner


def neumf_trace(eng, cuda, announce, overlap_min, fused):
    """four NeumfTrainer steps -> one list of "entry@stream" per step"""
    from rechorus_amd import _lib
    rng = np.random.default_rng(5)
    d, l1, B, C, n_users, n_items = 32, 32, 64, 3, 50, 200
    P = {"mf_u": (n_users, d), "mf_i": (n_items, d), "mlp_u": (n_users, d), "mlp_i": (n_items, d), "W1": (l1, 2 * d), "b1": (l1,),
         "w_out": (d + l1,)}
    P = {k: torch.from_numpy(rng.normal(0, 0.2, s).astype(np.float32)).to(cuda) for k, s in P.items()}
    batches = [(torch.from_numpy(rng.integers(0, n_users, size=B)).to(cuda), torch.from_numpy(rng.integers(0, n_items, size=(B, C))).to(cuda))
               for _ in range(5)]
    saved = eng._SAS_OVERLAP_MIN, eng._NEUMF_FUSED
    eng._SAS_OVERLAP_MIN, eng._NEUMF_FUSED = overlap_min, fused
    try:
        tr = eng.NeumfTrainer(P, opt="SGD", lr=0.05, l2=1e-4, rowwise=True)
        with Tracer(_lib, torch.cuda.current_stream()) as t:
            t.trainer = tr
            for k, (u, i) in enumerate(batches[:4]):
                t.steps.append([])
                nxt = batches[k + 1] if announce == "ahead" else batches[4] if (announce == "wrong" and k % 2 == 0) else None
                tr.step(u, i, next_batch=nxt)
        torch.cuda.synchronize()
    finally:
        eng._SAS_OVERLAP_MIN, eng._NEUMF_FUSED = saved
    return t.steps


def sasrec_trace(eng, cuda, n_items, overlap_min):
    """three SasrecTrainer steps -> one list of "entry@stream" per step"""
    from rechorus_amd import _lib
    from test_gpu_sasrec import _random_sasrec, to_dev
    rng = np.random.default_rng(7)
    d, n_heads, L, B, C = 32, 2, 8, 16, 3
    Pd = to_dev(_random_sasrec(rng, n_items, d, 1, L), 1, cuda)
    batches = []
    for _ in range(3):
        lengths = rng.integers(1, L + 1, size=B).astype(np.int64)
        hist = rng.integers(1, n_items, size=(B, L)).astype(np.int64) * (np.arange(L)[None, :] < lengths[:, None])
        iid = rng.integers(1, n_items, size=(B, C)).astype(np.int64)
        batches.append(tuple(torch.from_numpy(x).to(cuda) for x in (hist, lengths, iid)))
    saved = eng._SAS_OVERLAP_MIN
    eng._SAS_OVERLAP_MIN = overlap_min
    try:
        tr = eng.SasrecTrainer(Pd, n_heads, opt="Adam", lr=1e-3, l2=1e-5, rowwise=True)
        with Tracer(_lib, torch.cuda.current_stream()) as t:
            t.trainer = tr
            for b in batches:
                t.steps.append([])
                tr.step(*b)
        torch.cuda.synchronize()
    finally:
        eng._SAS_OVERLAP_MIN = saved
    return t.steps


BIG = 1 << 30      # an overlap threshold above every batch here: one stream

NEUMF_CONFIGS = {"two_streams": (0, True), "one_stream": (BIG, True), "three_kernel": (0, False)}
SASREC_CONFIGS = {"rows_one_stream": (20, BIG), "rows_two_streams": (20, 0), "sorted_one_stream": (400, BIG), "sorted_two_streams": (400, 0)}

# TRACES-BEGIN (one list per step; a step that repeats an earlier one of its configuration is written once)
NEUMF_TRACES = {}
_S = [["rc_bucket_plan@1", "rc_neumf_train_step@0", "rc_reduce_sum@1", "rc_neumf_mark_rows@1", "rc_bucket_plan@1", "rc_plan_update_pair@2",
       "rc_plan_update_pair@0", "rc_dense_update_multi@0"],
      ["rc_neumf_train_step@0", "rc_reduce_sum@1", "rc_neumf_unmark_rows@1", "rc_neumf_mark_rows@1", "rc_bucket_plan@1", "rc_plan_update_pair@2",
       "rc_plan_update_pair@0", "rc_dense_update_multi@0"]]
NEUMF_TRACES[('two_streams', 'ahead')] = [_S[0], _S[1], _S[1], _S[1]]
_S = [["rc_bucket_plan@1", "rc_neumf_train_step@0", "rc_reduce_sum@1", "rc_plan_update_pair@2", "rc_plan_update_pair@0", "rc_dense_update_multi@0"]]
NEUMF_TRACES[('two_streams', 'none')] = [_S[0], _S[0], _S[0], _S[0]]
_S = [["rc_bucket_plan@1", "rc_neumf_train_step@0", "rc_reduce_sum@1", "rc_neumf_mark_rows@1", "rc_bucket_plan@1", "rc_plan_update_pair@2",
       "rc_plan_update_pair@0", "rc_dense_update_multi@0"],
      ["rc_neumf_unmark_rows@1", "rc_bucket_plan@1", "rc_neumf_train_step@0", "rc_reduce_sum@1", "rc_plan_update_pair@2", "rc_plan_update_pair@0",
       "rc_dense_update_multi@0"]]
NEUMF_TRACES[('two_streams', 'wrong')] = [_S[0], _S[1], _S[0], _S[1]]
_S = [["rc_neumf_train_step@0", "rc_reduce_sum@0", "rc_bucket_plan@0", "rc_plan_update_pair@0", "rc_plan_update_pair@0", "rc_dense_update_multi@0"]]
NEUMF_TRACES[('one_stream', 'ahead')] = [_S[0], _S[0], _S[0], _S[0]]
_S = [["rc_neumf_train_step@0", "rc_reduce_sum@0", "rc_bucket_plan@0", "rc_plan_update_pair@0", "rc_plan_update_pair@0", "rc_dense_update_multi@0"]]
NEUMF_TRACES[('one_stream', 'none')] = [_S[0], _S[0], _S[0], _S[0]]
_S = [["rc_neumf_train_step@0", "rc_reduce_sum@0", "rc_bucket_plan@0", "rc_plan_update_pair@0", "rc_plan_update_pair@0", "rc_dense_update_multi@0"]]
NEUMF_TRACES[('one_stream', 'wrong')] = [_S[0], _S[0], _S[0], _S[0]]
_S = [["rc_bucket_plan@1", "rc_neumf_fwd@0", "rc_bpr_loss_fwd_bwd@0", "rc_reduce_sum@0", "rc_neumf_bwd@0", "rc_weighted_row_sum@0",
       "rc_weighted_row_sum@0", "rc_plan_update_pair@0", "rc_plan_update_pair@0", "rc_dense_update_multi@0"]]
NEUMF_TRACES[('three_kernel', 'ahead')] = [_S[0], _S[0], _S[0], _S[0]]
_S = [["rc_bucket_plan@1", "rc_neumf_fwd@0", "rc_bpr_loss_fwd_bwd@0", "rc_reduce_sum@0", "rc_neumf_bwd@0", "rc_weighted_row_sum@0",
       "rc_weighted_row_sum@0", "rc_plan_update_pair@0", "rc_plan_update_pair@0", "rc_dense_update_multi@0"]]
NEUMF_TRACES[('three_kernel', 'none')] = [_S[0], _S[0], _S[0], _S[0]]
_S = [["rc_bucket_plan@1", "rc_neumf_fwd@0", "rc_bpr_loss_fwd_bwd@0", "rc_reduce_sum@0", "rc_neumf_bwd@0", "rc_weighted_row_sum@0",
       "rc_weighted_row_sum@0", "rc_plan_update_pair@0", "rc_plan_update_pair@0", "rc_dense_update_multi@0"]]
NEUMF_TRACES[('three_kernel', 'wrong')] = [_S[0], _S[0], _S[0], _S[0]]
SASREC_TRACES = {}
_S = [["rc_sasrec_batch_fwd@0", "rc_bprmf_fwd_bwd@0", "rc_reduce_sum@0", "rc_sasrec_batch_bwd@0", "rc_rows_plan_build@0", "rc_rows_plan_update@0",
       "rc_sasrec_pos_grad@0", "rc_dense_update_multi@0"]]
SASREC_TRACES['rows_one_stream'] = [_S[0], _S[0], _S[0]]
_S = [["rc_sasrec_batch_fwd@0", "rc_rows_plan_build@1", "rc_bprmf_fwd_bwd@0", "rc_sasrec_batch_bwd_part@0", "rc_sasrec_batch_bwd_part@0",
       "rc_sasrec_pos_grad@0", "rc_dense_update_multi@0", "rc_reduce_sum@0", "rc_rows_plan_update@1"]]
SASREC_TRACES['rows_two_streams'] = [_S[0], _S[0], _S[0]]
_S = [["rc_sasrec_batch_fwd@0", "rc_bprmf_fwd_bwd@0", "rc_reduce_sum@0", "rc_sasrec_batch_bwd@0", "rc_sort_ids@0", "rc_segmented_update@0",
       "rc_sasrec_pos_grad@0", "rc_dense_update_multi@0"]]
SASREC_TRACES['sorted_one_stream'] = [_S[0], _S[0], _S[0]]
_S = [["rc_sasrec_batch_fwd@0", "rc_sort_ids@1", "rc_bprmf_fwd_bwd@0", "rc_sasrec_batch_bwd_part@0", "rc_sasrec_batch_bwd_part@0",
       "rc_sasrec_pos_grad@0", "rc_dense_update_multi@0", "rc_reduce_sum@0", "rc_segmented_update@1"]]
SASREC_TRACES['sorted_two_streams'] = [_S[0], _S[0], _S[0]]
# TRACES-END


@pytest.mark.parametrize("announce", ["ahead", "none", "wrong"])
@pytest.mark.parametrize("config", sorted(NEUMF_CONFIGS))
def test_neumf_trainer_launch_trace(config, announce, cuda, eng):
    overlap_min, fused = NEUMF_CONFIGS[config]
    steps = neumf_trace(eng, cuda, announce, overlap_min, fused)
    flat = [c.split("@")[0] for s in steps for c in s]
    assert ("rc_neumf_train_step" in flat) == fused and ("rc_neumf_fwd" in flat) == (not fused)      # the route that ran
    assert "rc_bucket_plan" in flat and "rc_sort_ids" not in flat
    assert ({c.split("@")[1] for s in steps for c in s} == {"0", "1", "2"}) == (config == "two_streams")
    for k, (got, want) in enumerate(zip(steps, NEUMF_TRACES[config, announce])):
        assert got == want, "step %d" % k
    assert len(steps) == len(NEUMF_TRACES[config, announce])


@pytest.mark.parametrize("config", sorted(SASREC_CONFIGS))
def test_sasrec_trainer_launch_trace(config, cuda, eng):
    n_items, overlap_min = SASREC_CONFIGS[config]
    steps = sasrec_trace(eng, cuda, n_items, overlap_min)
    flat = [c.split("@")[0] for s in steps for c in s]
    rows = config.startswith("rows")
    assert ("rc_rows_plan_build" in flat) == rows and ("rc_sort_ids" in flat) == (not rows)          # the route that ran
    assert ("rc_rows_plan_update" in flat) == rows and ("rc_segmented_update" in flat) == (not rows)
    assert ({c.split("@")[1] for s in steps for c in s} == {"0", "1"}) == config.endswith("two_streams")
    for k, (got, want) in enumerate(zip(steps, SASREC_TRACES[config])):
        assert got == want, "step %d" % k
    assert len(steps) == len(SASREC_TRACES[config])
