"""CPU: what the seven row-update wrappers of rechorus_amd/engine.py hand to the library -- segmented_update, segmented_update2
(one-wave-per-row branch), segmented_update_pair, RowsPlan.update, Plan.update, Plan.row_sums, Plan.update_pair -- with the library
calls recorded instead of made (the style of tests/test_fused_gather_layout.py: _lib.call, _lib.load, engine._stream, engine._ptr and
engine.workspace are recorders / stubs).  Every recorded call has exactly the argument count of its _lib.SIGNATURES entry, the slots
src2 / n_split / key_base / occ_base / flags / stride / base hold what the case asks for, and the whole tuple (tensors by name,
integers as they are) equals the literal written here.  The literals were recorded from the engine as it was BEFORE the wrappers
shared one marshaller (the three argument groups written out by hand at every site) and are unchanged since: the marshaller moved
the code, not an argument.  Also here: engine.new_opt_state, the one constructor of optimizer state."""
import ctypes as C

import pytest
import torch

from rechorus_amd import _lib, engine


class _FakeLib:
    """every *_workspace_bytes / *_bytes query answers 4096, every *_supported query 1"""

    def __getattr__(self, name):
        return lambda *a: 1 if name.endswith("_supported") else 4096


class _Counter:
    """a pre-zeroed ticket counter block of Plan.prezero_update_counters, without a device"""
    device = "dev"

    def __init__(self, t):
        self.t = t

    def data_ptr(self):
        return self.t.data_ptr()

    def record_stream(self, s):
        pass


class _Recorder:
    def __init__(self):
        self.calls, self.names, self.buffers = [], {}, {}

    def name(self, **tensors):
        for k, t in tensors.items():
            self.names[k] = t
        return tensors

    def workspace(self, nbytes, device, tag="default"):
        if tag not in self.buffers:
            self.buffers[tag] = self.names["ws:" + tag] = torch.zeros(8192, dtype=torch.uint8)
        self.calls.append(("workspace", int(nbytes), tag))
        return self.buffers[tag]

    def _addr(self, addr):
        for k, t in self.names.items():
            lo = t.data_ptr()
            if lo <= addr < lo + max(t.numel() * t.element_size(), 1):
                return k if addr == lo else "%s+%d" % (k, addr - lo)
        return "?"

    def token(self, a):
        if isinstance(a, torch.Tensor) or isinstance(a, _Counter):
            return self._addr(a.data_ptr())
        if isinstance(a, C.c_void_p):
            return None if not a.value else "&" + self._addr(a.value)
        if type(a).__name__ == "CArgObject":
            return "&hyper"
        return a

    def __call__(self, name, *args):
        assert len(args) == len(_lib.SIGNATURES[name][1]), (name, len(args))
        self.calls.append((name,) + tuple(self.token(a) for a in args))


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(_lib, "call", r)
    monkeypatch.setattr(_lib, "load", lambda: _FakeLib())
    monkeypatch.setattr(engine, "_stream", lambda: "stream")
    monkeypatch.setattr(engine, "_ptr", lambda t, *a, **k: t)
    monkeypatch.setattr(engine, "workspace", r.workspace)
    monkeypatch.setattr(engine, "_PLAN_CHECK", False)
    monkeypatch.setattr(engine, "_SEG_ROWS", True)
    monkeypatch.setattr(engine, "_SEG_ROWS_MIN_PER_ROW", 8)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: "stream")
    monkeypatch.setattr(engine, "_rows_plan_zeroed", set())
    return r


D, N_OCC, N_ROWS = 16, 40, 4        # 40 occurrences >= 8 * 4 rows: segmented_update2 takes the one-wave-per-row branch


def _tensors(rec, d=D, n=N_OCC, rows=N_ROWS):
    f = lambda *s: torch.zeros(s, dtype=torch.float32)
    return rec.name(W=f(rows, d), m=f(rows, d), v=f(rows, d), G=f(rows, d), keys=torch.zeros(n, dtype=torch.int32),
                    perm=torch.zeros(n, dtype=torch.int32), coef=f(n), src=f(n, d), src2=f(n, d), index=torch.zeros(n, dtype=torch.int64),
                    heads=torch.zeros(n, dtype=torch.int32), n_heads=torch.zeros(1, dtype=torch.int32),
                    step_dev=torch.zeros(1, dtype=torch.int64))


HYPER = engine.make_hyper("Adam")

# slot of every named argument in its entry point's argument list
SLOTS = {"rc_segmented_update": {"src2": 11, "n_split": 12, "key_base": 13, "occ_base": 14, "flags": 19},
         "rc_segmented_update_rows": {"src2": 12, "n_split": 13, "step_dev": 15},
         "rc_rows_plan_update": {"src2": 10, "n_split": 11, "step_dev": 13},
         "rc_plan_update": {"src2": 12, "n_split": 13},
         "rc_plan_row_sums": {"src2": 10, "n_split": 11},
         "rc_plan_update_pair": {"src_a": 11, "src_b": 12, "stride": 13, "base": 14, "counters": 16}}


def _last(rec, name, **slots):
    """the last recorded call of `name`, after checking the named slots"""
    call = [c for c in rec.calls if c[0] == name][-1]
    for k, want in slots.items():
        assert call[1 + SLOTS[name][k]] == want, (name, k, call[1 + SLOTS[name][k]], want)
    return call


def _ws_calls(rec):
    return [c for c in rec.calls if c[0] == "workspace"]


# ---- segmented_update -----------------------------------------------------------------------------------------------------------------

def test_segmented_update_one_source_rowwise_n_split_omitted(rec):
    t = _tensors(rec)
    engine.segmented_update(t["keys"], t["perm"], t["src"], HYPER, t["W"], t["m"], t["v"], coef=t["coef"], src_index=t["index"], div=3)
    call = _last(rec, "rc_segmented_update", src2=None, n_split=N_OCC, key_base=0, occ_base=0, flags=0)
    assert call == ("rc_segmented_update", "W", "m", "v", 16, "keys", "perm", 40, "coef", "src", "index", 3, None, 40, 0, 0, "&hyper",
                    None, None, None, 0, "&ws:seg", 8192, "stream")
    assert _ws_calls(rec) == [("workspace", 4096, "seg")]


def test_segmented_update_two_sources_dense_gradient_n_split_given(rec):
    t = _tensors(rec)
    engine.segmented_update(t["keys"], t["perm"], t["src"], dense_grad=t["G"], coef=t["coef"], div=3, src2=t["src2"], n_split=24)
    call = _last(rec, "rc_segmented_update", src2="src2", n_split=24, key_base=0, occ_base=0, flags=0)
    assert call == ("rc_segmented_update", None, None, None, 16, "keys", "perm", 40, "coef", "src", None, 3, "src2", 24, 0, 0, None,
                    "G", None, None, 0, "&ws:seg", 8192, "stream")


def test_segmented_update_head_list_skipping_singletons(rec):
    t = _tensors(rec)
    engine.segmented_update(t["keys"], t["perm"], t["src"], HYPER, t["W"], skip_singletons=True, heads=t["heads"], n_heads=t["n_heads"])
    call = _last(rec, "rc_segmented_update", src2=None, n_split=N_OCC, flags=_lib.RC_SEG_SKIP_SINGLETONS)
    assert call == ("rc_segmented_update", "W", None, None, 16, "keys", "perm", 40, None, "src", None, 1, None, 40, 0, 0, "&hyper",
                    None, "heads", "n_heads", _lib.RC_SEG_SKIP_SINGLETONS, "&ws:seg", 8192, "stream")


# ---- segmented_update2 ------------------------------------------------------------------------------------------------------------

def test_segmented_update2_rows_branch_rowwise_with_step_dev(rec):
    t = _tensors(rec)
    assert engine.seg_rows_route(N_OCC, N_ROWS, D)
    engine.segmented_update2(t["keys"], t["perm"], t["src"], t["src2"], 24, hyper=HYPER, W=t["W"], m=t["m"], v=t["v"], coef=t["coef"],
                             div=3, step_dev=t["step_dev"])
    call = _last(rec, "rc_segmented_update_rows", src2="src2", n_split=24, step_dev="step_dev")
    assert call == ("rc_segmented_update_rows", "W", "m", "v", 16, 4, "keys", "perm", 40, "coef", "src", None, 3, "src2", 24, "&hyper",
                    "step_dev", None, "&ws:seg_rows", 8192, "stream")
    assert _ws_calls(rec) == [("workspace", 4096, "seg_rows")]


def test_segmented_update2_rows_branch_dense_gradient(rec):
    t = _tensors(rec)
    engine.segmented_update2(t["keys"], t["perm"], t["src"], t["src2"], 24, coef=t["coef"], src_index=t["index"], div=3, dense_grad=t["G"])
    call = _last(rec, "rc_segmented_update_rows", src2="src2", n_split=24, step_dev=None)
    assert call == ("rc_segmented_update_rows", None, None, None, 16, 4, "keys", "perm", 40, "coef", "src", "index", 3, "src2", 24, None,
                    None, "G", "&ws:seg_rows", 8192, "stream")


def test_segmented_update2_head_list_branch_passes_both_sources_on(rec, monkeypatch):
    t = _tensors(rec)
    monkeypatch.setattr(engine, "_SEG_ROWS", False)
    engine.segmented_update2(t["keys"], t["perm"], t["src"], t["src2"], 24, hyper=HYPER, W=t["W"], m=t["m"], coef=t["coef"], div=3)
    call = _last(rec, "rc_segmented_update", src2="src2", n_split=24, key_base=0, occ_base=0, flags=0)
    assert call == ("rc_segmented_update", "W", "m", None, 16, "keys", "perm", 40, "coef", "src", None, 3, "src2", 24, 0, 0, "&hyper",
                    None, None, None, 0, "&ws:seg", 8192, "stream")
    with pytest.raises(RuntimeError, match="step_dev"):
        engine.segmented_update2(t["keys"], t["perm"], t["src"], t["src2"], 24, hyper=HYPER, W=t["W"], step_dev=t["step_dev"])


# ---- segmented_update_pair -----------------------------------------------------------------------------------------------------------

def test_segmented_update_pair_rowwise_and_dense_gradient(rec):
    t = _tensors(rec)
    f = lambda: torch.zeros((N_ROWS, D), dtype=torch.float32)
    t.update(rec.name(Wb=f(), mb=f(), vb=f(), Gb=f()))
    engine.segmented_update_pair(t["keys"], t["perm"], t["src"], t["src2"], hyper=HYPER, W=(t["W"], t["Wb"]), m=(t["m"], t["mb"]),
                                 v=(t["v"], t["vb"]), heads=t["heads"], n_heads=t["n_heads"])
    assert rec.calls[-1] == ("rc_segmented_update_pair", "W", "m", "v", "Wb", "mb", "vb", 16, "keys", "perm", 40, "src", "src2", "&hyper",
                             None, None, "heads", "n_heads", "&ws:seg", 8192, "stream")
    engine.segmented_update_pair(t["keys"], t["perm"], t["src"], t["src2"], dense_grad=(t["G"], t["Gb"]))
    assert rec.calls[-1] == ("rc_segmented_update_pair", None, None, None, None, None, None, 16, "keys", "perm", 40, "src", "src2", None,
                             "G", "Gb", None, None, "&ws:seg", 8192, "stream")
    assert _ws_calls(rec) == [("workspace", 4096, "seg")] * 2


# ---- RowsPlan.update ------------------------------------------------------------------------------------------------------------------

def _rows_plan(rec):
    ids_a, ids_b = torch.zeros((8, 3), dtype=torch.int64), torch.zeros((8, 2), dtype=torch.int64)      # 24 + 16 = 40 occurrences
    rec.name(ids_a=ids_a, ids_b=ids_b, lengths=torch.ones(8, dtype=torch.int64))
    return engine.RowsPlan(ids_a, ids_b, rec.names["lengths"], N_ROWS, D, tag="t_rows")


def test_rows_plan_update_rowwise_step_dev_and_dense_gradient(rec):
    t = _tensors(rec)
    plan = _rows_plan(rec)
    assert rec.calls[-1] == ("rc_rows_plan_build", "ids_a", 24, "ids_b", 16, "lengths", 2, 4, 16, "&ws:t_rows", 8192, "stream")
    plan.update(t["src"], hyper=HYPER, W=t["W"], m=t["m"], v=t["v"], coef=t["coef"], div=3, src2=t["src2"], step_dev=t["step_dev"])
    call = _last(rec, "rc_rows_plan_update", src2="src2", n_split=24, step_dev="step_dev")       # n_split = the plan's own n_a
    assert call == ("rc_rows_plan_update", "W", "m", "v", 16, 4, 40, "coef", "src", None, 3, "src2", 24, "&hyper", "step_dev", None,
                    "&ws:t_rows", 8192, "stream")
    plan.update(t["src"], coef=t["coef"], src_index=t["index"], div=3, src2=t["src2"], dense_grad=t["G"])
    call = _last(rec, "rc_rows_plan_update", src2="src2", n_split=24, step_dev=None)
    assert call == ("rc_rows_plan_update", None, None, None, 16, 4, 40, "coef", "src", "index", 3, "src2", 24, None, None, "G",
                    "&ws:t_rows", 8192, "stream")
    plan.update(t["src"], hyper=HYPER, W=t["W"])                                                  # one source
    call = _last(rec, "rc_rows_plan_update", src2=None, n_split=24, step_dev=None)
    assert call == ("rc_rows_plan_update", "W", None, None, 16, 4, 40, None, "src", None, 1, None, 24, "&hyper", None, None,
                    "&ws:t_rows", 8192, "stream")
    assert _ws_calls(rec) == [("workspace", 4096, "t_rows")]       # the plan's own buffer: update() asks for none


# ---- Plan ---------------------------------------------------------------------------------------------------------------------------------

N_A, N_B = 6, 4
# Plan(tag="t") lays its output out in workspace "t.out": rows_a at 0, rows_b at 256, occ at 512, the two counters at 768 / 772
ROWS = {"a": ("&ws:t.out", "&ws:t.out+768", 0), "b": ("&ws:t.out+256", "&ws:t.out+772", N_A)}


def _plan(rec):
    ids_a, ids_b = torch.zeros(N_A, dtype=torch.int64), torch.zeros(N_B, dtype=torch.int64)
    rec.name(ids_a=ids_a, ids_b=ids_b)
    plan = engine.Plan(ids_a, 100, ids_b, 50, tag="t")
    assert rec.calls[-1] == ("rc_bucket_plan", "ids_a", 6, 100, "ids_b", 4, 50, 1, None, "&ws:t.out", "&ws:t.out+768", "&ws:t.out+256",
                             "&ws:t.out+772", "&ws:t.out+512", "&ws:t.ws", 8192, "stream")
    assert plan.upd_counters is None
    del rec.calls[:]
    return plan


@pytest.mark.parametrize("side", ["a", "b"])
def test_plan_update_sources_and_the_n_split_default(rec, side):
    t = _tensors(rec, n=N_A + N_B)
    plan = _plan(rec)
    rows, cnt, _ = ROWS[side]
    head = ("rc_plan_update", "W", "m", "v", 16, rows, cnt, "&ws:t.out+512", 10)
    tail = ("&hyper", "&ws:t.upd", 8192, "stream")
    plan.update(side, t["W"], HYPER, m=t["m"], v=t["v"], coef=t["coef"], src=t["src"], src_index=t["index"], div=3)
    assert _last(rec, "rc_plan_update", src2=None, n_split=10) == head + ("coef", "src", "index", 3, None, 10) + tail    # one source: all of it
    plan.update(side, t["W"], HYPER, m=t["m"], v=t["v"], src2=t["src2"])
    assert _last(rec, "rc_plan_update", src2="src2", n_split=0) == head + (None, None, None, 1, "src2", 0) + tail        # only src2: from 0 on
    plan.update(side, t["W"], HYPER, m=t["m"], v=t["v"], coef=t["coef"], src=t["src"], div=3, src2=t["src2"], n_split=7)
    assert _last(rec, "rc_plan_update", src2="src2", n_split=7) == head + ("coef", "src", None, 3, "src2", 7) + tail
    assert _ws_calls(rec) == [("workspace", 4096, "t.upd")] * 3


@pytest.mark.parametrize("side", ["a", "b"])
def test_plan_row_sums_sources_and_the_n_split_default(rec, side):
    t = _tensors(rec, n=N_A + N_B)
    plan = _plan(rec)
    rows, cnt, _ = ROWS[side]
    head = ("rc_plan_row_sums", "G", 16, rows, cnt, "&ws:t.out+512", 10)
    tail = ("&ws:t.upd", 8192, "stream")
    assert plan.row_sums(side, t["G"], coef=t["coef"], src=t["src"], src_index=t["index"], div=3) is t["G"]
    assert _last(rec, "rc_plan_row_sums", src2=None, n_split=10) == head + ("coef", "src", "index", 3, None, 10) + tail
    plan.row_sums(side, t["G"], src2=t["src2"])
    assert _last(rec, "rc_plan_row_sums", src2="src2", n_split=0) == head + (None, None, None, 1, "src2", 0) + tail
    plan.row_sums(side, t["G"], coef=t["coef"], src=t["src"], div=3, src2=t["src2"], n_split=7)
    assert _last(rec, "rc_plan_row_sums", src2="src2", n_split=7) == head + ("coef", "src", None, 3, "src2", 7) + tail
    assert _ws_calls(rec) == [("workspace", 4096, "t.upd")] * 3


def test_plan_row_sums_of_an_empty_plan_launches_nothing(rec):
    empty = torch.zeros(0, dtype=torch.int64)
    rec.name(ids_a=empty)
    plan = engine.Plan(empty, 100, tag="t")
    del rec.calls[:]
    G = torch.zeros((4, D))
    assert plan.row_sums("a", G) is G and rec.calls == []


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("prezeroed", [False, True])
def test_plan_update_pair_block_or_two_sources_with_and_without_prezeroed_counters(rec, side, prezeroed):
    t = _tensors(rec, n=N_A + N_B)
    f = lambda *s: torch.zeros(s, dtype=torch.float32)
    t.update(rec.name(Wb=f(N_ROWS, D), mb=f(N_ROWS, D), vb=f(N_ROWS, D), block=f(N_A + N_B, 2 * D + 4), zeros=torch.zeros(16, dtype=torch.int32)))
    plan = _plan(rec)
    rows, cnt, base = ROWS[side]
    counters = None
    if prezeroed:
        plan.upd_counters = {"a": _Counter(t["zeros"][:8]), "b": _Counter(t["zeros"][8:])}
        counters = {"a": "&zeros", "b": "&zeros+32"}[side]
    head = ("rc_plan_update_pair", "W", "m", "v", "Wb", "mb", "vb", 16, rows, cnt, "&ws:t.out+512", 10)
    # two sources: stride 0
    plan.update_pair(side, t["W"], t["Wb"], t["src"], t["src2"], HYPER, ma=t["m"], va=t["v"], mb=t["mb"], vb=t["vb"], ws_tag=side)
    call = _last(rec, "rc_plan_update_pair", src_a="src", src_b="src2", stride=0, base=base, counters=counters)
    assert call == head + ("src", "src2", 0, base, "&hyper", counters, "&ws:t.upd" + side, 8192, "stream")
    if prezeroed:
        assert set(plan.upd_counters) == {"a", "b"} - {side}            # one use per side
    # one block of both gradients side by side, read where it lies: its row stride travels, the second pointer is null; the
    # counters of this side are spent, so the call zero-fills its own (null)
    plan.update_pair(side, t["W"], t["Wb"], t["block"], None, HYPER, ma=t["m"], va=t["v"], mb=t["mb"], vb=t["vb"])
    call = _last(rec, "rc_plan_update_pair", src_a="&block", src_b=None, stride=2 * D + 4, base=base, counters=None)
    assert call == head + ("&block", None, 36, base, "&hyper", None, "&ws:t.upd", 8192, "stream")
    assert _ws_calls(rec) == [("workspace", 4096, "t.upd" + side), ("workspace", 4096, "t.upd")]
    with pytest.raises(ValueError, match="block source"):
        plan.update_pair(side, t["W"], t["Wb"], t["block"][:, :D], None, HYPER)


def test_prezero_update_counters_hands_one_block_to_each_side(rec):
    plan = _plan(rec)
    plan.prezero_update_counters()
    z = plan.upd_counters
    assert set(z) == {"a", "b"} and z["a"].numel() == z["b"].numel() == 8 and z["a"].dtype == torch.int32
    assert z["b"].data_ptr() == z["a"].data_ptr() + 32 and not z["a"].any() and not z["b"].any()


# ---- optimizer state -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opt,keys", [("SGD", set()), ("Adagrad", {"m"}), ("Adam", {"m", "v"}), ("Adadelta", set())])
def test_new_opt_state(opt, keys):
    """m for Adam and Adagrad, v for Adam, each zeros like the tensor; SGD keeps nothing, and Adadelta (built for dense steps only:
    no row-wise trainer runs it) nothing either"""
    t = torch.full((5, 3), 2.0, dtype=torch.float32)
    st = engine.new_opt_state(t, opt)
    assert set(st) == keys
    for k, z in st.items():
        assert z.shape == t.shape and z.dtype == t.dtype and z.device == t.device and not z.any()
        assert z.data_ptr() != t.data_ptr()
    if len(st) == 2:
        assert st["m"].data_ptr() != st["v"].data_ptr()
