"""CPU: the guard-band harness (tests/guarded.py) detects what it claims, the allocator proxy serves rechorus_amd.engine, and every
`int rc_*(` entry point of include/rechorus_hip.h is either guarded (tests/guard_table.py GUARDED, with cases in
tests/test_gpu_guard_bands.py) or exempt with a reason -- a new entry point cannot land without a guard case."""
import os
import re

import pytest
import torch

from conftest import ROOT
import guard_table as T
import guarded as G

HEADER = os.path.join(ROOT, "include", "rechorus_hip.h")
CPU = torch.device("cpu")


@pytest.fixture()
def arena():
    return G.Arena(CPU, 1 << 20, guard=4096)


def _poke(arena, offset, value=0x5A):
    """flip one arena byte (offset relative to the arena's base) to a value that is in neither band pattern"""
    arena.buf[offset] = value


# ---- the harness detects what it claims ---------------------------------------------------------------------------------------

def test_untouched_arena_is_clean(arena):
    arena.take((3, 5), torch.float32, "out")
    arena.put(torch.arange(6, dtype=torch.int64), "ids")
    arena.put(torch.ones(4, 2), "table", kind="table")
    arena.check(tables={"table": []})


def test_one_byte_past_the_end_is_reported_with_name_and_offset(arena):
    arena.take((2, 2), torch.float32, "first")
    v = arena.take((3, 5), torch.float32, "victim")
    arena.take((4,), torch.int32, "third")
    view = arena.view_of(v)
    assert view.name == "victim" and view.nbytes == 60
    _poke(arena, view.end)
    with pytest.raises(G.GuardError, match=r"after 'victim'.*1 bytes, bytes \+0 \.\. \+0 past the tensor's end"):
        arena.check()
    arena.reset()
    v = arena.take((3, 5), torch.float32, "victim")
    view = arena.view_of(v)
    _poke(arena, view.end + 37)
    _poke(arena, view.end + 4095)
    with pytest.raises(G.GuardError, match=r"after 'victim'.*2 bytes, bytes \+37 \.\. \+4095 past"):
        arena.check()


def test_one_byte_before_the_start_is_reported(arena):
    v = arena.take((3, 5), torch.int64, "victim")
    view = arena.view_of(v)
    _poke(arena, view.start - 1)
    with pytest.raises(G.GuardError, match=r"before 'victim'.*bytes -1 \.\. -1 before the tensor's start \(-121 \.\. -121 from its end\)"):
        arena.check()


def test_a_band_byte_rewritten_with_its_own_pattern_is_not_a_finding_but_any_other_value_is(arena):
    v = arena.take((5,), torch.float32, "f")
    view = arena.view_of(v)
    _poke(arena, view.end, 0xAD)         # the float band's first byte IS 0xAD
    arena.check()
    _poke(arena, view.end, 0x00)
    with pytest.raises(G.GuardError):
        arena.check()


def test_an_input_altered_in_place_is_reported(arena):
    x = arena.put(torch.arange(12, dtype=torch.float32).view(3, 4), "x")
    ids = arena.put(torch.arange(5), "ids")
    arena.check()
    x[2, 1] = 100.0
    with pytest.raises(G.GuardError, match="input 'x' was altered in place"):
        arena.check()
    with pytest.raises(G.GuardError, match="input 'x'"):
        arena.check(inputs=[x])
    arena.check(inputs=[ids])            # only the listed inputs are held to their copies


def test_bit_identity_is_bitwise(arena):
    x = arena.put(torch.zeros(4), "x")
    x[1] = -0.0                          # equal as a float, another bit pattern
    with pytest.raises(G.GuardError, match="input 'x'"):
        arena.check()


def test_a_changed_row_outside_the_declared_row_set_is_reported(arena):
    W = arena.put(torch.ones(10, 3), "W", kind="table")
    W[4] += 1
    W[7] += 1
    arena.check(tables={"W": [4, 7]})
    arena.check(tables={"W": torch.tensor([7, 4, 4])})
    with pytest.raises(G.GuardError, match=r"table 'W': 1 rows outside the declared row set changed, first row 7, last row 7"):
        arena.check(tables={"W": [4]})
    with pytest.raises(G.GuardError, match="must name the rows"):
        arena.check()
    with pytest.raises(G.GuardError, match="does not hold"):
        arena.check(tables={"W": [4, 7], "V": []})


def test_band_patterns_read_as_nan_and_as_zero(arena):
    f = arena.take((7, 5), torch.float32, "f")
    i = arena.take((3,), torch.int64, "i")
    b = arena.take((5,), torch.int32, "offsets")
    vf, vi, vb = arena.view_of(f), arena.view_of(i), arena.view_of(b)
    g = arena.guard
    after_f = arena.buf[vf.end:vf.end + g].view(torch.float32)
    before_f = arena.buf[vf.start - g:vf.start].view(torch.float32)
    assert torch.isnan(after_f).all() and torch.isnan(before_f).all()
    assert (after_f.view(torch.int32) == G.FLOAT_WORD).all()
    for v in (vi, vb):
        lo = (v.end + 7) // 8 * 8        # an int64 view needs 8-byte alignment; the bytes skipped are checked as bytes below
        assert (arena.buf[v.end:v.end + g] == 0).all() and (arena.buf[v.start - g:v.start] == 0).all()
        assert (arena.buf[lo:lo + g - 8].view(torch.int64) == 0).all()
        assert (arena.buf[lo:lo + g - 8].view(torch.int32) == 0).all()
    # a float over-read that is KEPT is NaN in the value: one element past a row-major [7, 5] output
    flat = arena.buf[vf.start:vf.end + 4].view(torch.float32)
    assert flat.numel() == 36 and torch.isnan(flat[35])


def test_scratch_bands_are_small_indices_and_show_a_zero_fill_that_runs_too_far(arena):
    """beside uint8 buffers (workspaces, flags) the band is the 64-bit word 1: a zero fill past the declared size is a finding --
    it would vanish in a zero band -- and an index read from the band is 0 or 1"""
    ws = arena.take((1000,), torch.uint8, "ws")
    flags = arena.take((5,), torch.uint8, "flags")
    g = arena.guard
    for t in (ws, flags):
        v = arena.view_of(t)
        lo = (arena.base + v.end + 7) // 8 * 8 - arena.base
        assert (arena.buf[lo:lo + g - 8].view(torch.int64) == 1).all()
        w32 = arena.buf[lo:lo + g - 8].view(torch.int32)
        assert (w32[0::2] == 1).all() and (w32[1::2] == 0).all()
        assert int(arena.buf[v.end:v.end + g].max()) == 1 and int(arena.buf[v.start - g:v.start].max()) == 1
    arena.check()
    ws.zero_()
    arena.check()
    v = arena.view_of(ws)
    arena.buf[v.start:v.end + 24].zero_()              # a counter block zero-filled 24 bytes too far
    with pytest.raises(G.GuardError, match=r"after 'ws' \(out, 1000 bytes\) is dirty: 3 bytes, bytes \+0 \.\. \+16 past the tensor's end"):
        arena.check()
    assert G.band_of(torch.uint8) == "scratch" and G.band_of(torch.int32) == "int" and G.band_of(torch.float64) == "float"


def test_a_7_by_5_float_view_ends_exactly_at_the_first_guard_byte(arena):
    f = arena.take((7, 5), torch.float32, "f")
    v = arena.view_of(f)
    assert v.nbytes == 140 and v.end == v.start + 140 and v.end % 16 == 12
    assert f.data_ptr() + 140 == arena.base + v.end
    assert arena.buf[v.end:v.end + 4].tolist() == [0xAD, 0xDE, 0xC0, 0x7F]        # the very next byte is guard
    f.fill_(1.0)
    arena.check()
    assert f.is_contiguous() and f.shape == (7, 5)


def test_views_start_256_byte_aligned_with_full_bands_on_both_sides(arena):
    prev_end = 0
    for k, (shape, dtype) in enumerate([((7, 5), torch.float32), ((1,), torch.uint8), ((3,), torch.int64), ((1000,), torch.uint8),
                                        ((0, 4), torch.float32), ((), torch.float32)]):
        t = arena.take(shape, dtype, f"t{k}")
        v = arena.view_of(t) if t.numel() else arena.views[-1]
        assert (arena.base + v.start) % 256 == 0 and (t.numel() == 0 or t.data_ptr() == arena.base + v.start)
        assert v.start - v.lead >= arena.guard and v.trail_end - v.end == arena.guard
        assert v.lead >= prev_end                      # bands are not shared between neighbours of different patterns
        prev_end = v.trail_end
        assert arena.contains(t)
    assert not arena.contains(torch.zeros(4))
    arena.check()


def test_arena_reports_exhaustion():
    small = G.Arena(CPU, 16384, guard=4096)
    small.take((1000,), torch.float32, "fits")
    with pytest.raises(MemoryError):
        small.take((4000,), torch.float32, "does not")


# ---- the proxy serves rechorus_amd.engine ----------------------------------------------------------------------------------------

def test_workspace_is_served_at_exactly_the_requested_size(arena, monkeypatch):
    from rechorus_amd import engine
    cache = engine._ws_cache
    big = None
    with G.guarded(engine, arena, monkeypatch) as served:
        assert engine.torch is not torch and engine._ws_cache is not cache
        big = engine.workspace(1000, CPU, "t")
        assert big.numel() == 1000 and big.dtype == torch.uint8 and arena.contains(big) and big.data_ptr() % 256 == 0
        assert engine.workspace(1000, CPU, "t") is big         # the cache still works inside one block
        assert engine.workspace(10, CPU, "small").numel() == 256
        less = engine.workspace(600, CPU, "t")                 # ... but never hands out more than the call declares
        assert less is not big and less.numel() == 600 and arena.contains(less)
        assert served.count == 3 and served.scratch_bytes == 1856
        assert [w[:2] for w in served.workspaces] == [("t", 1000), ("t", 1000), ("small", 10), ("t", 600)]
    assert engine.torch is torch and engine._ws_cache is cache and ("cpu", "t") not in cache
    assert engine.workspace.__module__ == "rechorus_amd.engine"
    arena.reset()
    with G.guarded(engine, arena, monkeypatch) as served:
        again = engine.workspace(600, CPU, "t")                # a second, smaller request does not get the first one back
        assert again.numel() == 600 and served.count == 1
        again.fill_(7)
        arena.check()
        arena.buf[arena.view_of(again).end] = 0x5A             # what a kernel using 601 bytes of a 600-byte declaration does
        with pytest.raises(G.GuardError, match=r"engine#0:empty\(600,\):uint8.*\+0 \.\. \+0 past"):
            arena.check()
    assert engine.torch is torch and engine._ws_cache is cache


def test_proxy_serves_both_calling_conventions_and_passes_the_rest_through(arena):
    p = G._TorchProxy(arena)
    a = p.empty((3, 5), dtype=torch.float32, device=CPU)
    b = p.empty(7, dtype=torch.int32, device=CPU)
    c = p.zeros(2, 3, dtype=torch.int64, device="cpu")
    d = p.full((4,), -1, dtype=torch.int32, device=CPU)
    e = p.ones((2, 2), device=CPU)
    f = p.empty_like(a)
    g = p.zeros_like(b)
    h = p.empty(a.shape[:-1] + (4,), dtype=torch.float32, device=CPU)       # torch.Size arithmetic
    for t, shape, dtype in ((a, (3, 5), torch.float32), (b, (7,), torch.int32), (c, (2, 3), torch.int64), (d, (4,), torch.int32),
                            (e, (2, 2), torch.float32), (f, (3, 5), torch.float32), (g, (7,), torch.int32), (h, (3, 4), torch.float32)):
        assert tuple(t.shape) == shape and t.dtype == dtype and arena.contains(t) and t.is_contiguous()
    assert (c == 0).all() and (d == -1).all() and (e == 1).all() and (g == 0).all()
    assert len(p.served) == 8
    # device-less allocations pass through; attributes are the real module's
    outside = p.empty(5)
    assert not arena.contains(outside) and len(p.served) == 8
    assert p.float32 is torch.float32 and p.Tensor is torch.Tensor and p.arange(3).tolist() == [0, 1, 2]
    # what the arena cannot give raises instead of escaping it
    with pytest.raises(G.GuardError):
        p.empty((2, 2), dtype=torch.float32, device=CPU, pin_memory=True)
    with pytest.raises(G.GuardError):
        p.full_like
    with pytest.raises(G.GuardError):
        p.full((2,), 1.0, device=CPU)
    arena.check()


def test_engine_allocates_only_through_served_names():
    """the proxy can only see module-level torch.<name>(...) calls: engine.py must not allocate device memory another way"""
    text = open(os.path.join(ROOT, "rechorus_amd", "engine.py")).read()
    # (the one new_full((), ...) is a zero-dimensional constant of SasrecTrainer's tensor glue, no buffer a kernel writes)
    assert not re.search(r"\.new_(empty|zeros|ones|full|tensor)\((?!\(\), )", text)
    used = set(re.findall(r"\btorch\.(empty\w*|zeros\w*|ones\w*|full\w*|rand\w*)\(", text))
    assert used <= set(G._SERVED), sorted(used - set(G._SERVED))


# ---- coverage --------------------------------------------------------------------------------------------------------------------

def header_entry_points():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return set(re.findall(r"\bint\s+(rc_\w+)\s*\(", text))


def test_every_header_entry_point_is_guarded_or_exempt():
    declared = header_entry_points()
    assert len(declared) >= 120, len(declared)
    both = sorted(set(T.GUARDED) & set(T.EXEMPT))
    assert not both, f"both guarded and exempt: {both}"
    missing = sorted(declared - set(T.GUARDED) - set(T.EXEMPT))
    assert not missing, f"entry points without a guard case or an exemption in tests/guard_table.py: {missing}"
    stale = sorted((set(T.GUARDED) | set(T.EXEMPT)) - declared)
    assert not stale, f"tests/guard_table.py names entry points the header no longer declares: {stale}"
    for name, why in T.EXEMPT.items():
        assert isinstance(why, str) and len(why.strip()) >= 10 and "\n" not in why, name


def test_every_guarded_wrapper_exists_and_has_cases():
    from rechorus_amd import engine
    cases = open(os.path.join(ROOT, "tests", "test_gpu_guard_bands.py")).read()
    src = open(os.path.join(ROOT, "rechorus_amd", "engine.py")).read()
    for name, entry in T.GUARDED.items():
        obj = engine
        for part in entry["wrapper"].split("."):
            assert hasattr(obj, part), (name, entry["wrapper"])
            obj = getattr(obj, part)
        assert callable(obj), (name, entry["wrapper"])
        assert entry["cases"], name
        assert isinstance(entry.get("deterministic", True), bool)
        for fn in entry["cases"]:
            assert re.search(r"^def %s\(" % re.escape(fn), cases, flags=re.M), (name, fn)
        # the wrapper really reaches the entry point
        assert re.search(r'"%s"' % re.escape(name), src), name


def test_every_case_is_listed_in_the_table_and_every_listed_case_reaches_its_entry_point():
    import test_gpu_guard_bands as GB
    fns = {p.values[0] for p in GB.CASES}
    by_name = {f.__name__: f for f in fns}
    assert len(GB.CASES) >= 150 and len({p.id for p in GB.CASES}) == len(GB.CASES)
    for f in fns:
        for e in f.entries:
            assert e in T.GUARDED and f.__name__ in T.GUARDED[e]["cases"], (f.__name__, e)
    for e, entry in T.GUARDED.items():
        for name in entry["cases"]:
            assert name in by_name and e in by_name[name].entries, (e, name)
