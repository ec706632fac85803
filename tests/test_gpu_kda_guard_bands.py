"""GPU: the KDA engine wrappers run once on torch's allocator and once between guard bands -- inputs, outputs and the workspace
served from tests/guarded.py's arena and allocator stand-in, every view ending on the first band byte, the workspace exactly the
bytes rc_kda_aggregate_bwd_workspace_bytes declares.  The second run must leave every band and every input bit-identical, return
finite values and return the first run's bits.  The protocol is tests/test_gpu_guard_bands.py's, as
tests/test_gpu_din_guard_bands.py applies it; the cases live in this module's OWN list, the table is tests/kda_guard_table.py."""
import numpy as np
import pytest
import torch

import guard_table as T
import guarded as G
import kda_data as KD
import kda_guard_table as CT
from test_gpu_guard_bands import Placer, _flat, _n

pytestmark = pytest.mark.gpu

ARENA_BYTES = 64 << 20
f32 = np.float32
CASES = []
REACHED = {}        # case function -> [cases run, entry points called between the bands]


def case(entries, params, allocates=True):
    """register a case function for every parameter tuple; entries: the C entry points it reaches"""
    def deco(fn):
        fn.entries, fn.allocates = tuple(entries), allocates
        for p in params:
            p = p if isinstance(p, tuple) else (p,)
            CASES.append(pytest.param(fn, p, id=fn.__name__[5:] + "-" + "-".join(str(x).replace(" ", "") for x in p)))
        return fn
    return deco


@pytest.fixture(scope="module")
def arena(cuda):
    a = G.Arena(cuda, ARENA_BYTES)
    yield a
    del a


@pytest.fixture(scope="module")
def eng(cuda):
    from rechorus_amd import engine
    return engine


@pytest.mark.parametrize("fn,params", CASES)
def test_kda_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
    what = f"{fn.__name__[5:]} {params}"
    try:
        plain = fn(Placer(eng, cuda), *params)
        torch.cuda.synchronize()
        arena.reset()
        c = Placer(eng, cuda, arena)
        called = []
        real_call = eng._lib.call
        with G.guarded(eng, arena, monkeypatch) as served:
            monkeypatch.setattr(eng._lib, "call", lambda name, *a: called.append(name) or real_call(name, *a))
            got = fn(c, *params)
            torch.cuda.synchronize()
        monkeypatch.setattr(eng._lib, "call", real_call)
    except RuntimeError as e:
        if "illegal memory access" in str(e) or "HIP error" in str(e) or "hipError" in str(e):
            # the device is in an unknown state: nothing more is started on it in this session
            pytest.exit(f"GPU fault in {what}: {str(e).splitlines()[0]}", returncode=3)
        raise
    stray = sorted(set(called) - set(T.GUARDED) - set(CT.GUARDED))
    assert not stray, f"{what}: reached entry points that neither guard table lists as guarded: {stray}"
    REACHED.setdefault(fn.__name__, [0, set()])
    REACHED[fn.__name__][0] += 1
    REACHED[fn.__name__][1].update(called)
    arena.check(tables=c.tables)        # bands and inputs
    for tag, asked, buf in served.workspaces:
        assert arena.contains(buf), f"{what}: workspace '{tag}' escaped the arena"
        assert buf.numel() == max(asked, 256), f"{what}: workspace '{tag}' has {buf.numel()} bytes for a declaration of {asked}"
    asked = [n for tag, n, _ in served.workspaces if tag == "kda_bwd"]
    B, Cn, L, R, V, F, _ = params
    assert asked and all(n == eng._lib.load().rc_kda_aggregate_bwd_workspace_bytes(B, R, V, F) for n in asked)
    assert (served.count > 0) == fn.allocates, what
    a, b = _flat(plain), _flat(got)
    assert [p for p, _ in a] == [p for p, _ in b] and len(b) > 0, what
    for (path, x), (_, y) in zip(a, b):
        assert torch.is_tensor(y) and arena.contains(y), f"{what}: result '{path}' escaped the arena"
        assert bool(torch.isfinite(y).all()), f"{what}: result '{path}' is not finite"
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {path}"
        assert torch.equal(G._bytes(x.contiguous()), G._bytes(y.contiguous())), \
            f"{what}: '{path}' differs between the plain and the guarded run"


def test_every_entry_point_a_case_claims_was_called_between_the_bands():
    """runs after the cases (file order): a case function that ran all its cases called every entry point it lists"""
    n_cases = {}
    for p in CASES:
        n_cases[p.values[0].__name__] = n_cases.get(p.values[0].__name__, 0) + 1
    fns = {p.values[0].__name__: p.values[0] for p in CASES}
    for name, (ran, called) in REACHED.items():
        if ran == n_cases[name]:
            missing = sorted(set(fns[name].entries) - called)
            assert not missing, f"{name} never called {missing}"


# ---- cases -----------------------------------------------------------------------------------------------------------------------

# (B, C, L, R, V, F, include_val).  Every bound of the envelope on both sides that exists: V at all four widths; L = 1 and 64; R = 1
# and 8; F = 2 and 129; C below, at and past the backward's candidate tile (256 / (V / 4) lane-groups, at most 32) and a C * R that
# is no multiple of the forward's lane-groups; B = 1, B past one row per workgroup slice of the workspace (1,024 slices), a row
# without a valid position (a read past seq or a write past context would land on a band); with and without the value rows
@case(("rc_kda_aggregate_fwd", "rc_kda_aggregate_bwd"),
      [(1, 1, 1, 1, 16, 2, 1), (2, 2, 64, 8, 128, 129, 1), (3, 5, 7, 3, 32, 5, 0), (5, 100, 20, 5, 64, 33, 1), (2, 33, 3, 2, 16, 2, 1),
       (4, 8, 9, 8, 128, 17, 0), (3, 9, 64, 1, 128, 129, 1), (1030, 2, 3, 2, 16, 3, 1), (7, 16, 20, 3, 64, 33, 0), (2, 17, 5, 7, 64, 9, 1),
       (3, 32, 2, 1, 32, 2, 0), (1, 65, 33, 8, 32, 65, 1)])
def case_kda_aggregate(c, B, Cn, L, R, V, F, include_val):
    rng = np.random.default_rng(B + Cn + L + R + V + F)
    s = (1.5 / np.sqrt(2. * V)) ** (1. / 3.)
    fre, fim = KD.freq_tables(rng, R, F)
    dt = rng.uniform(0., 20., size=(B, L)).astype(f32)
    seq, target = c.put(_n(rng, B, L, V, sd=s), "seq"), c.put(_n(rng, B, Cn, V, sd=s), "target")
    value = c.put(_n(rng, B, Cn, R, V, sd=s), "value") if include_val else None
    rel, d_ctx = c.put(_n(rng, R, V, sd=s), "rel"), c.put(_n(rng, B, Cn, R, V), "d_context")
    hist, dt = c.put(KD.history(rng, B, L), "hist"), c.put(dt, "delta_t")
    fre, fim = c.put(fre, "freq_real"), c.put(fim, "freq_imag")
    ctx = c.eng.kda_aggregate_fwd(seq, hist, dt, target, value, rel, fre, fim, bool(include_val))
    grads = c.eng.kda_aggregate_bwd(seq, hist, dt, target, value, rel, fre, fim, d_ctx, bool(include_val))
    return {"context": ctx, **{k: g for k, g in zip(KD.GRADS, grads)}}
