"""GPU: the DIN engine wrappers run once on torch's allocator and once between guard bands -- inputs, outputs and the workspace
served from tests/guarded.py's arena and allocator stand-in, every view ending on the first band byte, the workspace exactly the
bytes rc_din_attention_bwd_workspace_bytes declares.  The second run must leave every band and every input bit-identical, return
finite values and return the first run's bits.  The protocol is tests/test_gpu_guard_bands.py's, as
tests/test_gpu_cfkg_guard_bands.py applies it; the cases live in this module's OWN list, the table is tests/din_guard_table.py."""
import numpy as np
import pytest
import torch

import din_guard_table as CT
import guard_table as T
import guarded as G
from test_gpu_guard_bands import Placer, _flat, _ids, _n

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
def test_din_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
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
    arena.check(tables=c.tables)        # bands, inputs, and table rows outside the batch
    for tag, asked, buf in served.workspaces:
        assert arena.contains(buf), f"{what}: workspace '{tag}' escaped the arena"
        assert buf.numel() == max(asked, 256), f"{what}: workspace '{tag}' has {buf.numel()} bytes for a declaration of {asked}"
    if "rc_din_attention_bwd" in called:
        asked = [n for tag, n, _ in served.workspaces if tag == "din_bwd"]
        B, H, widths = fn.bwd_shape(*params)
        n_layers, arr = eng._din_widths(widths)
        assert asked and all(n == eng._lib.load().rc_din_attention_bwd_workspace_bytes(B, H, n_layers, arr) for n in asked)
    assert (served.count > 0) == fn.allocates, what
    a, b = _flat(plain), _flat(got)
    assert [p for p, _ in a] == [p for p, _ in b] and len(b) > 0, what
    for (path, x), (_, y) in zip(a, b):
        assert torch.is_tensor(y) and arena.contains(y), f"{what}: result '{path}' escaped the arena"
        if y.dtype.is_floating_point:
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

# a tile is 64 rows (c, l) of one batch row, CT = max(1, 64 // L) candidates: C below, at and past CT; L = 1 and 64; H below and past
# the 16-wide reduction chunk and at both bounds; 1 to 3 layers, widths 16 to 256 and their sum at the bound; with and without
# dropout; the first and the last batch row with a full history, one row without any (a read past keys would land on a band)
@case(("rc_din_attention_fwd", "rc_din_attention_bwd"),
      [(1, 1, 1, 4, (16,), 0.0), (3, 1, 64, 512, (256,), 0.0), (2, 101, 10, 192, (64, 64, 64), 0.5), (33, 1, 40, 448, (64, 64), 0.0),
       (7, 5, 20, 12, (16, 240), 0.8), (5, 7, 10, 20, (32,), 0.0), (3, 64, 1, 16, (16, 16), 0.5), (2, 65, 1, 8, (16,), 0.0),
       (4, 6, 10, 8, (16, 16, 16), 0.0), (17, 2, 32, 36, (48,), 0.0), (2, 3, 33, 16, (16,), 0.5), (1, 13, 5, 512, (128, 128), 0.0)])
def case_din_attention(c, B, Cn, L, H, widths, p):
    rng = np.random.default_rng(B + Cn + L + H)
    lens = rng.integers(1, L + 1, size=B).astype(np.int64)
    lens[0], lens[-1] = L, L
    if B > 2:
        lens[1] = 0
    n_par = c.eng.din_param_count(H, widths)
    q, keys = c.put(_n(rng, B * Cn, H), "q"), c.put(_n(rng, B, L, H), "keys")
    flat, d_out = c.put(_n(rng, n_par, sd=0.05), "params"), c.put(_n(rng, B * Cn, H), "d_out")
    lengths = c.put(lens, "lengths")
    seed = c.seed(12345) if p else None
    out, att = c.eng.din_attention_fwd(q, keys, lengths, flat, Cn, widths, p, seed, 3, want_att=True)
    dq, dkeys, dflat = c.eng.din_attention_bwd(q, keys, lengths, flat, d_out, Cn, widths, p, seed, 3)
    return {"out": out, "att": att, "dq": dq, "dkeys": dkeys, "dparams": dflat}


case_din_attention.bwd_shape = lambda B, Cn, L, H, widths, p: (B, H, widths)
