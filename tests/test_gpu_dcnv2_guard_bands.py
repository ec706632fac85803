"""GPU: the DCNv2 engine wrappers run once on torch's allocator and once between guard bands -- inputs, outputs and the backward's
workspace served from tests/guarded.py's arena and allocator stand-in, every view ending on the first band byte, the workspace exactly
the bytes rc_dcnv2_mix_layer_bwd_workspace_bytes declares.  The second run must leave every band and every input bit-identical, return
finite values and return the first run's bits.  The protocol is tests/test_gpu_guard_bands.py's, as
tests/test_gpu_chorus_guard_bands.py applies it; the cases live in this module's OWN lists, the table is tests/dcnv2_guard_table.py.
A whole model step (forward, loss, backward through rechorus_amd.nn) runs under the same arena: whatever the engine allocates for it
lies between bands, and loss and every gradient repeat the unguarded step's bits."""
import numpy as np
import pytest
import torch

import dcnv2_guard_table as DT
import dcnv2_np as dnp
import guarded as G
from conftest import load_golden
from test_gpu_guard_bands import Placer, _flat

pytestmark = pytest.mark.gpu

ARENA_BYTES = 160 << 20
CASES, MODEL_CASES = [], []


def case(entries, params, into=CASES):
    def deco(fn):
        fn.entries = tuple(entries)
        for p in params:
            p = p if isinstance(p, tuple) else (p,)
            into.append(pytest.param(fn, p, id=fn.__name__[5:] + "-" + "-".join(str(x) for x in p)))
        return fn
    return deco


class _AliasArena(G.Arena):
    """the arena with every served tensor re-imported through DLPack: the same memory, but no longer a VIEW of the arena buffer in
    autograd's books.  The model step runs custom autograd Functions on what the engine allocates; autograd refuses a Function
    output that is a view whose base was written in place, and the arena writes its buffer in place whenever it lays a band."""

    def take(self, shape, dtype, name, kind="out"):
        t = torch.utils.dlpack.from_dlpack(torch.utils.dlpack.to_dlpack(super().take(shape, dtype, name, kind)))
        self.views[-1].tensor = t
        return t


@pytest.fixture(scope="module")
def arena(cuda):
    a = _AliasArena(cuda, ARENA_BYTES)
    yield a
    del a


@pytest.fixture(scope="module")
def eng(cuda):
    from rechorus_amd import engine
    return engine


def _fault(e, what):
    if "illegal memory access" in str(e) or "HIP error" in str(e) or "hipError" in str(e):
        # the device is in an unknown state: nothing more is started on it in this session
        pytest.exit(f"GPU fault in {what}: {str(e).splitlines()[0]}", returncode=3)


@pytest.mark.parametrize("fn,params", CASES)
def test_dcnv2_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
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
        _fault(e, what)
        raise
    assert sorted(set(called)) == sorted(DT.GUARDED), (what, called)
    arena.check()        # bands and inputs
    N, D, r, E = params[:4]
    asked = eng._lib.load().rc_dcnv2_mix_layer_bwd_workspace_bytes(N, D, r, E)
    scratch = [n for _, _, dt, n in served.allocations if dt == torch.uint8]
    assert asked > 0 and scratch == [max(asked, 256)], (what, asked, scratch)
    a, b = _flat(plain), _flat(got)
    assert [p for p, _ in a] == [p for p, _ in b] and len(b) == 9, what
    for (path, x), (_, y) in zip(a, b):
        assert arena.contains(y), f"{what}: result '{path}' escaped the arena"
        assert bool(torch.isfinite(y).all()), f"{what}: result '{path}' is not finite"
        assert x.shape == y.shape and torch.equal(G._bytes(x.contiguous()), G._bytes(y.contiguous())), \
            f"{what}: '{path}' differs between the plain and the guarded run"


# the envelope's corners, widths that are no multiple of 16, every tile height (16 / 32 / 64 rows), a row count that is no multiple
# of the tile, one row, and more tiles than workgroups (N = 4200 at 16 rows a tile: 263 tiles on 256 workgroups)
@case(("rc_dcnv2_mix_layer_fwd", "rc_dcnv2_mix_layer_bwd"),
      [(1, 8, 4, 1), (2, 8, 12, 4), (63, 24, 8, 2), (65, 132, 36, 3), (257, 512, 64, 2), (70, 1024, 128, 4), (4200, 36, 4, 2),
       (8200, 64, 16, 2), (16400, 20, 8, 1)])
def case_dcnv2_layer(c, N, D, r, E):
    names = ("X0", "Xl", "U", "V", "C", "bias", "Wg", "bg", "dXnext")
    t = [c.put(x, n) for x, n in zip(dnp.random_layer(N, D, r, E, seed=N + D + r + E), names)]
    res = {"Xnext": c.eng.dcnv2_mix_layer_fwd(*t[:8])}
    res.update(zip(dnp.GRAD_NAMES, c.eng.dcnv2_mix_layer_bwd(t[8], *t[:8])))
    return res


@case(("rc_dcnv2_mix_layer_fwd", "rc_dcnv2_mix_layer_bwd"),
      ["dcnv2_a_ctr_mix_stacked_d16_r8_e2_l3", "dcnv2_d_topk_mix_stacked_d4_r12_e4_l1"], into=MODEL_CASES)
def case_dcnv2_model_step(g, cuda):
    model, _ = dnp.scaled_model(g, cuda)
    model.train()
    loss = model.loss(model(dnp.feed(g, 1, cuda)))
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach(), **{k: p.grad for k, p in model.named_parameters()}}


@pytest.mark.parametrize("fn,params", MODEL_CASES)
def test_dcnv2_model_step_between_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
    g = load_golden(params[0])
    m = dnp.meta(g)
    try:
        plain = fn(g, cuda)
        arena.reset()
        called = []
        real_call = eng._lib.call
        with G.guarded(eng, arena, monkeypatch) as served:
            monkeypatch.setattr(eng._lib, "call", lambda name, *a: called.append(name) or real_call(name, *a))
            got = fn(g, cuda)
        monkeypatch.setattr(eng._lib, "call", real_call)
    except RuntimeError as e:
        _fault(e, params[0])
        raise
    assert called.count("rc_dcnv2_mix_layer_fwd") == m["L"] and called.count("rc_dcnv2_mix_layer_bwd") == m["L"], called
    arena.check()
    asked = eng._lib.load().rc_dcnv2_mix_layer_bwd_workspace_bytes(m["B"] * m["C"], m["d"] * len(m["fields"]), m["r"], m["E"])
    assert max(asked, 256) in [n for _, _, dt, n in served.allocations if dt == torch.uint8]
    assert sorted(plain) == sorted(got)
    for k in plain:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(G._bytes(plain[k].contiguous()), G._bytes(got[k].contiguous())), f"{params[0]}: '{k}' differs under the arena"
