"""GPU: the list-encoder engine wrappers run once on torch's allocator and once between guard bands -- inputs, outputs and the
backward's workspace served from tests/guarded.py's arena and allocator stand-in, every view ending on the first band byte, the
workspace exactly the bytes rc_listenc_block_bwd_workspace_bytes declares.  The second run must leave every band and every input
bit-identical, return finite values and return the first run's bits.  The protocol is tests/test_gpu_guard_bands.py's, as
tests/test_gpu_dcnv2_guard_bands.py applies it; the cases live in this module's OWN lists, the table is tests/listenc_guard_table.py.
A whole model step from a golden (the port's PRMGeneral / PRMSequential over the golden's ranker fixture: the ranker's forward and the
ranks of collate_batch, the two embedding gathers, rFF0, every block, rFF1, the list-level BPR, backward) runs under the same arena:
whatever the engine allocates for it lies between bands, and loss and every gradient repeat the unguarded step's bits.  So does a
bare stack of block nodes at the default shape, which no golden has."""
import os
import sys

import pytest
import torch

from conftest import ROOT, load_golden

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)
import guarded as G  # noqa: E402
import listenc_guard_table as LT  # noqa: E402
import prm_np as pnp  # noqa: E402
from test_gpu_dcnv2_guard_bands import _AliasArena, _fault
from test_gpu_guard_bands import Placer, _flat

pytestmark = pytest.mark.gpu

ARENA_BYTES = 192 << 20
CASES, STACK_CASES, MODEL_CASES = [], [], []


def case(entries, params, into=CASES):
    def deco(fn):
        fn.entries = tuple(entries)
        for p in params:
            p = p if isinstance(p, tuple) else (p,)
            into.append(pytest.param(fn, p, id=fn.__name__[5:] + "-" + "-".join(str(x) for x in p)))
        return fn
    return deco


@pytest.fixture(scope="module")
def arena(cuda):
    a = _AliasArena(cuda, ARENA_BYTES)
    yield a
    del a


@pytest.fixture(scope="module")
def eng(cuda):
    from rechorus_amd import engine
    return engine


def _run_twice(fn, params, cuda, eng, arena, monkeypatch, make, inside=True):
    what = f"{fn.__name__[5:]} {params}"
    try:
        plain = fn(make(None), *params)
        torch.cuda.synchronize()
        arena.reset()
        called = []
        real_call = eng._lib.call
        with G.guarded(eng, arena, monkeypatch) as served:
            monkeypatch.setattr(eng._lib, "call", lambda name, *a: called.append(name) or real_call(name, *a))
            got = fn(make(arena), *params)
            torch.cuda.synchronize()
        monkeypatch.setattr(eng._lib, "call", real_call)
    except RuntimeError as e:
        _fault(e, what)
        raise
    arena.check()        # bands and inputs
    a, b = _flat(plain), _flat(got)
    assert [p for p, _ in a] == [p for p, _ in b], what
    for (path, x), (_, y) in zip(a, b):
        assert not inside or arena.contains(y), f"{what}: result '{path}' escaped the arena"
        assert bool(torch.isfinite(y).all()), f"{what}: result '{path}' is not finite"
        assert x.shape == y.shape and torch.equal(G._bytes(x.contiguous()), G._bytes(y.contiguous())), \
            f"{what}: '{path}' differs between the plain and the guarded run"
    return what, called, served, b


@pytest.mark.parametrize("fn,params", CASES)
def test_listenc_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
    what, called, served, res = _run_twice(fn, params, cuda, eng, arena, monkeypatch, lambda ar: Placer(eng, cuda, ar))
    assert sorted(set(called)) == sorted(LT.GUARDED), (what, called)
    B, n, d, H, dff = params
    asked = eng._lib.load().rc_listenc_block_bwd_workspace_bytes(B, n, d, H, dff)
    scratch = [k for _, _, dt, k in served.allocations if dt == torch.uint8]
    assert asked > 0 and scratch == [max(asked, 256)], (what, asked, scratch)
    assert len(res) == 14, what


# the envelope's corners, lengths around the 16-row tile, every tile count (1 to 4), one list, one slot, more lists than workgroups,
# the widest list at the default width (the LDS ceiling of the backward), the widest width, head widths 4 to 64, and the register-
# resident weight-gradient path (d = 64, d_ff = 128) beside the one through the partial
@case(("rc_listenc_block_fwd", "rc_listenc_block_bwd"),
      [(1, 1, 16, 1, 16), (2, 1, 64, 4, 128), (3, 15, 16, 4, 256), (5, 16, 32, 2, 16), (7, 17, 64, 16, 128), (65, 33, 64, 1, 128),
       (4, 64, 64, 4, 128), (3, 64, 64, 4, 192), (6, 32, 128, 4, 256), (2, 31, 128, 32, 16), (260, 40, 64, 4, 128), (300, 9, 48, 3, 64)])
def case_listenc_block(c, B, n, d, H, dff):
    X, pad, W, dY = pnp.random_block(B, n, d, H, dff, seed=B + n + d + H + dff)
    x, m, dy = c.put(X, "X"), c.put(pad, "pad"), c.put(dY, "dY")
    w = [c.put(a, k) for a, k in zip(W, pnp.WEIGHTS)]
    res = {"Y": c.eng.listenc_block_fwd(x, m, w, H)}
    dX, grads = c.eng.listenc_block_bwd(dy, x, m, w, H)
    res["dX"] = dX
    res.update(zip(pnp.GRAD_NAMES[1:], grads))
    return res


@case(("rc_listenc_block_fwd", "rc_listenc_block_bwd"), [(9, 40, 64, 4, 128, 3), (4, 12, 32, 2, 128, 2)], into=STACK_CASES)
def case_listenc_stack_step(c, B, n, d, H, dff, L):
    from rechorus_amd import nn as hnn
    blocks = [pnp.random_block(B, n, d, H, dff, seed=50 + l) for l in range(L)]
    leaves = [[c.put(a, f"{k}{l}").requires_grad_(True) for a, k in zip(blocks[l][2], pnp.WEIGHTS)] for l in range(L)]
    x = c.put(blocks[0][0], "X").requires_grad_(True)
    pad, dY = c.put(blocks[0][1], "pad"), c.put(blocks[0][3], "dY")
    ws, y = c.eng.ListEncWorkspace(), x
    for l in range(L):
        y = hnn.list_encoder_block(y, pad, leaves[l], H, ws)
    (y * dY).sum().backward()
    torch.cuda.synchronize()
    return {"Y": y.detach(), "dX": x.grad, **{f"{k}{l}": t.grad for l in range(L) for k, t in zip(pnp.WEIGHTS, leaves[l])}}


@pytest.mark.parametrize("fn,params", STACK_CASES)
def test_listenc_stack_step_between_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
    # (autograd may hand a leaf its gradient as a copy of its own: only the bits are held here, not the addresses)
    what, called, served, _ = _run_twice(fn, params, cuda, eng, arena, monkeypatch, lambda ar: Placer(eng, cuda, ar), inside=False)
    B, n, d, H, dff, L = params
    assert called.count("rc_listenc_block_fwd") == L and called.count("rc_listenc_block_bwd") == L, called
    asked = eng._lib.load().rc_listenc_block_bwd_workspace_bytes(B, n, d, H, dff)
    assert [k for _, _, dt, k in served.allocations if dt == torch.uint8] == [max(asked, 256)]      # one workspace for the stack


@case(("rc_listenc_block_fwd", "rc_listenc_block_bwd"), ["prm_a_bprmf_e64_h64_4h_2b_3p4", "prm_d_sasrec_e16_h64_4h_1b_2p3"], into=MODEL_CASES)
def case_listenc_model_step(g, cuda, folder):
    from helpers.ImpressionRunner import ImpressionRunner
    m = pnp.meta(g)
    model, _ = pnp.golden_model(g, cuda, folder)
    model.train()
    fd = model.add_ranker_outputs(pnp.raw_batch(g, 1, cuda), m["B"])
    loss = model.loss(model(fd), ImpressionRunner._labels(fd, m["P"] + m["N"], m["P"], cuda))
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach(), **{k: p.grad for k, p in model.named_parameters() if p.requires_grad}}


@pytest.mark.parametrize("fn,params", MODEL_CASES)
def test_listenc_model_step_between_guard_bands(fn, params, cuda, eng, arena, monkeypatch, tmp_path):
    g = load_golden(params[0])
    m = pnp.meta(g)
    monkeypatch.chdir(tmp_path)
    try:
        plain = fn(g, cuda, tmp_path)
        arena.reset()
        called = []
        real_call = eng._lib.call
        with G.guarded(eng, arena, monkeypatch) as served:
            monkeypatch.setattr(eng._lib, "call", lambda name, *a: called.append(name) or real_call(name, *a))
            got = fn(g, cuda, tmp_path)
        monkeypatch.setattr(eng._lib, "call", real_call)
    except RuntimeError as e:
        _fault(e, params[0])
        raise
    assert called.count("rc_listenc_block_fwd") == m["blocks"] and called.count("rc_listenc_block_bwd") == m["blocks"], called
    arena.check()
    asked = eng._lib.load().rc_listenc_block_bwd_workspace_bytes(m["B"], m["P"] + m["N"], m["hidden"], m["H"], 128)
    assert asked > 0 and [k for _, _, dt, k in served.allocations if dt == torch.uint8].count(max(asked, 256)) == 1      # one for the stack
    assert sorted(plain) == sorted(got) and len(got) == 1 + 6 + 12 * m["blocks"]
    for k in plain:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(G._bytes(plain[k].contiguous()), G._bytes(got[k].contiguous())), f"{params[0]}: '{k}' differs under the arena"
