"""GPU: the set-attention engine wrappers run once on torch's allocator and once between guard bands -- inputs, outputs and the
backward's workspace served from tests/guarded.py's arena and allocator stand-in, every view ending on the first band byte, the
workspace exactly the bytes rc_setmab_bwd_workspace_bytes declares.  The second run must leave every band and every input
bit-identical, return finite values and return the first run's bits.  The protocol and helpers are
tests/test_gpu_listenc_guard_bands.py's; the cases live in this module's OWN lists, the table is tests/setmab_guard_table.py.  The
shared [nq, d] query source and a null pad are among the block cases.  A stack of induced blocks (two nodes each, h between them) and
a whole model step from the IMSAB goldens (the port's SetRankGeneral / SetRankSequential over the golden's ranker fixture) run under
the same arena: loss and every gradient repeat the unguarded step's bits."""
import os
import sys

import pytest
import torch

from conftest import ROOT, load_golden

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)
import guarded as G  # noqa: E402
import setmab_guard_table as MT  # noqa: E402
import setrank_np as snp  # noqa: E402
from test_gpu_dcnv2_guard_bands import _fault
from test_gpu_guard_bands import Placer
from test_gpu_listenc_guard_bands import _run_twice, arena, eng  # noqa: F401  (the fixtures and the two-run protocol)

pytestmark = pytest.mark.gpu

CASES, STACK_CASES, MODEL_CASES = [], [], []
ENTRIES = ("rc_setmab_fwd", "rc_setmab_bwd")


def case(entries, params, into=CASES):
    def deco(fn):
        fn.entries = tuple(entries)
        for p in params:
            p = p if isinstance(p, tuple) else (p,)
            into.append(pytest.param(fn, p, id=fn.__name__[5:] + "-" + "-".join(str(x) for x in p)))
        return fn
    return deco


@pytest.mark.parametrize("fn,params", CASES)
def test_setmab_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
    what, called, served, res = _run_twice(fn, params, cuda, eng, arena, monkeypatch, lambda ar: Placer(eng, cuda, ar))
    shared = params[6]
    assert sorted(set(called)) == sorted(MT.GUARDED), (what, called)
    B, nq, nk, d, H, dff = params[:6]
    asked = eng._lib.load().rc_setmab_bwd_workspace_bytes(B, nq, nk, d, H, dff)
    scratch = [k for _, _, dt, k in served.allocations if dt == torch.uint8]
    assert asked > 0 and scratch == [max(asked, 256)], (what, asked, scratch)
    assert len(res) == 15 and tuple(dict(res)["dQs"].shape) == ((nq, d) if shared else (B, nq, d)), what


# (B, nq, nk, d, H, d_ff, shared, masked): the envelope's corners, row counts around the 16-row tile on either side, every tile count
# (1 to 4) on either side, the largest pairs the backward's LDS admits at the default width, the widest width, head widths 4 to 64,
# one list, one row, more lists than workgroups, the register-resident weight-gradient path (d = 64, d_ff = 128) beside the one
# through the partial; a shared source with and without a mask, per-list queries with and without one
@case(ENTRIES, [(1, 1, 1, 16, 1, 16, 0, 0), (2, 20, 1, 64, 4, 128, 1, 1), (3, 1, 20, 64, 4, 128, 0, 0), (5, 20, 15, 16, 4, 256, 1, 0),
                (7, 17, 20, 64, 16, 128, 0, 1), (65, 20, 33, 64, 1, 128, 1, 1), (4, 20, 64, 64, 4, 128, 1, 1), (4, 64, 20, 64, 4, 128, 0, 0),
                (3, 64, 48, 64, 4, 128, 0, 1), (3, 48, 64, 64, 4, 128, 1, 1), (6, 32, 32, 128, 4, 256, 1, 1), (2, 31, 20, 128, 32, 16, 0, 0),
                (260, 20, 40, 64, 4, 128, 1, 1), (260, 40, 20, 64, 4, 128, 0, 0), (300, 20, 9, 48, 3, 64, 1, 0)])
def case_setmab_block(c, B, nq, nk, d, H, dff, shared, masked):
    Qs, Ks, pad, W, dY = snp.random_mab(B, nq, nk, d, H, dff, shared, masked, seed=B + nq + nk + d + H + dff)
    q, k, dy = c.put(Qs, "Qs"), c.put(Ks, "Ks"), c.put(dY, "dY")
    m = c.put(pad, "pad") if masked else None
    w = [c.put(a, n) for a, n in zip(W, snp.WEIGHTS)]
    res = {"Y": c.eng.setmab_fwd(q, k, m, w, H, bool(shared))}
    dQs, dKs, grads = c.eng.setmab_bwd(dy, q, k, m, w, H, bool(shared))
    res["dQs"], res["dKs"] = dQs, dKs
    res.update(zip(snp.GRAD_NAMES[2:], grads))
    return res


@case(ENTRIES, [(9, 40, 64, 4, 128, 3), (4, 12, 32, 2, 128, 2)], into=STACK_CASES)
def case_setmab_stack_step(c, B, n, d, H, dff, L):
    from rechorus_amd import nn as hnn
    one = [snp.random_mab(B, snp.M, n, d, H, dff, 1, 1, seed=60 + l) for l in range(L)]
    two = [snp.random_mab(B, n, snp.M, d, H, dff, 0, 0, seed=70 + l) for l in range(L)]
    leaf = lambda a, name: c.put(a, name).requires_grad_(True)
    I = [leaf(one[l][0], f"I{l}") for l in range(L)]
    w1 = [[leaf(a, f"1{k}{l}") for a, k in zip(one[l][3], snp.WEIGHTS)] for l in range(L)]
    w2 = [[leaf(a, f"2{k}{l}") for a, k in zip(two[l][3], snp.WEIGHTS)] for l in range(L)]
    x = leaf(one[0][1], "X")
    pad, dY = c.put(one[0][2], "pad"), c.put(two[0][4], "dY")
    ws, y = c.eng.SetMabWorkspace(), x
    for l in range(L):
        y = hnn.induced_set_block(y, pad, I[l], w1[l], w2[l], H, ws)
    (y * dY).sum().backward()
    torch.cuda.synchronize()
    out = {"Y": y.detach(), "dX": x.grad}
    for l in range(L):
        out[f"dI{l}"] = I[l].grad
        out.update({f"1{k}{l}": t.grad for k, t in zip(snp.WEIGHTS, w1[l])})
        out.update({f"2{k}{l}": t.grad for k, t in zip(snp.WEIGHTS, w2[l])})
    return out


@pytest.mark.parametrize("fn,params", STACK_CASES)
def test_setmab_stack_step_between_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
    # (autograd may hand a leaf its gradient as a copy of its own: only the bits are held here, not the addresses)
    what, called, served, _ = _run_twice(fn, params, cuda, eng, arena, monkeypatch, lambda ar: Placer(eng, cuda, ar), inside=False)
    B, n, d, H, dff, L = params
    assert called.count("rc_setmab_fwd") == 2 * L and called.count("rc_setmab_bwd") == 2 * L, called
    lib = eng._lib.load()
    asked = sorted(max(256, lib.rc_setmab_bwd_workspace_bytes(B, *s, d, H, dff)) for s in ((snp.M, n), (n, snp.M)))
    assert sorted(k for _, _, dt, k in served.allocations if dt == torch.uint8) == asked      # one buffer per shape for the stack


@case(ENTRIES, ["setrank_a_bprmf_imsab_e32_h64_4h_1b_6p11", "setrank_c_sasrec_imsab_e16_h32_2h_2b_2p3"], into=MODEL_CASES)
def case_setmab_model_step(g, cuda, folder):
    from helpers.ImpressionRunner import ImpressionRunner
    m = snp.meta(g)
    model, _ = snp.golden_model(g, cuda, folder)
    model.train()
    fd = model.add_ranker_outputs(snp.raw_batch(g, 1, cuda), m["B"])
    loss = model.loss(model(fd), ImpressionRunner._labels(fd, m["P"] + m["N"], m["P"], cuda))
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach(), **{k: p.grad for k, p in model.named_parameters() if p.requires_grad}}


@pytest.mark.parametrize("fn,params", MODEL_CASES)
def test_setmab_model_step_between_guard_bands(fn, params, cuda, eng, arena, monkeypatch, tmp_path):
    g = load_golden(params[0])
    m = snp.meta(g)
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
    assert called.count("rc_setmab_fwd") == 2 * m["blocks"] and called.count("rc_setmab_bwd") == 2 * m["blocks"], called
    arena.check()
    lib, n = eng._lib.load(), m["P"] + m["N"]
    scratch = [k for _, _, dt, k in served.allocations if dt == torch.uint8]
    for s in ((snp.M, n), (n, snp.M)):      # one buffer per shape for the whole stack
        asked = lib.rc_setmab_bwd_workspace_bytes(m["B"], *s, m["hidden"], m["H"], 128)
        assert asked > 0 and scratch.count(max(asked, 256)) == 1, (s, asked, scratch)
    assert sorted(plain) == sorted(got) and len(got) == 1 + 6 + 25 * m["blocks"]
    for k in plain:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(G._bytes(plain[k].contiguous()), G._bytes(got[k].contiguous())), f"{params[0]}: '{k}' differs under the arena"
