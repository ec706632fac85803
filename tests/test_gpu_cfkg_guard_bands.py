"""GPU: every CFKG engine wrapper runs once on torch's allocator and once between guard bands -- inputs, outputs and workspaces
served from tests/guarded.py's arena and allocator stand-in, every view ending on the first band byte, the workspace exactly the
bytes rc_cfkg_fwd_bwd_workspace_bytes declares.  The second run must leave every band, every input and every table row outside
the batch bit-identical, return finite values and return the first run's bits.  The protocol is tests/test_gpu_guard_bands.py's,
as tests/test_gpu_slrc_guard_bands.py applies it; the cases live in this module's OWN list, the table is tests/cfkg_guard_table.py."""
import numpy as np
import pytest
import torch

import cfkg_guard_table as CT
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
def test_cfkg_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
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
    if "rc_cfkg_fwd_bwd" in called:
        asked = [n for tag, n, _ in served.workspaces if tag == "cfkg_front"]
        assert asked and all(n == eng._lib.load().rc_cfkg_fwd_bwd_workspace_bytes(*fn.front_shape(*params)) for n in asked)
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

N_USERS, N_ROWS = 23, 301        # E has N_ROWS rows, the first N_USERS of them users


def _quad(rng, B, n_rel):
    """(h, t, hn, tn, r): the first and the last row of E and the last relation occur -- a read past them would land on a band"""
    h, hn = _ids(rng, 0, N_ROWS, B), _ids(rng, 0, N_ROWS, B)
    t, tn = _ids(rng, N_USERS, N_ROWS, B), _ids(rng, N_USERS, N_ROWS, B)
    r = _ids(rng, 0, n_rel, B)
    h[0], t[-1], hn[-1], tn[0], r[-1] = 0, N_ROWS - 1, N_ROWS - 1, t[0], n_rel - 1
    return h, t, hn, tn, r


# every width; n_rel at and between the accumulator counts 1 / 2 / 4 / 8; B on both sides of the rows a workgroup takes (256 / 128 /
# 64 / 32 at d = 16 / 32 / 64 / 128); C = 1, a wave's share, and past one workgroup's candidates, shared and distinct heads
@case(("rc_cfkg_scores", "rc_cfkg_scores_bwd", "rc_cfkg_fwd_bwd"),
      [(16, 1, 1, 1), (16, 3, 256, 100), (16, 8, 257, 3), (32, 2, 128, 7), (32, 5, 129, 1025), (64, 4, 64, 100), (64, 4, 65, 101),
       (64, 8, 3, 1025), (128, 8, 32, 33), (128, 1, 33, 100)])
def case_cfkg_front(c, d, n_rel, B, Cn):
    rng = np.random.default_rng(d + n_rel + B + Cn)
    E, R = c.put(_n(rng, N_ROWS, d, sd=0.3), "E"), c.put(_n(rng, n_rel, d, sd=0.3), "R")
    res = {}
    for shared in (True, False):
        head = np.repeat(_ids(rng, 0, N_USERS, B)[:, None], Cn, axis=1) if shared else _ids(rng, 0, N_ROWS, B, Cn)
        rel = np.zeros((B, Cn), np.int64) if shared else _ids(rng, 0, n_rel, B, Cn)
        tail = _ids(rng, N_USERS, N_ROWS, B, Cn)
        tail[0, -1], tail[-1, 0], rel[-1, -1] = N_ROWS - 1, N_USERS, (0 if shared else n_rel - 1)
        tag = "shared" if shared else "mixed"
        ids = [c.put(x, n + tag) for x, n in ((head, "head"), (tail, "tail"), (rel, "rel"))]
        res["scores_" + tag] = c.eng.cfkg_scores(E, R, *ids)
        res["grads_" + tag] = c.eng.cfkg_scores_grads(E, R, *ids, c.put(_n(rng, B, Cn), "gpred" + tag))
    quad = [c.put(x, n) for x, n in zip(_quad(rng, B, n_rel), ("h", "t", "hn", "tn", "r"))]
    res["fused"] = c.eng.cfkg_fwd_bwd(E, R, *quad, margin=0.5)
    res["fused_nopred"] = c.eng.cfkg_fwd_bwd(E, R, *quad, margin=0.0, want_pred=False)
    return res


case_cfkg_front.front_shape = lambda d, n_rel, B, Cn: (B, d, n_rel)


@case(("rc_cfkg_fwd_bwd", "rc_sort_ids", "rc_segmented_update", "rc_reduce_sum", "rc_dense_update"),
      [(16, 1, "SGD", 3), (64, 4, "Adam", 65), (32, 3, "Adagrad", 129), (128, 8, "SGD", 33)])
def case_cfkg_trainer(c, d, n_rel, opt, B):
    rng = np.random.default_rng(d + B)
    h, t, hn, tn, r = _quad(rng, B, n_rel)
    head, tail, rel = np.stack([h, h, h, hn], 1), np.stack([t, t, tn, t], 1), np.repeat(r[:, None], 4, 1)
    E = c.table(_n(rng, N_ROWS, d, sd=0.3), "E", np.concatenate([h, t, hn, tn]))
    R = c.table(_n(rng, n_rel, d, sd=0.3), "R", np.arange(n_rel))
    ids = [c.put(x, n) for x, n in zip((head, tail, rel), ("head", "tail", "rel"))]
    tr = c.eng.CfkgTrainer(E, R, margin=0.5, opt=opt, lr=0.01, l2=1e-4)
    losses = [tr.step(*ids).clone() for _ in range(2)]
    res = {"E": E, "R": R, "loss": c.eng.reduce_sum(torch.cat(losses), 1.0)}
    for k in ("E", "R"):
        res.update({f"{n}_{k}": x for n, x in tr.state[k].items()})
    return res


case_cfkg_trainer.front_shape = lambda d, n_rel, opt, B: (B, d, n_rel)
