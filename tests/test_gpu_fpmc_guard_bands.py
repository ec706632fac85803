"""GPU: every FPMC engine wrapper runs once on torch's allocator and once between guard bands -- inputs, outputs and workspaces
served from tests/guarded.py's arena and allocator stand-in, every view ending on the first band byte, the workspace exactly the
bytes rc_fpmc_item_update_workspace_bytes declares.  The second run must leave every band, every input and every table row outside
the batch bit-identical, return finite values and return the first run's bits.  The protocol is tests/test_gpu_guard_bands.py's;
the cases live in this module's OWN list (that file's CASES is held to tests/guard_table.py case by case), the table is
tests/fpmc_guard_table.py."""
import numpy as np
import pytest
import torch

import fpmc_guard_table as FT
import guard_table as T
import guarded as G
from test_gpu_guard_bands import Placer, _flat, _ids, _n, _opt_tables

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
def test_fpmc_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
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
    stray = sorted(set(called) - set(T.GUARDED) - set(FT.GUARDED))
    assert not stray, f"{what}: reached entry points that neither guard table lists as guarded: {stray}"
    REACHED.setdefault(fn.__name__, [0, set()])
    REACHED[fn.__name__][0] += 1
    REACHED[fn.__name__][1].update(called)
    arena.check(tables=c.tables)        # bands, inputs, and table rows outside the batch
    for tag, asked, buf in served.workspaces:
        assert arena.contains(buf), f"{what}: workspace '{tag}' escaped the arena"
        assert buf.numel() == max(asked, 256), f"{what}: workspace '{tag}' has {buf.numel()} bytes for a declaration of {asked}"
    if "rc_fpmc_item_update" in called:
        asked = [n for tag, n, _ in served.workspaces if tag == "fpmc_item"]
        assert asked and all(n == eng._lib.load().rc_fpmc_item_update_workspace_bytes(*fn.item_update_shape(*params)) for n in asked)
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

N_USERS, N_ITEMS = 23, 301


def _tables(c, rng, d, touched=None):
    """UI, LI, IU, IL: inputs, or (touched = {name: rows}) tables updated in place"""
    out = []
    for name, rows in (("UI", N_USERS), ("LI", N_ITEMS), ("IU", N_ITEMS), ("IL", N_ITEMS)):
        x = _n(rng, rows, d, sd=0.2)
        out.append(c.table(x, name, touched[name]) if touched and name in touched else c.put(x, name))
    return out


def _batch(rng, B, Cn, hot=False):
    uid, lid, iid = _ids(rng, 0, N_USERS, B), _ids(rng, 0, N_ITEMS, B), _ids(rng, 0, N_ITEMS, B, Cn)
    if hot:      # rows with more than 32 occurrences (the long-row kernel) beside singletons
        iid.reshape(-1)[: iid.size // 3] %= 5
    iid[0, -1], iid[-1, 0] = N_ITEMS - 1, 0
    return uid, lid, iid


# both paths of rc_fpmc_fwd_bwd at every width: register (several tuples per wave, the full 50-row layout) and streaming
@case(("rc_fpmc_scores", "rc_fpmc_fwd_bwd"),
      [(16, 1, 2), (16, 3, 265), (32, 3, 5), (32, 2, 201), (64, 7, 100), (64, 5, 101), (64, 65, 65), (128, 5, 33), (128, 2, 100),
       (64, 3, 1)])
def case_fpmc_front(c, d, B, Cn):
    rng = np.random.default_rng(d + B + Cn)
    UI, LI, IU, IL = _tables(c, rng, d)
    ids = _batch(rng, B, Cn)
    uid, lid, iid = (c.put(x, n) for x, n in zip(ids, ("uid", "lid", "iid")))
    res = {"scores": c.eng.fpmc_scores(UI, LI, IU, IL, uid, lid, iid)}
    if Cn == 1:      # one candidate is the score kernel's case; the fused step needs a negative: the same column twice
        iid = c.put(np.concatenate([ids[2], ids[2]], axis=1), "iid2")
    res["fused"] = c.eng.fpmc_fwd_bwd(UI, LI, IU, IL, uid, lid, iid)
    res["fused_nopred"] = c.eng.fpmc_fwd_bwd(UI, LI, IU, IL, uid, lid, iid, want_pred=False)
    return res


@case(("rc_fpmc_item_update", "rc_sort_ids", "rc_segment_heads"),
      [(d, opt) for d in (16, 32, 64, 128) for opt in (None, "SGD", "Adam")] + [(64, "Adagrad")])
def case_fpmc_item_update(c, d, opt):
    rng = np.random.default_rng(d + 7)
    B, Cn = 37, 9
    uid, lid, iid = _batch(rng, B, Cn, hot=True)
    UI, LI = c.put(_n(rng, N_USERS, d, sd=0.2), "UI"), c.put(_n(rng, N_ITEMS, d, sd=0.2), "LI")
    gpred = c.put(_n(rng, B, Cn), "gpred")
    d_uid, d_lid = c.put(uid, "uid"), c.put(lid, "lid")
    keys, perm = c.eng.sort_ids(c.put(iid, "iid"), N_ITEMS)
    _, heads, n_heads = c.eng.segment_heads(keys, perm, want_single=False)
    if opt is None:
        Ga, Gb = c.inout(np.zeros((N_ITEMS, d), f32), "GIU"), c.inout(np.zeros((N_ITEMS, d), f32), "GIL")
        c.eng.fpmc_item_update(keys, perm, heads, n_heads, gpred, UI, LI, d_uid, d_lid, dense_grad=(Ga, Gb))
        return {"GIU": Ga, "GIL": Gb}
    IU, mIU, vIU = _opt_tables(c, rng, N_ITEMS, d, opt, iid, "IU")
    IL, mIL, vIL = _opt_tables(c, rng, N_ITEMS, d, opt, iid, "IL")
    c.eng.fpmc_item_update(keys, perm, heads, n_heads, gpred, UI, LI, d_uid, d_lid, hyper=c.eng.make_hyper(opt, lr=0.01, l2=1e-4, step=3),
                           IU=IU, IL=IL, m=(mIU, mIL), v=(vIU, vIL))
    return {"IU": IU, "mIU": mIU, "vIU": vIU, "IL": IL, "mIL": mIL, "vIL": vIL}


case_fpmc_item_update.item_update_shape = lambda d, opt: (37 * 9, d)


@case(("rc_fpmc_fwd_bwd", "rc_fpmc_item_update", "rc_sort_ids", "rc_segment_heads", "rc_segmented_update", "rc_reduce_sum"),
      [(16, "SGD", 3, 5), (64, "Adam", 7, 100), (64, "Adagrad", 5, 101), (128, "SGD", 33, 10)])
def case_fpmc_trainer(c, d, opt, B, Cn):
    rng = np.random.default_rng(d + B)
    uid, lid, iid = _batch(rng, B, Cn, hot=True)
    UI, LI, IU, IL = _tables(c, rng, d, touched={"UI": uid, "LI": lid, "IU": iid, "IL": iid})
    ids = [c.put(x, n) for x, n in zip((uid, lid, iid), ("uid", "lid", "iid"))]
    tr = c.eng.FpmcTrainer(UI, LI, IU, IL, opt=opt, lr=0.01, l2=1e-4)
    losses = [tr.step(*ids).clone() for _ in range(2)]
    res = {"UI": UI, "LI": LI, "IU": IU, "IL": IL, "loss": c.eng.reduce_sum(torch.cat(losses), 1.0)}
    for k in ("UI", "LI", "IU", "IL"):
        res.update({f"{n}{k}": t for n, t in tr.state[k].items()})
    return res


case_fpmc_trainer.item_update_shape = lambda d, opt, B, Cn: (B * Cn, d)
