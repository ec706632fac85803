"""GPU: every SLRC+ engine wrapper runs once on torch's allocator and once between guard bands -- inputs, outputs and workspaces
served from tests/guarded.py's arena and allocator stand-in, every view ending on the first band byte, the workspace exactly the
bytes rc_slrc_item_update_workspace_bytes declares.  The second run must leave every band, every input and every table row outside
the batch bit-identical, return finite values and return the first run's bits.  The protocol is tests/test_gpu_guard_bands.py's,
as tests/test_gpu_fpmc_guard_bands.py applies it; the cases live in this module's OWN list, the table is tests/slrc_guard_table.py."""
import numpy as np
import pytest
import torch

import guard_table as T
import guarded as G
import slrc_guard_table as ST
from test_gpu_guard_bands import Placer, _flat, _ids, _n

pytestmark = pytest.mark.gpu

ARENA_BYTES = 64 << 20
f32 = np.float32
CASES = []
REACHED = {}        # case function -> [cases run, entry points called between the bands]
ITEM_TABLES = ("I", "item_bias", "alphas", "pis", "betas", "sigmas", "mus")


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
def test_slrc_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
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
    stray = sorted(set(called) - set(T.GUARDED) - set(ST.GUARDED))
    assert not stray, f"{what}: reached entry points that neither guard table lists as guarded: {stray}"
    REACHED.setdefault(fn.__name__, [0, set()])
    REACHED[fn.__name__][0] += 1
    REACHED[fn.__name__][1].update(called)
    arena.check(tables=c.tables)        # bands, inputs, and table rows outside the batch
    for tag, asked, buf in served.workspaces:
        assert arena.contains(buf), f"{what}: workspace '{tag}' escaped the arena"
        assert buf.numel() == max(asked, 256), f"{what}: workspace '{tag}' has {buf.numel()} bytes for a declaration of {asked}"
    if "rc_slrc_item_update" in called:
        asked = [n for tag, n, _ in served.workspaces if tag == "slrc_item"]
        assert asked and all(n == eng._lib.load().rc_slrc_item_update_workspace_bytes(*fn.item_update_shape(*params)) for n in asked)
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


def _params(c, rng, d, R, touched=None):
    """the ten parameters in engine.SLRC_PARAMS order: inputs, or (touched = {name: rows}) tables updated in place.  The last item's
    rows end each Hawkes table: a read past them would land on a band."""
    shapes = {"U": (N_USERS, d), "I": (N_ITEMS, d), "user_bias": (N_USERS, 1), "item_bias": (N_ITEMS, 1), "global_alpha": (1,)}
    out = []
    for name in c.eng.SLRC_PARAMS:
        x = np.asarray(_n(rng, *shapes.get(name, (N_ITEMS, R)), sd=0.2))
        if name == "betas":
            x[0, 0], x[1, R - 1], x[2, 0] = -1.5, 9.0, 11.0        # below, at and above the clamp
        if name == "sigmas":
            x[3, 0], x[4, R - 1], x[5, 0] = -1.5, 9.0, 11.0
        if touched is None:
            out.append(c.put(x, name))
        elif name == "global_alpha":
            out.append(c.inout(x, name))
        else:
            out.append(c.table(x, name, touched[name]))
    return out


def _batch(rng, B, Cn, R, hot=False):
    uid, iid = _ids(rng, 0, N_USERS, B), _ids(rng, 0, N_ITEMS, B, Cn)
    if hot:      # rows with more than 32 occurrences (the long-row kernel) beside singletons
        iid.reshape(-1)[: iid.size // 3] %= 6
    iid[0, -1], iid[-1, 0] = N_ITEMS - 1, 0
    iv = np.where(rng.random((B, Cn, R)) < 0.4, -1.0, rng.uniform(0, 3, (B, Cn, R))).astype(f32)
    iv[0, 0, 0] = 0.0
    return uid, iid, iv


# both paths of rc_slrc_fwd_bwd at every width: register (the smallest and the full 25-row layout) and streaming; R = 1, 3, 8
@case(("rc_slrc_scores", "rc_slrc_fwd_bwd", "rc_slrc_excitation_bwd"),
      [(16, 1, 1, 2), (16, 3, 3, 401), (32, 3, 3, 5), (32, 8, 2, 201), (64, 3, 7, 100), (64, 3, 5, 101), (64, 1, 65, 65),
       (128, 8, 5, 33), (128, 3, 2, 51), (64, 3, 3, 1)])
def case_slrc_front(c, d, R, B, Cn):
    rng = np.random.default_rng(d + R + B + Cn)
    P = _params(c, rng, d, R)
    uid, iid, iv = _batch(rng, B, Cn, R)
    d_uid, d_iid, d_iv = c.put(uid, "uid"), c.put(iid, "iid"), c.put(iv, "intervals")
    res = {"scores": c.eng.slrc_scores(P, d_uid, d_iid, d_iv)}
    res["excitation"] = c.eng.slrc_excitation_grads(P, d_uid, d_iid, d_iv, c.put(_n(rng, B, Cn), "gpred"))
    if Cn == 1:      # one candidate is the score kernel's case; the fused step needs a negative: the same column twice
        d_iid, d_iv = c.put(np.concatenate([iid, iid], axis=1), "iid2"), c.put(np.concatenate([iv, iv], axis=1), "intervals2")
    res["fused"] = c.eng.slrc_fwd_bwd(P, d_uid, d_iid, d_iv)
    res["fused_nopred"] = c.eng.slrc_fwd_bwd(P, d_uid, d_iid, d_iv, want_pred=False)
    return res


@case(("rc_slrc_item_update", "rc_sort_ids", "rc_segment_heads"),
      [(d, R, opt) for d, R in ((16, 8), (32, 3), (64, 3), (128, 1)) for opt in (None, "SGD", "Adam")] + [(64, 8, "Adagrad")])
def case_slrc_item_update(c, d, R, opt):
    rng = np.random.default_rng(d + R + 7)
    B, Cn = 37, 9
    uid, iid, _ = _batch(rng, B, Cn, R, hot=True)
    U = c.put(_n(rng, N_USERS, d, sd=0.2), "U")
    gpred, hgrad = c.put(_n(rng, B, Cn), "gpred"), c.put(_n(rng, B * Cn, 5 * R), "hgrad")
    d_uid = c.put(uid, "uid")
    keys, perm = c.eng.sort_ids(c.put(iid, "iid"), N_ITEMS)
    _, heads, n_heads = c.eng.segment_heads(keys, perm, want_single=False)
    width = {"I": d, "item_bias": 1}
    if opt is None:
        dense = [c.inout(np.zeros((N_ITEMS, width.get(k, R)), f32), "G" + k) for k in ITEM_TABLES]
        c.eng.slrc_item_update(keys, perm, heads, n_heads, gpred, hgrad, U, d_uid, dense_grad=dense)
        return dict(zip(ITEM_TABLES, dense))
    W = [c.table(_n(rng, N_ITEMS, width.get(k, R)), k, iid) for k in ITEM_TABLES]
    m = [c.table(np.abs(_n(rng, N_ITEMS, width.get(k, R), sd=0.01)), "m" + k, iid) for k in ITEM_TABLES] if opt != "SGD" else None
    v = [c.table(np.abs(_n(rng, N_ITEMS, width.get(k, R), sd=0.01)) ** 2, "v" + k, iid) for k in ITEM_TABLES] if opt == "Adam" else None
    c.eng.slrc_item_update(keys, perm, heads, n_heads, gpred, hgrad, U, d_uid, hyper=c.eng.make_hyper(opt, lr=0.01, l2=1e-4, step=3),
                           W=W, m=m, v=v)
    return {"W": W, "m": m, "v": v}


case_slrc_item_update.item_update_shape = lambda d, R, opt: (37 * 9, d)


@case(("rc_slrc_user_bias_update", "rc_sort_ids"), [(1, None), (37, None), (37, "SGD"), (300, "Adam"), (37, "Adagrad")])
def case_slrc_user_bias(c, B, opt):
    rng = np.random.default_rng(B)
    uid = _ids(rng, 0, N_USERS, B)
    uid[0], uid[-1] = N_USERS - 1, 0
    keys, perm = c.eng.sort_ids(c.put(uid, "uid"), N_USERS)
    ubgrad = c.put(_n(rng, B), "ubgrad")
    if opt is None:
        G_ = c.inout(np.zeros((N_USERS, 1), f32), "Gub")
        c.eng.slrc_user_bias_update(keys, perm, ubgrad, dense_grad=G_)
        return {"G": G_}
    W = c.table(_n(rng, N_USERS, 1), "user_bias", uid)
    m = c.table(np.abs(_n(rng, N_USERS, 1, sd=0.01)), "m", uid) if opt != "SGD" else None
    v = c.table(np.abs(_n(rng, N_USERS, 1, sd=0.01)) ** 2, "v", uid) if opt == "Adam" else None
    c.eng.slrc_user_bias_update(keys, perm, ubgrad, hyper=c.eng.make_hyper(opt, lr=0.01, l2=1e-4, step=3), user_bias=W, m=m, v=v)
    return {"W": W, "m": m, "v": v}


@case(("rc_slrc_fwd_bwd", "rc_slrc_item_update", "rc_slrc_user_bias_update", "rc_sort_ids", "rc_segment_heads", "rc_segmented_update",
       "rc_reduce_sum", "rc_dense_update"),
      [(16, 1, "SGD", 3, 5), (64, 3, "Adam", 7, 100), (64, 3, "Adagrad", 5, 101), (128, 8, "SGD", 33, 10)])
def case_slrc_trainer(c, d, R, opt, B, Cn):
    rng = np.random.default_rng(d + B)
    uid, iid, iv = _batch(rng, B, Cn, R, hot=True)
    touched = {k: (uid if k in ("U", "user_bias") else iid) for k in c.eng.SLRC_PARAMS}
    P = _params(c, rng, d, R, touched=touched)
    ids = [c.put(x, n) for x, n in zip((uid, iid, iv), ("uid", "iid", "intervals"))]
    tr = c.eng.SlrcTrainer(*P, opt=opt, lr=0.01, l2=1e-4)
    losses = [tr.step(*ids).clone() for _ in range(2)]
    res = dict(zip(c.eng.SLRC_PARAMS, P))
    res["loss"] = c.eng.reduce_sum(torch.cat(losses), 1.0)
    for k in c.eng.SLRC_PARAMS:
        res.update({f"{n}_{k}": t for n, t in tr.state[k].items()})
    return res


case_slrc_trainer.item_update_shape = lambda d, R, opt, B, Cn: (B * Cn, d)
