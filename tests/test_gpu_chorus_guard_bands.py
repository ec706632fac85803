"""GPU: every Chorus engine wrapper runs once on torch's allocator and once between guard bands -- inputs, outputs and workspaces
served from tests/guarded.py's arena and allocator stand-in, every view ending on the first band byte, the workspaces exactly the
bytes rc_chorus_front_workspace_bytes / rc_chorus_category_update_workspace_bytes declare.  The second run must leave every band,
every input and every table row outside the batch bit-identical, return finite values and return the first run's bits.  The protocol
is tests/test_gpu_guard_bands.py's, as tests/test_gpu_slrc_guard_bands.py applies it; the cases live in this module's OWN list, the
table is tests/chorus_guard_table.py."""
import numpy as np
import pytest
import torch

import chorus_guard_table as CHT
import guard_table as T
import guarded as G
import slrc_guard_table as ST
from test_gpu_guard_bands import Placer, _flat, _ids, _n

pytestmark = pytest.mark.gpu

ARENA_BYTES = 64 << 20
f32 = np.float32
CASES = []
REACHED = {}        # case function -> [cases run, entry points called between the bands]
KINDS = {1: [0], 3: [0, 1, 2], 8: [0, 1, 2, 0, 2, 1, 1, 2]}


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
def test_chorus_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
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
    stray = sorted(set(called) - set(T.GUARDED) - set(ST.GUARDED) - set(CHT.GUARDED))
    assert not stray, f"{what}: reached entry points that no guard table lists as guarded: {stray}"
    REACHED.setdefault(fn.__name__, [0, set()])
    REACHED[fn.__name__][0] += 1
    REACHED[fn.__name__][1].update(called)
    arena.check(tables=c.tables)        # bands, inputs, and table rows outside the batch
    lib = eng._lib.load()
    for tag, asked, buf in served.workspaces:
        assert arena.contains(buf), f"{what}: workspace '{tag}' escaped the arena"
        assert buf.numel() == max(asked, 256), f"{what}: workspace '{tag}' has {buf.numel()} bytes for a declaration of {asked}"
    if "rc_chorus_fwd_bwd" in called or "rc_chorus_scores_bwd" in called:
        asked = [n for tag, n, _ in served.workspaces if tag == "chorus_front"]
        assert asked and all(n == lib.rc_chorus_front_workspace_bytes(*fn.front_shape(*params)) for n in asked)
    if "rc_chorus_category_update" in called:
        asked = [n for tag, n, _ in served.workspaces if tag == "chorus_cat"]
        assert asked and all(n == lib.rc_chorus_category_update_workspace_bytes(*fn.category_shape(*params)) for n in asked)
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

N_USERS, N_ITEMS, N_CAT = 23, 301, 19


def _params(c, rng, d, R, n_cat=N_CAT, touched=None):
    """the nine parameters in engine.CHORUS_PARAMS order: inputs, or (touched = {name: rows | None}) tables updated in place.  The last
    category's row ends each category table: a read past it would land on a band."""
    shapes = {"U": (N_USERS, d), "I": (N_ITEMS, d), "Rel": (R, d), "w": (1, d), "user_bias": (N_USERS, 1), "item_bias": (N_ITEMS, 1)}
    out = []
    for name in c.eng.CHORUS_PARAMS:
        x = np.asarray(_n(rng, *shapes.get(name, (n_cat, R)), sd=0.2))
        if name == "betas" and n_cat >= 5:
            x[0, 0], x[1, R - 1], x[2, 0], x[3, R - 1] = -1.5, 9.0, 11.0, -0.8     # below, at and above the clamp; a kernel beyond +-1
        if name == "sigmas" and n_cat >= 5:
            x[3, 0], x[4, R - 1], x[2, R - 1] = -1.5, 9.0, 11.0
        if touched is None or isinstance(touched.get(name, "in"), str):      # "in": the step must leave it bit-identical
            out.append(c.put(x, name))
        elif touched[name] is None:
            out.append(c.inout(x, name))
        else:
            out.append(c.table(x, name, touched[name]))
    return out


def _batch(rng, B, Cn, R, n_cat=N_CAT, hot=False):
    uid, iid, cid = _ids(rng, 0, N_USERS, B), _ids(rng, 0, N_ITEMS, B, Cn), _ids(rng, 0, n_cat, B, Cn)
    if hot:      # a category with most of the occurrences beside rare ones
        cid.reshape(-1)[: cid.size // 2] = min(2, n_cat - 1)
    iid[0, -1], iid[-1, 0], cid[0, -1], cid[-1, 0] = N_ITEMS - 1, 0, n_cat - 1, 0
    iv = np.where(rng.random((B, Cn, R)) < 0.4, -1.0, rng.uniform(0, 3, (B, Cn, R))).astype(f32)
    iv[0, 0, 0] = 0.0
    return uid, iid, cid, iv


# every width; R = 1, 3, 8; B on both sides of the 16 tuples of a workgroup; C = 1 (scores and the given-gradient backward only), odd,
# 100 and past a thousand; BPR and GMF
@case(("rc_chorus_scores", "rc_chorus_fwd_bwd", "rc_chorus_scores_bwd"),
      [(16, 1, 1, 2, 0), (16, 3, 17, 5, 1), (32, 3, 3, 5, 0), (32, 8, 15, 33, 1), (64, 3, 7, 100, 0), (64, 3, 17, 101, 1),
       (64, 1, 33, 65, 0), (128, 8, 5, 33, 0), (128, 3, 2, 51, 1), (64, 3, 3, 1, 0), (128, 8, 3, 1, 1), (64, 3, 2, 1031, 0)])
def case_chorus_front(c, d, R, B, Cn, gmf):
    rng = np.random.default_rng(d + R + B + Cn)
    P = _params(c, rng, d, R)
    uid, iid, cid, iv = _batch(rng, B, Cn, R)
    ids = [c.put(x, n) for x, n in zip((uid, iid, cid, iv), ("uid", "iid", "cid", "intervals"))]
    kinds = KINDS[R]
    res = {"scores": c.eng.chorus_scores(P, *ids, kinds, bool(gmf))}
    res["bwd"] = c.eng.chorus_scores_grads(P, *ids, kinds, c.put(_n(rng, B, Cn), "gpred"), bool(gmf))
    if Cn == 1:      # the fused step needs a negative: the same column twice
        ids[1:] = [c.put(np.concatenate([x, x], axis=1), n + "2") for x, n in zip((iid, cid, iv), ("iid", "cid", "intervals"))]
    res["fused"] = c.eng.chorus_fwd_bwd(P, *ids, kinds, bool(gmf))
    res["fused_nopred"] = c.eng.chorus_fwd_bwd(P, *ids, kinds, bool(gmf), want_pred=False)
    return res


case_chorus_front.front_shape = lambda d, R, B, Cn, gmf: (B, d, R)


# n_occ on both sides of the piece size; one category owning everything, every occurrence its own, a hot mix
@case(("rc_chorus_category_update", "rc_sort_ids", "rc_segment_heads"),
      [(n, R, mode, opt) for n, R, mode in ((1, 3, "one"), (1023, 1, "one"), (1024, 3, "mix"), (1025, 8, "one"), (3079, 3, "mix"),
                                            (1025, 3, "own"), (3079, 8, "mix")) for opt in (None, "Adam")] +
      [(2049, 3, "mix", "SGD"), (2049, 3, "one", "Adagrad")])
def case_chorus_category_update(c, n, R, mode, opt):
    rng = np.random.default_rng(n + R)
    n_cat = case_chorus_category_update.category_shape(n, R, mode, opt)[1]
    cid = np.zeros(n, np.int64) if mode == "one" else (rng.permutation(n).astype(np.int64) if mode == "own" else _ids(rng, 0, n_cat, n))
    if mode == "mix":
        cid[: n // 2], cid[-1] = 2, n_cat - 1
    kgrad = c.put(_n(rng, n, 3 * R), "kgrad")
    keys, perm = c.eng.sort_ids(c.put(cid, "cid"), n_cat)
    _, heads, n_heads = c.eng.segment_heads(keys, perm, want_single=False)
    names = c.eng.CHORUS_CAT_TABLES
    if opt is None:
        dense = [c.inout(np.zeros((n_cat, R), f32), "G" + k) for k in names]
        c.eng.chorus_category_update(keys, perm, heads, n_heads, kgrad, n_cat, dense_grad=dense)
        return dict(zip(names, dense))
    W = [c.table(_n(rng, n_cat, R), k, cid) for k in names]
    m = [c.table(np.abs(_n(rng, n_cat, R, sd=0.01)), "m" + k, cid) for k in names] if opt != "SGD" else None
    v = [c.table(np.abs(_n(rng, n_cat, R, sd=0.01)) ** 2, "v" + k, cid) for k in names] if opt == "Adam" else None
    c.eng.chorus_category_update(keys, perm, heads, n_heads, kgrad, n_cat, hyper=c.eng.make_hyper(opt, lr=0.01, l2=1e-4, step=3),
                                 W=W, m=m, v=v)
    return {"W": W, "m": m, "v": v}


case_chorus_category_update.category_shape = lambda n, R, mode, opt: (n, {"one": 1, "own": n, "mix": N_CAT}[mode], R)


@case(("rc_chorus_fwd_bwd", "rc_chorus_category_update", "rc_slrc_user_bias_update", "rc_sort_ids", "rc_segment_heads",
       "rc_segmented_update", "rc_reduce_sum", "rc_dense_update"),
      [(16, 1, "SGD", 3, 5, 0), (64, 3, "Adam", 17, 100, 0), (64, 3, "Adagrad", 5, 101, 1), (128, 8, "SGD", 33, 40, 1)])
def case_chorus_trainer(c, d, R, opt, B, Cn, gmf):
    rng = np.random.default_rng(d + B)
    uid, iid, cid, iv = _batch(rng, B, Cn, R, hot=True)
    kinds = KINDS[R]
    sub = 2 in kinds
    touched = {"U": uid, "I": iid, "Rel": None, "betas": cid, "mus": cid if sub else "in", "sigmas": cid if sub else "in",
               "w": None if gmf else "in", "user_bias": "in" if gmf else uid, "item_bias": "in" if gmf else iid}
    P = _params(c, rng, d, R, touched=touched)
    ids = [c.put(x, n) for x, n in zip((uid, iid, cid, iv), ("uid", "iid", "cid", "intervals"))]
    tr = c.eng.ChorusTrainer(*P, kinds=kinds, gmf=bool(gmf), opt=opt, lr=0.01, l2=1e-4, lr_scale=0.1)
    losses = [tr.step(*ids).clone() for _ in range(2)]
    res = dict(zip(c.eng.CHORUS_PARAMS, P))
    res["loss"] = c.eng.reduce_sum(torch.cat(losses), 1.0)
    for k in c.eng.CHORUS_PARAMS:
        res.update({f"{n}_{k}": t for n, t in tr.state[k].items()})
    return res


case_chorus_trainer.front_shape = lambda d, R, opt, B, Cn, gmf: (B, d, R)
case_chorus_trainer.category_shape = lambda d, R, opt, B, Cn, gmf: (B * Cn, N_CAT, R)
