"""GPU: every entry point the engine marshals runs once on torch's allocator and once between guard bands (tests/guarded.py), and the
second run must (a) leave every band and every input bit-identical, (b) have taken every output and every workspace from the
arena -- the workspace at exactly the size the entry point's own *_workspace_bytes function declares --, (c) return finite values
and (d) return the first run's bits.  Values are not re-derived here: each family's float64 test does that; this file ties where a
kernel writes, how far it reads and how much scratch it uses to those already-pinned results.

A case is a function of a placer `c`: it builds its inputs from a seeded generator, places each with c.put / c.table / c.inout (a
fresh device tensor on the first run, an arena view on the second), calls the engine wrapper and returns the results.  Result keys
that start with "~" are held to the arena only (buffers that are partly unspecified by contract, or whose record ORDER is decided by
an integer ticket: tests/guard_table.py names the atomic), keys that start with "=" to bit equality only (canonical forms of those).
RC_GUARD_REPORT=<file>: every case appends its line of profiles/guard_bands.txt."""
import os
import time

import numpy as np
import pytest
import torch

import guard_table as T
import guarded as G

pytestmark = pytest.mark.gpu

ARENA_BYTES = 256 << 20
f32 = np.float32


@pytest.fixture(scope="module")
def arena(cuda):
    a = G.Arena(cuda, ARENA_BYTES)
    yield a
    del a


@pytest.fixture(scope="module")
def eng(cuda):
    from rechorus_amd import engine
    return engine


class Placer:
    """arena None: plain device tensors (the unguarded run); else arena views with the input's bits kept for arena.check()"""

    def __init__(self, eng, dev, arena=None):
        self.eng, self.dev, self.arena = eng, dev, arena
        self.tables = {}
        self.names = set()

    def put(self, x, name, kind="in"):
        if x is None:
            return None
        assert name not in self.names, name
        self.names.add(name)
        x = torch.as_tensor(x)
        if self.arena is None:
            return x.to(self.dev).contiguous().clone()
        return self.arena.put(x.contiguous(), name, kind)

    def table(self, x, name, rows):
        """a table the call updates in place: only `rows` (indices of its first dimension) may change"""
        self.tables[name] = np.unique(np.asarray(rows).reshape(-1))
        return self.put(x, name, "table")

    def inout(self, x, name):
        return self.put(x, name, "inout")

    def scratch(self, shape, name):
        """an uninitialised float buffer a caller outside engine.py owns (rechorus_amd/lgcn.py's propagation buffers)"""
        if self.arena is None:
            return torch.empty(shape, dtype=torch.float32, device=self.dev)
        return self.arena.take(shape, torch.float32, name, "out")

    def seed(self, value, name="seed"):
        return self.put(np.array([value], dtype=np.int64), name)


CASES = []
REACHED = {}        # case function -> [cases run, entry points called between the bands]


def case(entries, params, allocates=True, nonfinite_ok=()):
    """register a case function for every parameter tuple; entries: the C entry points it reaches (held against guard_table.GUARDED)"""
    def deco(fn):
        fn.entries, fn.allocates, fn.nonfinite_ok = tuple(entries), allocates, tuple(nonfinite_ok)
        for p in params:
            p = p if isinstance(p, tuple) else (p,)
            CASES.append(pytest.param(fn, p, id=fn.__name__[5:] + "-" + "-".join(str(x).replace(" ", "") for x in p)))
        return fn
    return deco


def _flat(x, path=""):
    if x is None:
        return []
    if torch.is_tensor(x):
        return [(path, x)]
    if isinstance(x, dict):
        return [p for k in x for p in _flat(x[k], f"{path}.{k}" if path else str(k))]
    if isinstance(x, (list, tuple)):
        return [p for k, v in enumerate(x) for p in _flat(v, f"{path}[{k}]")]
    return [(path, x)]


def _record(line):
    path = os.environ.get("RC_GUARD_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("fn,params", CASES)
def test_guard_bands(fn, params, cuda, eng, arena, monkeypatch):
    t0 = time.perf_counter()
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
            _record(f"{what}: FAULT {str(e).splitlines()[0]}")
            pytest.exit(f"GPU fault in {what}: {str(e).splitlines()[0]}", returncode=3)
        raise
    stray = sorted(set(called) - set(T.GUARDED))
    assert not stray, f"{what}: reached entry points that tests/guard_table.py does not list as guarded: {stray}"
    REACHED.setdefault(fn.__name__, [0, set()])
    REACHED[fn.__name__][0] += 1
    REACHED[fn.__name__][1].update(called)
    what += " [" + " ".join(dict.fromkeys(called)) + "]"
    try:
        arena.check(tables=c.tables)
    except G.GuardError as e:
        _record(f"{what}: FINDING {e}")
        raise
    # every workspace came from the arena at exactly the declared size (engine.workspace() has always rounded up to 256 bytes)
    for tag, asked, buf in served.workspaces:
        assert arena.contains(buf), f"{what}: workspace '{tag}' escaped the arena"
        assert buf.numel() == max(asked, 256), f"{what}: workspace '{tag}' has {buf.numel()} bytes for a declaration of {asked}"
    if fn.allocates:
        assert served.count > 0, f"{what}: the wrapper allocated nothing from the arena -- the case has tested nothing"
    else:
        assert served.count == 0, f"{what}: declared as allocating nothing, but {served.count} allocations were served"
    a, b = _flat(plain), _flat(got)
    assert [p for p, _ in a] == [p for p, _ in b] and len(b) > 0, what
    n_in_arena = 0
    for (path, x), (_, y) in zip(a, b):
        arena_only, equal_only = path.startswith("~"), path.startswith("=")
        if not torch.is_tensor(y):
            assert x == y, f"{what}: {path}: {x!r} != {y!r}"
            continue
        if not equal_only:
            assert arena.contains(y), f"{what}: result '{path}' {tuple(y.shape)} escaped the arena"
            n_in_arena += 1
            if y.dtype.is_floating_point and not arena_only and path not in fn.nonfinite_ok:
                assert bool(torch.isfinite(y).all()), f"{what}: result '{path}' is not finite ({int((~torch.isfinite(y)).sum())} elements)"
        if not arena_only:
            assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {path}"
            same = torch.equal(G._bytes(x.contiguous()), G._bytes(y.contiguous()))
            if not same:
                diff = (x != y) if not x.dtype.is_floating_point else ~((x == y) | (torch.isnan(x) & torch.isnan(y)))
                raise AssertionError(f"{what}: '{path}' differs between the plain and the guarded run: {int(diff.sum())} of {x.numel()} elements")
    assert n_in_arena > 0, what
    _record(f"{what}: outputs {served.output_bytes} B, workspace declared {served.scratch_bytes} B, {served.count} arena allocations, "
            f"clean ({time.perf_counter() - t0:.3f} s)")


def test_every_entry_point_a_case_claims_was_called_between_the_bands():
    """runs after the cases (same module, file order): a case function that ran all its cases called every entry point it is listed
    for in tests/guard_table.py at least once -- a wrapper that stops reaching a kernel cannot leave its row of the table green"""
    n_cases = {}
    for p in CASES:
        n_cases[p.values[0].__name__] = n_cases.get(p.values[0].__name__, 0) + 1
    fns = {p.values[0].__name__: p.values[0] for p in CASES}
    for name, (ran, called) in REACHED.items():
        if ran == n_cases[name]:
            missing = sorted(set(fns[name].entries) - called)
            assert not missing, f"{name} never called {missing}"


def test_the_bands_see_a_kernel_that_is_told_one_row_too_many(cuda, eng, arena):
    """the harness on the device, with real kernels: rc_gather_rows told n + 1 rows stores one row past a [7, 5] output -- 20 bytes,
    reported at +0 .. +19 --, and rc_reduce_sum told n + 1 elements keeps the band's NaN.  Both stay inside the arena's own
    allocation (the bands are 64 KiB of it); the same calls with the true counts are clean."""
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())
    for n_told, dirty in ((7, False), (8, True)):
        arena.reset()
        W = arena.put(torch.arange(50, dtype=torch.float32).view(10, 5) + 1, "W")
        ids = arena.put(torch.tensor([3, 1, 4, 1, 5, 9, 2, 6], dtype=torch.int64), "ids")
        out = arena.take((7, 5), torch.float32, "out")
        eng._lib.call("rc_gather_rows", p(W), 5, p(ids), n_told, p(out), eng._stream())
        x = arena.put(torch.ones(35), "x")
        total = arena.take((1,), torch.float32, "total")
        eng._lib.call("rc_reduce_sum", p(x), 35 + int(dirty), 1.0, p(total), eng._stream())
        torch.cuda.synchronize()
        assert torch.equal(out, W[ids[:7]])
        if dirty:
            with pytest.raises(G.GuardError, match=r"after 'out' \(out, 140 bytes\) is dirty: 20 bytes, bytes \+0 \.\. \+19 past the tensor's end"):
                arena.check()
            assert bool(torch.isnan(total).all())
        else:
            arena.check()
            assert total.item() == 35.0


# ---- helpers ---------------------------------------------------------------------------------------------------------------------

def _n(rng, *shape, sd=1.0):
    return rng.normal(0, sd, shape).astype(f32)


def _ids(rng, lo, hi, *shape):
    return rng.integers(lo, hi, size=shape).astype(np.int64)


def _hist(rng, B, L, n_items):
    """right-padded histories with lengths in [1, L], the first at full length -> (hist, lengths)"""
    lengths = rng.integers(1, L + 1, B).astype(np.int64)
    lengths[0] = L
    hist = _ids(rng, 1, n_items, B, L) * (np.arange(L)[None, :] < lengths[:, None])
    return hist.astype(np.int64), lengths


def _canon_records(rows, occ):
    """rc_bucket_plan's records (row, start, n, 0) and grouped positions in a canonical form: rows ascending, each with its positions"""
    r = rows.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    o = occ.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    out = []
    for row, start, n, _ in r[np.argsort(r[:, 0], kind="stable")] if len(r) else []:
        out += [row, n] + o[start:start + n].tolist()
    return torch.tensor(out, dtype=torch.int64)


# ---- dense layers ----------------------------------------------------------------------------------------------------------------

@case(("rc_linear_fwd", "rc_linear_bwd"),
      [(M, N, K, relu, p) for M, N, K in ((1, 1, 1), (3, 5, 7), (65, 63, 17), (257, 130, 66), (5000, 2, 20)) for relu, p in ((False, 0.0), (True, 0.3))])
def case_linear(c, M, N, K, relu, p):
    rng = np.random.default_rng(M * 131 + N * 17 + K)
    X, W, b, dY = c.put(_n(rng, M, K), "X"), c.put(_n(rng, N, K, sd=0.2), "W"), c.put(_n(rng, N), "b"), c.put(_n(rng, M, N), "dY")
    seed = c.seed(1234567 + M) if p > 0 else None
    Y = c.eng.linear_fwd(X, W, b, relu, p, seed, site=2)
    dX, dW, db = c.eng.linear_bwd(X, W, Y if relu else None, dY, drop_p=p)
    res = {"Y": Y, "dX": dX, "dW": dW, "db": db}
    if (M, N, K) == (65, 63, 17):
        none_x, res["dW_alone"], none_b = c.eng.linear_bwd(X, W, Y if relu else None, dY, drop_p=p, need_dx=False, need_db=False)
        assert none_x is None and none_b is None
    return res


@case(("rc_tower_tail_fwd", "rc_tower_tail_bwd"), [(1, 64, 16, 0.0), (37, 128, 32, 0.5), (513, 512, 16, 0.1)])
def case_tower_tail(c, M, K, N2, p2):
    rng = np.random.default_rng(M + K + N2)
    assert c.eng.tower_tail_supported(M, K, N2)
    X = np.where(rng.random((M, K)) < 0.45, 0.0, np.abs(_n(rng, M, K, sd=0.5))).astype(f32)
    X, W2, b2, w3, b3 = c.put(X, "X"), c.put(_n(rng, N2, K, sd=0.1), "W2"), c.put(_n(rng, N2, sd=0.1), "b2"), c.put(_n(rng, 1, N2, sd=0.3), "w3"), c.put(_n(rng, 1, sd=0.1), "b3")
    dz = c.put(_n(rng, M, 1), "dz")
    seed = c.seed(123456789 + (M << 33)) if p2 > 0 else None
    H2, z = c.eng.tower_tail_fwd(X, W2, b2, w3, b3, p2, seed, 1)
    grads = c.eng.tower_tail_bwd(X, W2, w3, H2, dz, p2, need_dx=True, x_act=True, x_drop_p=0.2)
    return {"H2": H2, "z": z, "grads": grads}


# ---- sequence layers -------------------------------------------------------------------------------------------------------------

@case(("rc_seq_attention_fwd", "rc_seq_attention_bwd", "rc_seq_offsets"),
      [(1, 1, 1, 4, "causal"), (2, 9, 5, 3, "causal"), (3, 70, 3, 20, "causal+len"), (2, 33, 4, 8, "batchmask")])
def case_seq_attention(c, B, L, H, dk, kind):
    rng = np.random.default_rng(B * 1000 + L)
    D = H * dk
    q, k, v, w = (_n(rng, B * L, D) for _ in range(4))
    lengths = rng.integers(1, L + 1, B).astype(np.int64) if "len" in kind else np.full(B, L, dtype=np.int64)
    lengths[0] = L
    valid = (np.arange(L)[None, :] < lengths[:, None]).reshape(-1)
    off = c.eng.seq_offsets(c.put(lengths, "lengths"), L) if "len" in kind else None
    mask = None
    if "mask" in kind:
        m = rng.random((B, L, L)) < 0.7
        m[:, L // 2, :] = False          # a row that sees nothing
        mask = c.put(m.astype(np.uint8), "mask")
    Q, K, V = c.put(q, "Q"), c.put(k, "K"), c.put(v, "V")
    dctx = c.put(w * valid[:, None], "dctx")
    ctx, lse = c.eng.seq_attention_fwd(Q, K, V, off, B, L, H, mask=mask, causal="causal" in kind)
    dQ, dK, dV = c.eng.seq_attention_bwd(Q, K, V, off, B, L, H, lse, dctx, mask=mask, causal="causal" in kind)
    return {"off": off, "ctx": ctx, "lse": lse, "dQ": dQ, "dK": dK, "dV": dV}


@case(("rc_seq_add_layernorm_fwd", "rc_seq_add_layernorm_bwd"), [(7, 48, 0.5), (50, 64, 0.0), (333, 128, 0.3)])
def case_seq_add_layernorm(c, rows, d, p):
    rng = np.random.default_rng(rows + d)
    L = 10 if rows % 10 == 0 else 1
    B = rows // L
    lengths = rng.integers(1, L + 1, B).astype(np.int64)
    lengths[0] = L
    off = c.eng.seq_offsets(c.put(lengths, "lengths"), L) if L > 1 else None
    A, R, w, b, dy = c.put(_n(rng, rows, d), "A"), c.put(_n(rng, rows, d), "R"), c.put(1 + 0.1 * _n(rng, d), "w"), c.put(0.1 * _n(rng, d), "b"), c.put(_n(rng, rows, d), "dy")
    seed = c.seed(123456789) if p > 0 else None
    res = {}
    for with_r in (True, False):
        Y, xhat, rstd = c.eng.seq_add_layernorm_fwd(A, R if with_r else None, w, b, off, L, p, seed, 3)
        dA, dR, dw, db = c.eng.seq_add_layernorm_bwd(dy, xhat, rstd, w, off, L, p, seed, 3, need_dR=with_r)
        res[f"r{int(with_r)}"] = {"Y": Y, "xhat": xhat, "rstd": rstd, "dA": dA, "dR": dR, "dw": dw, "db": db}
    return res


@case(("rc_seq_offsets", "rc_seq_embed_fwd", "rc_seq_pick_last_fwd", "rc_seq_pick_last_bwd", "rc_seq_pos_grad"), [(4, 1, 20), (9, 13, 64), (300, 50, 6)])
def case_seq_rest(c, B, L, d):
    rng = np.random.default_rng(3 + B)
    hist, lengths = _hist(rng, B, L, 40)
    I, P = c.put(_n(rng, 40, d), "item_emb"), c.put(_n(rng, L + 1, d), "pos_emb")
    h, n = c.put(hist, "hist"), c.put(lengths, "lengths")
    X = c.eng.seq_embed(I, P, h, n)
    hv = c.eng.seq_pick_last(X, n, B, L)
    dX = c.eng.seq_pick_last_bwd(c.put(_n(rng, B, d), "dhv"), n, B, L)
    gx = c.put(_n(rng, B * L, d) * (hist > 0).reshape(-1, 1), "gx")
    return {"off": c.eng.seq_offsets(n, L), "X": X, "hv": hv, "dX": dX, "GP": c.eng.seq_pos_grad(gx, n, B, L, L + 3)}


@case(("rc_seq_embed_fwdpos_fwd", "rc_seq_pos_grad_fwdpos"), [(1, 4), (20, 64)])
def case_seq_fwdpos(c, L, d):
    rng = np.random.default_rng(L + d)
    B = 5
    hist, lengths = _hist(rng, B, L, 40)
    h, n = c.put(hist, "hist"), c.put(lengths, "lengths")
    X = c.eng.seq_embed_fwdpos(c.put(_n(rng, 40, d), "item_emb"), c.put(_n(rng, L + 2, d), "pos_emb"), h, n)
    gx = c.put(_n(rng, B * L, d) * (hist > 0).reshape(-1, 1), "gx")
    return {"X": X, "GP": c.eng.seq_pos_grad_fwdpos(gx, n, B, L, L + 2)}


# ---- SASRec encoders ------------------------------------------------------------------------------------------------------------

def _sasrec_problem(which):
    """-> (parameters by the reference's names, n_layers, n_heads, hist, lengths): the smallest golden case inside the encoders'
    envelope, or a random model at (d, layers, heads, L, B)"""
    import test_gpu_sasrec as TS
    from conftest import load_golden
    from test_oracle_sasrec import params
    if which == "golden":
        name = min(TS.CASES, key=lambda n: (load_golden(n)["hist"].size, n))
        g = load_golden(name)
        return params(g), int(g["meta"][2]), int(g["meta"][3]), g["hist"], g["len"]
    d, n_layers, n_heads, L, B = which
    rng = np.random.default_rng(d + L + B)
    P = TS._random_sasrec(rng, 60, d, n_layers, L)
    hist, lengths = _hist(rng, B, L, 60)
    return P, n_layers, n_heads, hist, lengths


@case(("rc_sasrec_fwd", "rc_sasrec_bwd", "rc_sasrec_batch_fwd", "rc_sasrec_batch_bwd", "rc_sasrec_batch_bwd_part", "rc_sasrec_pos_grad"),
      [(which, impl) for which in ("golden", (32, 1, 1, 7, 3), (64, 1, 2, 20, 90)) for impl in ("sequence", "batch", "batch-split")])
def case_sasrec(c, which, impl):
    import test_gpu_sasrec as TS
    P, n_layers, n_heads, hist, lengths = _sasrec_problem(which)
    B, L = hist.shape
    if L > 64 and impl == "sequence":      # more than 64 positions: the batch encoder only
        impl = "batch"
    item_emb, pos_emb = c.put(P["i_embeddings.weight"], "item_emb"), c.put(P["p_embeddings.weight"], "pos_emb")
    layers = [{k: c.put(np.ascontiguousarray(P["transformer_block.%d.%s" % (l, v)]), f"L{l}.{k}") for k, v in TS.LAYER_NAMES.items()}
              for l in range(n_layers)]
    h, n = c.put(hist, "hist"), c.put(lengths, "lengths")
    d = item_emb.shape[1]
    rng = np.random.default_rng(B)
    hv, saved = c.eng.sasrec_fwd(item_emb, pos_emb, layers, n_heads, h, n, save=True, impl=impl.split("-")[0])
    hv_eval, none = c.eng.sasrec_fwd(item_emb, pos_emb, layers, n_heads, h, n, save=False, impl=impl.split("-")[0])
    dhv = c.put(_n(rng, B, d), "dhv")
    if impl == "batch-split":
        g_hist, grads, finish = c.eng.sasrec_bwd(layers, n_heads, n, saved, dhv, split=True)
        finish()
    else:
        g_hist, grads = c.eng.sasrec_bwd(layers, n_heads, n, saved, dhv)
    # the saved state is the forward's scratch for its backward: what it holds past the rows the backward reads is unspecified
    return {"hv": hv, "hv_eval": hv_eval, "~saved": saved.data, "g_hist": g_hist, "grads": grads,
            "GP": c.eng.sasrec_pos_grad(g_hist, n, pos_emb.shape[0])}


# ---- BPRMF -----------------------------------------------------------------------------------------------------------------------

@case(("rc_gather_rows", "rc_gather_rows_pair", "rc_gather_dot_fwd", "rc_weighted_row_sum", "rc_bprmf_fwd_bwd"),
      [(64, 1, 2), (64, 7, 9), (64, 4, 33), (48, 7, 9), (128, 4, 33), (20, 3, 5)])
def case_gather(c, d, B, Cn):
    rng = np.random.default_rng(d + B + Cn)
    n_users, n_items = 23, 301
    U, I, I2 = c.put(_n(rng, n_users, d, sd=0.1), "U"), c.put(_n(rng, n_items, d, sd=0.1), "I"), c.put(_n(rng, n_items, d, sd=0.1), "I2")
    uid, iid = c.put(_ids(rng, 0, n_users, B), "uid"), c.put(_ids(rng, 0, n_items, B, Cn), "iid")
    coef = c.put(_n(rng, B, Cn), "coef")
    res = {"rows": c.eng.gather_rows(I, iid), "pair": c.eng.gather_rows_pair(I, I2, iid), "dot": c.eng.gather_dot(U, I, uid, iid),
           "wsum": c.eng.weighted_row_sum(I, iid, coef)}
    res["fused"] = c.eng.bprmf_fwd_bwd(U, I, uid, iid)            # (d = 48, 20: the LDS route)
    res["fused_nopred"] = c.eng.bprmf_fwd_bwd(U, I, uid, iid, want_pred=False)
    return res


@case(("rc_bpr_loss_fwd_bwd", "rc_reduce_sum"), [(1, 2), (7, 5), (259, 17), (65, 100)])
def case_bpr_loss(c, B, Cn):
    rng = np.random.default_rng(B + Cn)
    pred = c.put(_n(rng, B, Cn, sd=2.0), "pred")
    loss, loss_vec, gpred = c.eng.bpr_loss(pred)
    loss2, loss_vec2, none = c.eng.bpr_loss(pred, need_grad=False)
    return {"loss": loss, "loss_vec": loss_vec, "gpred": gpred, "loss2": loss2, "sum": c.eng.reduce_sum(pred.reshape(-1), 0.5)}


# ---- sort / segments ---------------------------------------------------------------------------------------------------------

@case(("rc_sort_ids", "rc_segment_heads"), [1, 257, 70001])
def case_sort(c, n):
    rng = np.random.default_rng(n)
    n_rows = 5000
    ids = _ids(rng, 0, n_rows, n)
    ids[: n // 3] = ids[: n // 3] % 7
    keys, perm = c.eng.sort_ids(c.put(ids, "ids"), n_rows)
    single, heads, n_heads = c.eng.segment_heads(keys, perm)
    single_m, heads_m, n_heads_m = c.eng.segment_heads(keys, perm, only_multi=True)
    canon = lambda hd, nh: torch.sort(hd[:int(nh.item())].cpu()).values
    return {"keys": keys, "perm": perm, "single": single, "~heads": heads, "n_heads": n_heads, "=heads": canon(heads, n_heads),
            "single_m": single_m, "~heads_m": heads_m, "n_heads_m": n_heads_m, "=heads_m": canon(heads_m, n_heads_m)}


def _opt_tables(c, rng, n_rows, d, opt, touched, tag=""):
    """(W, m, v) of one table as c.table views: only `touched` rows may change"""
    W = c.table(_n(rng, n_rows, d), "W" + tag, touched)
    m = c.table(np.abs(_n(rng, n_rows, d, sd=0.01)), "m" + tag, touched) if opt in ("Adam", "Adagrad") else None
    v = c.table(np.abs(_n(rng, n_rows, d, sd=0.01)) ** 2, "v" + tag, touched) if opt == "Adam" else None
    return W, m, v


@case(("rc_segmented_update",), [(d, opt) for d in (8, 16, 128) for opt in (None, "Adam")])
def case_segmented(c, d, opt):
    rng = np.random.default_rng(d)
    n_rows, n_src, n, div = 300, 50, 2000, 4
    ids = np.minimum(rng.zipf(1.3, size=n), n_rows - 1).astype(np.int64)          # hot rows
    keys, perm = c.eng.sort_ids(c.put(ids, "ids"), n_rows)
    src, coef = c.put(_n(rng, n_src, d), "src"), c.put(_n(rng, n), "coef")
    src_index = c.put(_ids(rng, 0, n_src, (n + div - 1) // div), "src_index")
    if opt is None:
        G_ = c.inout(np.zeros((n_rows, d), f32), "G")
        c.eng.segmented_update(keys, perm, src, coef=coef, src_index=src_index, div=div, dense_grad=G_)
        return {"G": G_}
    W, m, v = _opt_tables(c, rng, n_rows, d, opt, ids)
    c.eng.segmented_update(keys, perm, src, hyper=c.eng.make_hyper(opt, lr=0.01, l2=1e-4, step=3), W=W, m=m, v=v, coef=coef,
                           src_index=src_index, div=div)
    return {"W": W, "m": m, "v": v}


@case(("rc_segmented_update_pair",), [(d, opt) for d in (8, 16, 128) for opt in (None, "Adam")])
def case_segmented_pair(c, d, opt):
    rng = np.random.default_rng(d + 1)
    n_rows, n = 300, 1500
    assert c.eng.segmented_pair_supported(d)
    ids = np.minimum(rng.zipf(1.3, size=n), n_rows - 1).astype(np.int64)
    keys, perm = c.eng.sort_ids(c.put(ids, "ids"), n_rows)
    _, heads, n_heads = c.eng.segment_heads(keys, perm, want_single=False)
    ga, gb = c.put(_n(rng, n, d), "ga"), c.put(_n(rng, n, d), "gb")
    if opt is None:
        Ga, Gb = c.inout(np.zeros((n_rows, d), f32), "Ga"), c.inout(np.zeros((n_rows, d), f32), "Gb")
        c.eng.segmented_update_pair(keys, perm, ga, gb, dense_grad=(Ga, Gb), heads=heads, n_heads=n_heads)
        return {"Ga": Ga, "Gb": Gb}
    Wa, ma, va = _opt_tables(c, rng, n_rows, d, opt, ids, "a")
    Wb, mb, vb = _opt_tables(c, rng, n_rows, d, opt, ids, "b")
    c.eng.segmented_update_pair(keys, perm, ga, gb, hyper=c.eng.make_hyper(opt, lr=0.01, l2=1e-4, step=3), W=(Wa, Wb), m=(ma, mb), v=(va, vb),
                                heads=heads, n_heads=n_heads)
    return {"Wa": Wa, "ma": ma, "va": va, "Wb": Wb, "mb": mb, "vb": vb}


def _rows_problem(rng, d, n_rows, n_a, Cn, n_b):
    ids_a = _ids(rng, 0, n_rows, n_a, Cn)
    ids_a[ids_a == 3] = 4                       # row 3 never occurs
    ids_b = _ids(rng, 0, n_rows, n_b)
    ids_b[ids_b == 3] = 5
    ids_b[: n_b // 3] = 7                       # a hot row (chunked path)
    return ids_a, ids_b


@case(("rc_segmented_update_rows",), [(16, 50, 600, 3, 700, "SGD"), (64, 97, 2000, 4, 1500, "Adam"), (128, 40, 900, 2, 0, None)])
def case_segmented_rows(c, d, n_rows, n_a, Cn, n_b, opt):
    rng = np.random.default_rng(d + n_rows)
    ids_a, ids_b = _rows_problem(rng, d, n_rows, n_a, Cn, n_b)
    ids = np.concatenate([ids_a.reshape(-1), ids_b])
    assert c.eng.seg_rows_route(len(ids), n_rows, d)
    keys, perm = c.eng.sort_ids(c.put(ids, "ids"), n_rows)
    coef, src, src2 = c.put(_n(rng, n_a * Cn), "coef"), c.put(_n(rng, n_a, d), "src"), c.put(_n(rng, max(n_b, 1), d), "src2")
    if opt is None:
        G_ = c.inout(np.zeros((n_rows, d), f32), "G")
        c.eng.segmented_update2(keys, perm, src, src2, n_a * Cn, coef=coef, div=Cn, dense_grad=G_)
        return {"G": G_}
    W, m, v = _opt_tables(c, rng, n_rows, d, opt, ids)
    c.eng.segmented_update2(keys, perm, src, src2, n_a * Cn, hyper=c.eng.make_hyper(opt, lr=0.01, l2=1e-4, step=3), W=W, m=m, v=v, coef=coef, div=Cn)
    return {"W": W, "m": m, "v": v}


@case(("rc_rows_plan_build", "rc_rows_plan_update", "rc_rows_plan_views"), [(16, 50, 200, 3, 4, "SGD"), (64, 97, 500, 4, 3, "Adam"), (128, 40, 450, 2, 0, None)])
def case_rows_plan(c, d, n_rows, B, Cn, L, opt):
    rng = np.random.default_rng(d + n_rows + B)
    ids_a = _ids(rng, 1, n_rows, B, Cn)
    ids_a[ids_a == 3] = 4
    ids_a[: B // 3, 0] = 7
    lengths = rng.integers(0, L + 1, size=B).astype(np.int64)
    hist = _ids(rng, 1, n_rows, B, max(L, 1))[:, :L]
    hist[hist == 3] = 5
    hist = (hist * (np.arange(L)[None, :] < lengths[:, None])).astype(np.int64)
    n_b = B * L
    assert c.eng.rows_plan_supported(n_rows, B * Cn + n_b, d)
    rp = c.eng.RowsPlan(c.put(ids_a, "ids_a"), c.put(hist, "hist") if L else None, c.put(lengths, "lengths") if L else None, n_rows, d, tag="guard_rows_plan")
    views = rp.views()
    src2 = _n(rng, max(n_b, 1), d)
    src2[:n_b][(np.arange(L)[None, :] >= lengths[:, None]).reshape(-1)] = 0
    coef, src, src2 = c.put(_n(rng, B * Cn), "coef"), c.put(_n(rng, B, d), "src"), c.put(src2, "src2")
    touched = np.concatenate([ids_a.reshape(-1), hist.reshape(-1)])
    res = {"~ws": rp.ws, "=start": views[2], "=end": views[3], "=status": views[4]}
    if opt is None:
        res["G"] = c.inout(np.zeros((n_rows, d), f32), "G")
        rp.update(src, coef=coef, div=Cn, src2=src2, dense_grad=res["G"])
        return res
    W, m, v = _opt_tables(c, rng, n_rows, d, opt, touched)
    rp.update(src, hyper=c.eng.make_hyper(opt, lr=0.01, l2=1e-4, step=3), W=W, m=m, v=v, coef=coef, div=Cn, src2=src2)
    res.update(W=W, m=m, v=v)
    return res


# ---- narrow tables / small route ---------------------------------------------------------------------------------------------

@case(("rc_segmented_update",), [(3, 50, 2048, 0.9), (1, 300, 70000, 0.5)])
def case_narrow_tiles(c, d, n_rows, n, hot):
    rng = np.random.default_rng(d * 1000 + n_rows)
    ids = _ids(rng, 0, n_rows, n)
    ids[rng.random(n) < hot] = n_rows // 2
    return {"G": c.eng.embedding_dense_backward(c.put(_n(rng, n, d), "go"), c.put(ids, "ids"), n_rows, route="sort")}


@case(("rc_small_row_sums", "rc_small_row_sums_planned"), [(d, n_rows, n) for d in (1, 2, 3, 4, 32) for n_rows, n in ((50, 1), (300, 2049))])
def case_small_row_sums(c, d, n_rows, n):
    rng = np.random.default_rng(d + n)
    assert c.eng.small_route_ok(n, n_rows, d)
    ids = c.put(_ids(rng, 0, n_rows, n), "ids")
    G1 = c.eng.embedding_dense_backward(c.put(_n(rng, n, d), "go"), ids, n_rows, route="small", small_tag="guard_small")
    G2 = c.eng.embedding_dense_backward(c.put(_n(rng, n, d), "go2"), ids, n_rows, route="small", small_again=True, small_tag="guard_small")
    return {"G1": G1, "G2": G2}


@case(("rc_small_row_sums", "rc_small_row_sums_planned"), [(16, 1), (64, 1), (4, 3), (3, 2)])
def case_small_pair(c, d_a, d_b):
    rng = np.random.default_rng(d_a + d_b)
    n_rows, n = 120, 777
    ids = c.put(_ids(rng, 0, n_rows, n), "ids")
    Ga, Gb = c.eng.small_row_sums_pair(ids, n_rows, c.put(_n(rng, n, d_a), "src_a"), c.put(_n(rng, n, d_b), "src_b"))
    return {"Ga": Ga, "Gb": Gb}


# ---- plan-driven step --------------------------------------------------------------------------------------------------------

def _bprmf_problem(d, B, Cn, n_items, n_users=40):
    from test_gpu_bprmf import _random_problem
    return _random_problem(np.random.default_rng(d + B + Cn), n_users, n_items, d, B, Cn)


@case(("rc_bucket_plan",), [(300, 100, 20000, True), (513, 2, 700, False), (100, 9, 300, True)])
def case_bucket_plan(c, B, Cn, n_items, list_single_a):
    U, I, uid, iid = _bprmf_problem(32, B, Cn, n_items)
    out = c.eng.bucket_plan(c.put(iid, "iid"), n_items, c.put(uid, "uid"), 40, list_single_a=list_single_a)
    return {"~rows_a": out["rows_a"], "~rows_b": out["rows_b"], "~occ": out["occ"], "single": out["single"],
            "=a": _canon_records(out["rows_a"], out["occ"]), "=b": _canon_records(out["rows_b"], out["occ"])}


@case(("rc_bucket_plan", "rc_plan_update", "rc_plan_update_pair", "rc_plan_row_sums", "rc_plan_distinct"),
      [(d, opt) for d in (16, 64, 128) for opt in ("SGD", "Adam")])
def case_plan_updates(c, d, opt):
    rng = np.random.default_rng(d)
    n_rows, n_src, n_a, n_b, div = 3000, 50, 5000, 700, 4
    ids_a = np.minimum(rng.zipf(1.3, size=n_a), n_rows - 1).astype(np.int64)
    ids_b = _ids(rng, 0, 40, n_b)
    a, b = c.put(ids_a, "ids_a"), c.put(ids_b, "ids_b")
    plan = c.eng.Plan(a, n_rows, b, 40, tag="guard.plan")
    h = c.eng.make_hyper(opt, lr=0.01, l2=1e-4, step=2)
    W, m, v = _opt_tables(c, rng, n_rows, d, opt, ids_a)
    plan.update("a", W, h, m=m, v=v, coef=c.put(_n(rng, n_a), "coef"), src=c.put(_n(rng, n_src, d), "src"),
                src_index=c.put(_ids(rng, 0, n_src, (n_a + div - 1) // div), "src_index"), div=div)
    Wb, mb, vb = _opt_tables(c, rng, 40, d, opt, ids_b, "_b")
    plan.update("b", Wb, h, m=mb, v=vb, src2=c.put(_n(rng, n_b, d), "gb"), n_split=n_a)
    res = {"W": W, "m": m, "v": v, "Wb": Wb, "mb": mb, "vb": vb}
    if 2 * d <= 256:
        Wp, mp, vp = _opt_tables(c, rng, n_rows, d, opt, ids_a, "_p")
        Wq, mq, vq = _opt_tables(c, rng, n_rows, d, opt, ids_a, "_q")
        plan.update_pair("a", Wp, Wq, c.put(_n(rng, n_a, d), "gp"), c.put(_n(rng, n_a, d), "gq"), h, ma=mp, va=vp, mb=mq, vb=vq)
        res.update(Wp=Wp, mp=mp, vp=vp, Wq=Wq, mq=mq, vq=vq)
    res["sums"] = plan.row_sums("a", c.table(np.zeros((n_rows, d), f32), "sums", ids_a), src2=c.put(_n(rng, n_a + n_b, d), "g_all"))
    uniq, inverse, cnt = plan.distinct("a")
    k = int(cnt.item())
    res.update({"~uniq": uniq, "~inverse": inverse, "=count": k, "=uniq": torch.sort(uniq[:k].cpu()).values, "=ids": uniq[inverse].cpu()})
    assert torch.equal(res["=ids"], torch.from_numpy(ids_a))
    return res


@case(("rc_bprmf_fwd_bwd_update", "rc_bucket_multi_bitmap"),
      [(d, B, Cn, n_items, opt, how) for d, B, Cn, n_items in ((64, 300, 100, 20000), (64, 513, 2, 700), (32, 100, 9, 300))
       for opt, how in (("SGD", "bitmap"), ("Adam", "flags"))])
def case_bprmf_update(c, d, B, Cn, n_items, opt, how):
    U, I, uid, iid = _bprmf_problem(d, B, Cn, n_items)
    rng = np.random.default_rng(B)
    Ud, uid_d, iid_d = c.put(U, "U"), c.put(uid, "uid"), c.put(iid, "iid")
    Id, m, v = c.table(I, "I", iid), None, None
    if opt == "Adam":
        m, v = c.table(np.abs(_n(rng, n_items, d, sd=1e-3)), "m", iid), c.table(np.abs(_n(rng, n_items, d, sd=1e-3)) ** 2, "v", iid)
    h = c.eng.make_hyper(opt, lr=0.05, l2=1e-3, step=3)
    res = {}
    if how == "bitmap":
        res["~bitmap"] = multi = c.eng.bucket_multi_bitmap(iid_d, n_items)      # (words of untouched id ranges are unspecified)
        out = c.eng.bprmf_fwd_bwd_update(Ud, Id, uid_d, iid_d, None, h, mI=m, vI=v, multi=multi, want_pred=True)
    else:
        keys, perm = c.eng.sort_ids(iid_d, n_items)
        out = c.eng.bprmf_fwd_bwd_update(Ud, Id, uid_d, iid_d, c.eng.mark_singletons(keys, perm), h, mI=m, vI=v)
    res.update(out=out, I=Id, m=m, v=v)
    return res


@case(("rc_bprmf_train_step_ahead",),
      [(d, B, Cn, n_items, opt, mode) for d, B, Cn, n_items in ((64, 300, 100, 20000), (64, 513, 2, 700), (32, 100, 9, 300))
       for opt in ("SGD", "Adam") for mode in (0, 1, 2)])
def case_bprmf_trainer(c, d, B, Cn, n_items, opt, mode):
    """BprmfTrainer.step without a next batch (no look-ahead, nothing on a second stream); mode: rc_bprmf_step_pipeline -- 0 the
    small-batch step these shapes take by themselves, 1 the radix-sort pipeline, 2 the bucket plan on the caller's stream"""
    U, I, uid, iid = _bprmf_problem(d, B, Cn, n_items)
    lib = c.eng._lib.load()
    Ud, Id = c.table(U, "U", uid), c.table(I, "I", iid)
    uid_d, iid_d = c.put(uid, "uid"), c.put(iid, "iid")
    prev = lib.rc_bprmf_step_pipeline(mode)
    try:
        tr = c.eng.BprmfTrainer(Ud, Id, opt=opt, lr=0.05, l2=1e-3)
        pred = c.inout(np.zeros((B, Cn), f32), "pred")
        loss = tr.step(uid_d, iid_d, pred=pred)
        torch.cuda.synchronize()
    finally:
        lib.rc_bprmf_step_pipeline(prev)
    return {"U": Ud, "I": Id, "mU": tr.mU, "vU": tr.vU, "mI": tr.mI, "vI": tr.vI, "loss": loss, "pred": pred, "~ws": tr._ws}


# ---- dense optimizers --------------------------------------------------------------------------------------------------------

DENSE_SHAPES = [(300, 64), (300, 1), (300, 20), (777,)]


@case(("rc_dense_update", "rc_dense_update_multi", "rc_step_increment"), [("Adam",), ("Adadelta",)], allocates=False)
def case_dense_update(c, opt):
    rng = np.random.default_rng(len(opt))
    h = c.eng.make_hyper(opt, lr=0.01, l2=1e-3, step=3)
    mk = lambda s, tag, sd=1.0, sq=False: c.inout(np.abs(_n(rng, *s, sd=sd)) ** (2 if sq else 1) if sq else _n(rng, *s, sd=sd), tag)
    single, multi = [], []
    for k, s in enumerate(DENSE_SHAPES):
        for tag, items in (("s", single), ("m", multi)):
            items.append((mk(s, f"W{tag}{k}"), c.put(_n(rng, *s), f"G{tag}{k}"), h, mk(s, f"m{tag}{k}", 0.1, opt == "Adadelta"), mk(s, f"v{tag}{k}", 0.01, True)))
    for W, G_, hh, m, v in single:
        c.eng.dense_update(W, G_, hh, m, v)
    step_dev = c.inout(np.array([2], dtype=np.int64), "step_dev") if opt == "Adam" else None
    c.eng.dense_update_multi(multi, opt, step_dev=step_dev)
    return {"single": [(W, m, v) for W, _, _, m, v in single], "multi": [(W, m, v) for W, _, _, m, v in multi], "step": step_dev}


@case(("rc_dense_update_rows_dev", "rc_step_increment", "rc_step_increment2"), [0, 1, 2], allocates=False)
def case_dense_rows(c, touched):
    rng = np.random.default_rng(touched)
    rows = 300
    hit = rng.permutation(rows)[:37]
    stale = rng.permutation(rows)[:60]
    flags = np.zeros(rows, dtype=np.int32)
    flags[stale] = 6
    flags[hit] = 7
    h = c.eng.make_hyper("Adam", lr=1e-3, l2=1e-4, step=1)
    step_dev, other = c.inout(np.array([6], dtype=np.int64), "step_dev"), c.inout(np.array([41], dtype=np.int64), "other")
    c.eng.defer_increment(other)           # the next increment of another counter takes it along: rc_step_increment2
    c.eng.step_increment(step_dev)
    assert c.eng.take_deferred(other)
    c.eng.step_increment(other)            # rc_step_increment on its own
    fl = c.put(flags, "flags")
    changing = hit if touched == 1 else (np.setdiff1d(np.arange(rows), hit) if touched == 0 else np.arange(rows))
    items, keep = [], []
    for k, s in enumerate(DENSE_SHAPES[:3]):
        Gs = np.full(s, np.nan, dtype=f32)            # the gradient scratch is garbage outside the stamped rows
        Gs[hit] = _n(rng, len(hit), s[1])
        W, m, v = (c.table(x, f"{n}{k}", changing) for n, x in (("W", _n(rng, *s)), ("m", _n(rng, *s, sd=0.1)), ("v", np.abs(_n(rng, *s, sd=0.01)))))
        items.append((W, c.put(Gs, f"G{k}") if touched else None, h, m, v, fl, s[1]))
        keep.append((W, m, v))
    if touched:                                        # the plain tensor goes with the stamped rows
        s = DENSE_SHAPES[3]
        W, m, v = c.inout(_n(rng, *s), "W3"), c.inout(_n(rng, *s, sd=0.1), "m3"), c.inout(np.abs(_n(rng, *s, sd=0.01)), "v3")
        items.insert(0, (W, c.put(_n(rng, *s), "G3"), h, m, v, None, 0))
        keep.append((W, m, v))
    c.eng.dense_update_rows(items, step_dev, touched=touched, max_blocks=7 if touched == 0 else 0)
    return {"tensors": keep, "step": step_dev, "other": other}


@case(("rc_buir_ema",), [((300, 64), (777,)), ((1,), (300, 20))], allocates=False)
def case_ema(c, sa, sb):
    rng = np.random.default_rng(len(sa))
    ta, tb = c.inout(_n(rng, *sa), "target_a"), c.inout(_n(rng, *sb), "target_b")
    c.eng.ema_update(ta, c.put(_n(rng, *sa), "online_a"), tb, c.put(_n(rng, *sb), "online_b"), 0.995)
    return {"ta": ta, "tb": tb}


# ---- NeuMF -------------------------------------------------------------------------------------------------------------------

def _neumf_params(c, rng, d, l1, n_users, n_items, item_rows=None):
    P = {"mf_u": (n_users, d), "mf_i": (n_items, d), "mlp_u": (n_users, d), "mlp_i": (n_items, d), "W1": (l1, 2 * d), "b1": (l1,), "w_out": (d + l1,)}
    out = {}
    for k, s in P.items():
        x = _n(rng, *s, sd=0.3 if k[0] == "m" else 0.2)
        out[k] = c.table(x, k, item_rows) if (item_rows is not None and k in ("mf_i", "mlp_i")) else c.put(x, k)
    return out


@case(("rc_neumf_fwd", "rc_neumf_bwd"), [(32, 64, 7, 3, 0.0), (64, 32, 33, 5, 0.3)])
def case_neumf(c, d, l1, B, Cn, p):
    rng = np.random.default_rng(d + B)
    P = _neumf_params(c, rng, d, l1, 17, 40)
    uid, iid, gp = c.put(_ids(rng, 0, 17, B), "uid"), c.put(_ids(rng, 0, 40, B, Cn), "iid"), c.put(_n(rng, B, Cn), "gp")
    seed = c.seed(4242) if p > 0 else None
    pred = c.eng.neumf_fwd(P, uid, iid, p, seed)
    rows, dense = c.eng.neumf_bwd(P, uid, iid, gp, p, seed)
    return {"pred": pred, "rows": rows, "dense": dense}


@case(("rc_neumf_head_fwd_bwd",), [(64, 32, 70, 2), (32, 64, 33, 11)])
def case_neumf_head(c, d, l1, B, Cn):
    rng = np.random.default_rng(d + B + 1)
    assert c.eng.neumf_head_kernel_selected(Cn, d, l1)
    urows, irows = c.put(_n(rng, B, 2 * d, sd=0.3), "urows"), c.put(_n(rng, B * Cn, 2 * d, sd=0.3), "irows")
    W1, b1, wo = c.put(_n(rng, l1, 2 * d, sd=0.2), "W1"), c.put(_n(rng, l1, sd=0.2), "b1"), c.put(_n(rng, d + l1, sd=0.2), "w_out")
    return {"out": c.eng.neumf_head_fwd_bwd(urows, irows, W1, b1, wo, B, Cn, 1.0 / B, want_pred=True)}


@case(("rc_neumf_zhead_fwd_bwd", "rc_linear_fwd", "rc_linear_bwd"), [(7, 2, 8, 6), (7, None, 1, 1)])
def case_neumf_zhead(c, B, Cn, d, l1):
    rng = np.random.default_rng(31 + d)
    if Cn is None:        # tests/envelopes.py ZHEAD_SHAPES[1]: the longest candidate list the kernel takes
        from test_gpu_envelope_edges import scan_max
        Cn = scan_max(lambda n: c.eng._lib.load().rc_neumf_zhead_supported(n, d, l1), 2, 1 << 14)
    assert c.eng.neumf_zhead_supported(Cn, d, l1)
    urows, irows = c.put(_n(rng, B, 2 * d, sd=0.4), "urows"), c.put(_n(rng, B * Cn, d + l1, sd=0.4), "irows")
    W1, b1, wo = c.put(_n(rng, l1, 2 * d, sd=0.4), "W1"), c.put(_n(rng, l1, sd=0.4), "b1"), c.put(_n(rng, d + l1), "w_out")
    return {"out": c.eng.neumf_zhead(urows, irows, W1, b1, wo, B, Cn, 1.0 / B, want_pred=True)}


@case(("rc_neumf_train_step", "rc_neumf_mark_rows", "rc_neumf_unmark_rows"),
      [(32, 64, 1, 3, 50, "SGD", 0.0, False), (32, 32, 130, 17, 4000, "Adagrad", 0.0, True), (64, 32, 65, 100, 900, "Adam", 0.2, False)])
def case_neumf_step(c, d, l1, B, Cn, n_items, opt, p, marked):
    rng = np.random.default_rng(11 + B)
    n_users = 37
    assert c.eng.neumf_train_step_supported(Cn, d, l1)
    uid, iid = _ids(rng, 0, n_users, B), _ids(rng, 0, n_items, B, Cn)
    iid[:, 0] = iid[:, 0] % 7
    P = _neumf_params(c, rng, d, l1, n_users, n_items, item_rows=iid)
    state = {k: {} for k in P}
    for k in ("mf_i", "mlp_i"):
        if opt in ("Adam", "Adagrad"):
            state[k]["m"] = c.table(np.abs(_n(rng, n_items, d, sd=0.01)), "m_" + k, iid)
        if opt == "Adam":
            state[k]["v"] = c.table(np.abs(_n(rng, n_items, d, sd=0.01)) ** 2, "v_" + k, iid)
    u, i = c.put(uid, "uid"), c.put(iid, "iid")
    z = lambda *s: np.zeros(s, f32)
    out = {k: c.inout(x, "out_" + k) for k, x in (("loss_vec", z(B)), ("g_mf_i", z(B * Cn, d)), ("g_mlp_i", z(B * Cn, d)), ("gu_mf", z(B, d)),
                                                   ("gu_mlp", z(B, d)), ("W1", z(l1, 2 * d)), ("b1", z(l1)), ("w_out", z(d + l1)))}
    marks = c.inout(np.zeros(max(int(c.eng._lib.load().rc_neumf_train_step_marks_bytes(n_items)), 1), np.uint8), "marks")
    pred = c.inout(z(B, Cn), "pred")
    if marked:
        c.eng.neumf_mark_rows(i, n_items, marks)
    c.eng.neumf_train_step(P, state, u, i, c.eng.make_hyper(opt, lr=0.03, l2=1e-4, step=2), marks, out, pred=pred, marked=marked,
                           drop_p=p, seed=c.seed(99) if p > 0 else None)
    if marked:
        c.eng.neumf_mark_rows(i, n_items, marks, unmark=True)
    # marks = owner words [n_items] | multi flags: owner[id] is the position of whichever occurrence stored last (plain stores,
    # csrc/neumf_step.hip:654 -- "the FLAGS do not depend on the schedule", the owner words do); the flags are zero again after the step
    flags = marks[(4 * n_items + 255) // 256 * 256:]
    return {"out": out, "pred": pred, "~marks": marks, "=flags": flags.clone(), "mf_i": P["mf_i"], "mlp_i": P["mlp_i"], "state": state}


# ---- context models ----------------------------------------------------------------------------------------------------------

@case(("rc_fm_second_order_fwd", "rc_fm_second_order_bwd"), [5, 24, 64])
def case_fm(c, d):
    rng = np.random.default_rng(d)
    res = {}
    for k, (shape, F) in enumerate((((1,), 1), ((63,), 2), ((33, 5), 7))):
        V, gout, add = c.put(_n(rng, *shape, F, d, sd=0.5), f"V{k}"), c.put(_n(rng, *shape), f"gout{k}"), c.put(_n(rng, *shape, F, d), f"add{k}")
        res[k] = (c.eng.fm_second_order(V), c.eng.fm_second_order_bwd(V, gout), c.eng.fm_second_order_bwd(V, gout, add=add))
    return res


@case(("rc_gather_fields", "rc_gather_fields_fused", "rc_numeric_field_grads", "rc_small_row_sums_planned"), [(6, 7, 3), (16, 33, 5), (64, 48, 1)])
def case_gather_fields(c, d, B, Cn):
    e = c.eng
    rng = np.random.default_rng(d * 1000 + B)
    spec = [(e.FIELD_IDS, 11, True), (e.FIELD_I64, 0, True), (e.FIELD_IDS, 300, False), (e.FIELD_F64, 0, False),
            (e.FIELD_IDS, 5, True), (e.FIELD_F32, 0, True), (e.FIELD_IDS, 70, False)]
    F = len(spec)
    kinds = [k for k, _, _ in spec]
    vec = [c.put(_n(rng, v, d, sd=0.5) if k == e.FIELD_IDS else _n(rng, d, 1, sd=0.5), f"vec{f}") for f, (k, v, _) in enumerate(spec)]
    lin = [c.put(_n(rng, v, 1, sd=0.5) if k == e.FIELD_IDS else _n(rng, 1, 1, sd=0.5), f"lin{f}") for f, (k, v, _) in enumerate(spec)]
    ids = []
    for f, (k, v, per_row) in enumerate(spec):
        shape = (B,) if per_row else (B, Cn)
        x = {e.FIELD_IDS: lambda: _ids(rng, 0, max(v, 1), *shape), e.FIELD_I64: lambda: _ids(rng, 0, 7, *shape),
             e.FIELD_F64: lambda: rng.random(shape) * 6, e.FIELD_F32: lambda: (rng.random(shape) * 6).astype(f32)}[k]()
        ids.append(c.put(x, f"ids{f}"))
    num = [f for f in range(F) if kinds[f] != e.FIELD_IDS]
    n = B * Cn
    res = {"plain": tuple(e.gather_fields(vec, ids, Cn, tables1=lin, kinds=kinds))}
    gV, gL = c.put(_n(rng, n, F, d), "gV"), c.put(_n(rng, n, F), "gL")
    res["numeric"] = e.numeric_field_grads(gV, gL, [ids[f] for f in num], num, F, Cn, d)
    if d in (16, 32, 64, 128):
        fused = e.gather_fields(vec, ids, Cn, tables1=lin, kinds=kinds, numeric_key=-1, fm=True, plan=True)
        res["fused"] = tuple(fused[:6])
        res["~plan_ws"] = fused.plan_ws
        res["sums"] = e.small_row_sums_planned(fused.plan_ws, n * F, fused.offsets[-1], gV.view(n * F, d), gL.view(n * F, 1), d, (F, B, Cn),
                                               numeric=([ids[f] for f in num], num, F, Cn))
    return res


@case(("rc_bce_prob_fwd_bwd", "rc_bce_ranking_fwd_bwd", "rc_ctr_head_fwd_bwd", "rc_ctr_head_fwd_bwd_sums", "rc_ctr_head_bwd"), [(1, 1), (77, 7), (1025, 3)])
def case_ctr_heads(c, n, F):
    rng = np.random.default_rng(n)
    p = c.put((1.0 / (1.0 + np.exp(-rng.normal(0, 3, size=n)))).astype(f32), "p")
    y = c.put(rng.integers(0, 2, size=n).astype(f32), "y")
    bias, lin_, t1, t2 = c.put(_n(rng, 1), "bias"), c.put(_n(rng, n, F), "lin"), c.put(_n(rng, n), "term1"), c.put(_n(rng, n), "term2")
    label = c.put(rng.integers(0, 2, size=n).astype(np.int64), "label")
    head = c.eng.ctr_head(bias, lin_, t1, None, label)
    sums = c.eng.ctr_head_sums(bias, lin_, t1, t2, label)
    full = c.eng.ctr_head_sums(bias, lin_, None, t2, label, full=True)
    return {"bce": c.eng.bce_prob(p, y), "rank": c.eng.bce_ranking(c.put(_n(rng, n, F + 1), "pred")), "head": head, "sums": sums, "full": full,
            "bwd": c.eng.ctr_head_bwd(sums[2], sums[1], c.put(np.array([0.7], f32), "g_loss"), F)}


# ---- list-wise ---------------------------------------------------------------------------------------------------------------

def _lists(rng, B, mp, mn, no_negative_row):
    pred = _n(rng, B, mp + mn, sd=1.5)
    target = np.full((B, mp + mn), -1, dtype=np.int64)
    for b in range(B):
        n_pos, n_neg = rng.integers(1, mp + 1), (0 if (b == 0 and no_negative_row) else rng.integers(1, mn + 1))
        target[b, :n_pos] = 1
        target[b, mp:mp + n_neg] = 0
    return pred, target


@case(("rc_list_loss_fwd_bwd", "rc_softmax_ce_fwd_bwd", "rc_list_bpr_fwd_bwd"), [(4, 3, 4), (5, 100, 200)])
def case_list_losses(c, B, mp, mn):
    """row 0 has no negative for the kinds that normalise by the negatives' count and define such a row as zero (listnet, softmaxCE,
    attention_rank); the pairwise kinds average over the row's pairs, 0 / 0 = NaN in the reference as well: they get a full row"""
    from oracle.listloss_oracle import H_NORMALISED
    rng = np.random.default_rng(B + mp)
    pred, target = _lists(rng, B, mp, mn, False)
    pred0, target0 = _lists(rng, B, mp, mn, True)
    p, t, p0, t0 = c.put(pred, "pred"), c.put(target, "target"), c.put(pred0, "pred0"), c.put(target0, "target0")
    res = {name: c.eng.list_loss(*((p0, t0) if name in H_NORMALISED else (p, t)), mp, kind) for name, kind in c.eng.LIST_KINDS.items()}
    res["nograd"] = c.eng.list_loss(p0, t0, mp, c.eng.LIST_KINDS["listnet"], need_grad=False)
    res["ce"] = c.eng.softmax_ce(p0, t0, mp)
    res["bpr"], res["bprhard"] = c.eng.list_bpr(p, t, mp), c.eng.list_bpr(p, t, mp, hard=True)
    return res


@case(("rc_list_metrics",), [("n20",), ("widest", "n"), ("widest", "n/2")])
def case_list_metrics(c, which, mp_rule=None):
    rng = np.random.default_rng(len(which))
    lib = c.eng._lib.load()
    if which == "n20":
        n, mp, topk, N = 20, 10, [1, 2, 3, 5, 10, 20, 50], 7
    else:
        from test_gpu_envelope_edges import scan_max
        n = scan_max(lambda k: lib.rc_list_metrics_supported(k, k, 1), 1, 1 << 14)
        mp = n if mp_rule == "n" else n // 2
        topk, N = [1, 10, 1000, n, n + 5], 5
    assert c.eng.list_metrics_supported(n, mp, len(topk))
    pred = rng.choice(np.linspace(-2, 2, 41).astype(f32), size=(N, n))
    pos, neg = rng.integers(0, mp + 3, size=N).astype(np.int64), rng.integers(0, n - mp + 3, size=N).astype(np.int64)
    per_row, mean = c.eng.list_metrics(c.put(pred, "pred"), c.put(pos, "pos"), c.put(neg, "neg"), mp, topk)
    return {"per_row": per_row, "mean": mean}


# ---- evaluation / sampler ----------------------------------------------------------------------------------------------------

def _clicked(rng, n_users, n_items, per_user=9):
    ptr, items = [0], []
    for _ in range(n_users):
        s = np.unique(rng.integers(1, n_items, size=rng.integers(0, per_user)))
        items.extend(s.tolist())
        ptr.append(len(items))
    return np.array(ptr, dtype=np.int64), np.array(items if items else [1], dtype=np.int64)


@case(("rc_target_rank", "rc_full_catalogue_rank"), [32, 64])
def case_eval(c, d):
    rng = np.random.default_rng(d)
    n_items, N, n_users = 301, 37, 11
    ptr, items = _clicked(rng, n_users, n_items)
    I, Uv = c.put(_n(rng, n_items, d, sd=0.3), "I"), c.put(_n(rng, N, d, sd=0.3), "Uvec")
    users, targets = c.put(_ids(rng, 0, n_users, N), "users"), c.put(_ids(rng, 1, n_items, N), "targets")
    assert c.eng.full_catalogue_rank_supported(d)
    res = {"masked": c.eng.full_catalogue_rank(Uv, I, users, targets, c.put(ptr, "ptr"), c.put(items, "items")),
           "plain": c.eng.full_catalogue_rank(Uv, I, None, targets)}
    for k, (n, Cn) in enumerate(((1, 1), (7, 2), (33, 100), (5, 65))):
        res[f"rank{k}"] = c.eng.target_rank(c.put(_n(rng, n, Cn), f"pred{k}"))
    return res


@case(("rc_comirec_score_max",), [(1, 4, 1), (100, 36, 3)])
def case_score_max(c, Cn, d, K):
    rng = np.random.default_rng(Cn + d)
    n_items, B = 301, 5
    return {"pred": c.eng.comirec_score_max(c.put(_n(rng, B, K, d, sd=0.5), "interests"), c.put(_n(rng, n_items, d, sd=0.5), "item_emb"),
                                            c.put(_ids(rng, 0, n_items, B, Cn), "iid"))}


@case(("rc_sample_negatives", "rc_assemble_candidates", "rc_gather_history"), [1, 99])
def case_sampler(c, K):
    rng = np.random.default_rng(K)
    n_users, n_items, n, B = 40, 301, 97, 33
    ptr, items = _clicked(rng, n_users, n_items)
    users, its = _ids(rng, 0, n_users, n), _ids(rng, 1, n_items, n)
    u, it = c.put(users, "users"), c.put(its, "items")
    neg = c.eng.sample_negatives(u, K, n_items, c.put(ptr, "ptr"), c.put(items, "clicked"), seed=2 ** 63 + 12345, base_index=10 ** 12)
    neg_plain = c.eng.sample_negatives(u, K, n_items, seed=3)
    idx = c.put(rng.permutation(n)[:B].astype(np.int64), "idx")
    cand = c.eng.assemble_candidates(idx, u, it, neg)
    cand0 = c.eng.assemble_candidates(idx, u, it, None)
    hp = np.concatenate([[0], np.cumsum(rng.integers(1, 30, size=n_users))]).astype(np.int64)
    flat_i, flat_t = _ids(rng, 1, n_items, int(hp[-1])), np.arange(int(hp[-1]), dtype=np.int64)
    pos = np.array([rng.integers(0, hp[x + 1] - hp[x] + 1) for x in users], dtype=np.int64)
    pd, hpd, fi, ft = c.put(pos, "pos"), c.put(hp, "his_ptr"), c.put(flat_i, "his_items"), c.put(flat_t, "his_times")
    hist = {L: c.eng.gather_history(idx, u, pd, hpd, fi, L, his_times=ft) for L in (1, 5, 50)}
    return {"neg": neg, "neg_plain": neg_plain, "cand": cand, "cand0": cand0, "hist": hist, "all": c.eng.gather_history(None, u, pd, hpd, fi, 7)}


@case(("rc_stage_batch",), [(1, 1, 1), (33, 7, 3)], allocates=False)
def case_stage_batch(c, B, L, Cn):
    """the copy SasrecTrainer.step makes in front of a hipGraph replay, called as the trainer calls it (engine.py) -- without the graph"""
    import ctypes as C
    rng = np.random.default_rng(B)
    hist, lengths = _hist(rng, B, L, 60)
    h, n, i = c.put(hist, "hist"), c.put(lengths, "lengths"), c.put(_ids(rng, 1, 60, B, Cn), "iid")
    static = c.inout(np.full(h.numel() + n.numel() + i.numel(), -7, dtype=np.int64), "static")
    p = lambda t: C.c_void_p(t.data_ptr())
    c.eng._lib.call("rc_stage_batch", p(h), h.numel(), p(n), n.numel(), p(i), i.numel(), p(static), c.eng._stream())
    assert torch.equal(static, torch.cat([h.reshape(-1), n.reshape(-1), i.reshape(-1)]))
    return {"static": static}


# ---- LightGCN ----------------------------------------------------------------------------------------------------------------

@case(("rc_lgcn_propagate_fwd", "rc_lgcn_propagate_bwd"), [(d, L, chunk) for d, L in ((4, 3), (48, 0), (64, 2)) for chunk in (7, None)])
def case_lgcn(c, d, L, chunk):
    from rechorus_amd import lgcn
    rng = np.random.default_rng(5)
    n_users, n_items = 40, 30
    u = np.concatenate([rng.integers(0, 27, 90), rng.choice(np.arange(n_users), 25, replace=False)])       # users 27 .. 39: some isolated
    i = np.concatenate([rng.integers(0, 20, 90), np.full(25, 3)])                                           # item 3: degree >= 25; 20 .. 29 isolated
    key = np.unique(u * n_items + i)
    indptr, indices, data = lgcn.build_norm_adj(n_users, n_items, (key // n_items, key % n_items))
    graph = lgcn.LgcnGraph.build(n_users, n_items, indptr, indices, data, c.dev, chunk=chunk)
    N = n_users + n_items
    # the propagation buffers belong to the graph object (rechorus_amd/lgcn.py): placed by hand, at the sizes LgcnGraph.buffers gives them
    graph._buffers[d] = (c.scratch((N, d), "buf_a"), c.scratch((N, d), "buf_b"), c.scratch((max(graph.n_parts, 1), d), "partials"),
                         c.scratch((N, d), "persistent"))
    E, G_ = _n(rng, N, d, sd=0.1), _n(rng, N, d, sd=0.1)
    out = c.eng.lgcn_propagate_fwd(graph, c.put(E[:n_users], "user_emb"), c.put(E[n_users:], "item_emb"), L)
    gu, gi = c.eng.lgcn_propagate_bwd(graph, c.put(G_[:n_users], "grad_user"), c.put(G_[n_users:], "grad_item"), L)
    return {"out": out, "gu": gu, "gi": gi}


# ---- newer models ------------------------------------------------------------------------------------------------------------

@case(("rc_directau_fwd", "rc_directau_bwd"), [(2, 4), (33, 4), (129, 256), (300, 36)])
def case_directau(c, B, d):
    rng = np.random.default_rng(B + d)
    u, v = _n(rng, B, d), _n(rng, B, d)
    u[1], v[1] = u[0], v[0] * 7.0
    ue, ie = c.put(u, "user_e"), c.put(v, "item_e")
    out, pred, buf, gen = c.eng.directau_fwd(ue, ie, gamma=0.3, prediction=True)
    gu, gi = c.eng.directau_bwd(c.put(np.array([1.5], f32), "grad_out"), B, d, (1.0, 0.15, 0.15), buf)
    tab, ids = c.put(_n(rng, 50, d), "table"), c.put(_ids(rng, 0, 50, B), "row_ids")
    out2, none, buf2, _ = c.eng.directau_fwd(tab, tab, gamma=1.0, user_ids=ids, item_ids=ids)
    # the scratch keeps the forward's intermediates for the backward; its tail is the partials of the last launch: arena only
    return {"out": out, "pred": pred, "~buf": buf, "gu": gu, "gi": gi, "out_ids": out2, "~buf2": buf2}


@case(("rc_buir_fwd", "rc_buir_bwd", "rc_buir_query", "rc_buir_scores"), [(B, d) for B in (1, 63, 65) for d in (16, 48)])
def case_buir(c, B, d):
    from test_gpu_buir import _random_problem
    tabs, W, b, uid, iid = _random_problem(d, B, seed=1000 * d + B)
    t = [c.put(a, n) for a, n in zip(tabs, ("user_online", "user_target", "item_online", "item_target"))]
    Wd, bd, u, i = c.put(W, "W"), c.put(b, "b"), c.put(uid, "uid"), c.put(iid, "iid")
    loss, pred = c.eng.buir_fwd(*t, Wd, bd, u, i)
    grads = c.eng.buir_bwd(c.put(np.array([3.0], f32), "grad_out"), *t, Wd, bd, u, i)
    q, cc = c.eng.buir_query(t[0], Wd, bd, u)
    rng = np.random.default_rng(B)
    scores = {K: c.eng.buir_scores(q, cc, t[2], c.put(_ids(rng, 0, 40, B, K), f"cand{K}")) for K in (1, 99)}
    return {"loss": loss.reshape(1), "pred": pred, "grads": grads, "q": q, "c": cc, "scores": scores}


@case(("rc_comirec_fwd", "rc_comirec_bwd"), [(1, 1, 4, 1, 1, 1), (3, 2, 4, 1, 2, 1), (129, 256, 36, 5, 3, 0), (65, 20, 64, 8, 4, 1)])
def case_comirec(c, B, L, d, A, K, add_pos):
    from test_gpu_comirec import _random_problem
    P, hist, lengths, target, d_user = _random_problem(B, L, d, A, K, add_pos, seed=B + 7 * L + d)
    dev = {k: c.put(v, k) for k, v in P.items()}
    h, n, t, du = c.put(hist, "hist"), c.put(lengths, "lengths"), c.put(target, "target"), c.put(d_user, "d_user")
    interests, attn, sel, user = c.eng.comirec_fwd(dev["I"], dev["Pos"], dev["W1"], dev["b1"], dev["W2"], dev["b2"], h, n, targets=t)
    grads = c.eng.comirec_bwd(dev["I"], dev["Pos"], dev["W1"], dev["b1"], dev["W2"], h, n, attn, sel, user, du)
    ev = c.eng.comirec_fwd(dev["I"], dev["Pos"], dev["W1"], dev["b1"], dev["W2"], dev["b2"], h, n, want_attn=False)
    return {"interests": interests, "attn": attn, "sel": sel, "user": user, "grads": grads, "eval": ev}


@case(("rc_autoint_layer_fwd", "rc_autoint_layer_bwd"), [(1, 2, 4, 4, 1), (3, 3, 36, 20, 5), (257, 32, 8, 4, 4), (5, 7, 128, 64, 2)])
def case_autoint(c, N, F, Din, A, H):
    from test_gpu_autoint import layer_problem
    prob, _, _ = layer_problem(N, F, Din, A, H, seed=1000 * F + Din + A + H + N)
    t = [c.put(a, f"p{k}") for k, a in enumerate(prob)]
    Y = c.eng.autoint_layer_fwd(*t[:6], H)
    return {"Y": Y, "grads": c.eng.autoint_layer_bwd(*t[:5], Y, t[6], H)}


@case(("rc_finalmlp_gate_fwd", "rc_finalmlp_gate_bwd"),
      [(1, 1, 12, (4, 4), (4, 36), "11", 0.0), (33, 3, 36, (20, 20), (36, 64), "BB", 0.0), (129, 1, 520, (256, 4), (36, 64), "1N", 0.0),
       (31, 1, 36, (20, 4), (36, 4), "1N", 0.3)])
def case_finalmlp_gate(c, N, Cn, D, Gw, H, kinds, p):
    from test_gpu_finalmlp import _gate_case
    _, X, st, dA, _, _, _, _ = _gate_case(c.dev, N, Cn, D, Gw, H, kinds, (p, p))
    Xd = c.put(X, "X")
    streams = [tuple(c.put(a, f"s{s}.{k}") for k, a in enumerate(st[s])) + (p, c.seed(12345 + 7 * s, f"seed{s}") if p > 0 else None, 100 + s) for s in (0, 1)]
    dAd = [c.put(dA[s], f"dA{s}") for s in (0, 1)]
    A1, A2 = c.eng.finalmlp_gate_fwd(Xd, Cn, streams[0], streams[1])
    return {"A1": A1, "A2": A2, "grads": c.eng.finalmlp_gate_bwd(Xd, Cn, streams[0], streams[1], A1, dAd[0], A2, dAd[1])}


@case(("rc_finalmlp_fusion_fwd", "rc_finalmlp_fusion_bwd"), [(N, H1, H2, h) for N in (1, 33, 129) for H1, H2, h in ((4, 4, 1), (12, 36, 3))])
def case_finalmlp_fusion(c, N, H1, H2, h):
    from test_gpu_finalmlp import _fusion_case
    ar, _ = _fusion_case(c.dev, N, H1, H2, h)
    x, y, wxy, wx, bx, wy, by, dout = (c.put(a, f"a{k}") for k, a in enumerate(ar))
    return {"out": c.eng.finalmlp_fusion_fwd(x, y, wxy, wx, bx, wy, by, h), "grads": c.eng.finalmlp_fusion_bwd(x, y, wxy, wx, wy, dout, h)}


@case(("rc_contra_loss_fwd", "rc_contra_loss_bwd"), [(B, d, lab) for B in (1, 33) for d in (4, 64) for lab in (False, True)])
def case_contra(c, B, d, with_labels):
    rng = np.random.default_rng(B + d)
    va, vb = c.put(_n(rng, B, d), "va"), c.put(_n(rng, B, d), "vb")
    labels = c.put(_ids(rng, 1, 5, B), "labels") if with_labels else None
    loss, buf, gen = c.eng.contra_loss_fwd(va, vb, labels, 0.2)
    ga, gb = c.eng.contra_loss_bwd(c.put(np.array([2.0], f32), "grad_out"), labels, B, d, 0.2, buf)
    assert buf.numel() == c.eng.contra_layout(d, B)[2]        # the host-side restatement of the layout is the declared size
    return {"loss": loss, "~buf": buf, "ga": ga, "gb": gb}


# ---- sharded routing on one device -----------------------------------------------------------------------------------------

@case(("rc_route_by_owner", "rc_owner_unpack"), [(world, n) for world in (1, 3) for n in (1, 63, 4097)])
def case_route(c, world, n):
    rng = np.random.default_rng(world + n)
    ids = _ids(rng, 0, 10_000_000, n)
    ids[: n // 3] = ids[: n // 3] % 5
    d_ids = c.put(ids, "ids")
    order, counts, local = c.eng.route_by_owner(d_ids, world)
    order2, counts2, packed = c.eng.route_by_owner(d_ids, world, tuple_base=1000, div=7)
    return {"order": order, "counts": counts, "local": local, "order2": order2, "counts2": counts2, "packed": packed,
            "unpacked": c.eng.owner_unpack(packed)}


@case(("rc_owner_backward",), [("SGD", 64), ("Adam", 32)])
def case_owner_backward(c, opt, d):
    rng = np.random.default_rng(d)
    n_rows, n_tuples, n = 500, 30, 400
    t = np.sort(_ids(rng, 0, n_tuples, n))
    t[t == 17] = 18
    rows = _ids(rng, 0, n_rows, n)
    rows[::9] = rows[::9] % 11
    assert c.eng.owner_backward_supported(d)
    r = c.put(rows, "rows")
    prep = c.eng.Plan(r, n_rows, tag="guard.owner", list_single_a=False)
    I, m, v = _opt_tables(c, rng, n_rows, d, opt, rows)
    pug = c.eng.owner_backward(I, m, v, c.put(_n(rng, n_tuples, d, sd=0.1), "Uall"), c.put(t.astype(np.int32), "t32"), r, c.put(_n(rng, n), "g"),
                               prep.single, n_tuples, c.eng.make_hyper(opt, lr=0.05, l2=1e-3, step=1))
    return {"pug": pug, "I": I, "m": m, "v": v}
