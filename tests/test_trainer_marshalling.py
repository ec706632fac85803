"""CPU: what one step() of the four row-wise trainers of rechorus_amd/engine.py (FpmcTrainer, SlrcTrainer, CfkgTrainer,
ChorusTrainer) hands to the library, what the eight per-shape workspace classes ask the library and allocate, and what the sixteen
*_check_shape functions raise -- with the library calls recorded instead of made (the recorder of
tests/test_row_update_marshalling.py: _lib.call, _lib.load, engine._stream, engine._ptr and engine.workspace are recorders / stubs).

A trainer case compares the WHOLE ordered list of recorded calls with a literal: the entry point, every argument (tensors by name,
`&` for a pointer, name+bytes for an offset into a tensor, integers and floats as they are, `[...]` for a host array) and every
engine.workspace() request with its tag and byte count.  A tensor the engine allocates itself is named by its place in the step's
allocation order, dtype and shape (`#4:f32[3, 2]`), so the order of the allocations is part of the literal too.  engine._ptr keeps
its dtype and contiguity checks here and loses only the device check: the pointer arrays of rc_slrc_item_update and
rc_chorus_category_update are built from addresses, which an identity stub cannot give.

The literals were recorded from the engine as it was BEFORE the trainers shared a base class and went through segmented_update /
sort_ids for every row update (each trainer with its own optimizer check, state dictionary and _mv; FpmcTrainer and SlrcTrainer
marshalling rc_segmented_update and rc_sort_ids by hand; one class body per workspace; one three-line body per shape check) and are
unchanged since: that refactor moved code, not an argument, a byte count or an error text."""
import ctypes as C

import pytest
import torch

from rechorus_amd import _lib, engine

D, B, CN, N_USERS, N_ITEMS, R, N_CAT = 16, 3, 2, 5, 7, 2, 3
_SHORT = {torch.float32: "f32", torch.int32: "i32", torch.int64: "i64", torch.uint8: "u8"}
_ALLOCATORS = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like")


class _FakeLib:
    """every *_check_shape answers `status`, every *_bytes / *_layout query `answer` (and is listed in `queries`), every *_supported
    query 1; rc_last_error_string gives `reason`"""

    def __init__(self, answer=4096, status=_lib.RC_OK, reason=b"the library's reason"):
        self.answer, self.status, self.reason, self.queries = answer, status, reason, []

    def __getattr__(self, name):
        if name == "rc_last_error_string":
            return lambda: self.reason
        if name.endswith("_check_shape"):
            return lambda *a: self.status
        if name.endswith("_supported"):
            return lambda *a: 1

        def query(*a):
            self.queries.append((name,) + a)
            return self.answer
        return query


class _NamingTorch:
    """the name `torch` inside the engine: the real module, except that every tensor an allocation function returns is named"""

    def __init__(self, rec):
        self.__dict__["_rec"] = rec

    def __getattr__(self, name):
        fn = getattr(torch, name)
        if name not in _ALLOCATORS:
            return fn
        return lambda *a, **k: self._rec.allocated(fn(*a, **k))


class _Recorder:
    def __init__(self):
        self.calls, self.names, self.buffers, self.hypers, self.n_alloc = [], {}, {}, {}, 0

    def name(self, **tensors):
        self.names.update(tensors)
        return tensors

    def allocated(self, t):
        self.names["#%d:%s%s" % (self.n_alloc, _SHORT[t.dtype], list(t.shape))] = t
        self.n_alloc += 1
        return t

    def forget_allocations(self):
        """after a trainer's constructor: its state tensors get their own names, the step's allocations count from 0"""
        self.names = {k: t for k, t in self.names.items() if not k.startswith("#")}
        self.n_alloc = 0

    def workspace(self, nbytes, device, tag="default"):
        if tag not in self.buffers:
            self.buffers[tag] = self.names["ws:" + tag] = torch.zeros(8192, dtype=torch.uint8)
        self.calls.append(("workspace", tag, int(nbytes)))
        return self.buffers[tag]

    def _addr(self, addr):
        for k, t in self.names.items():
            lo = t.data_ptr()
            if lo <= addr < lo + max(t.numel() * t.element_size(), 1):
                return k if addr == lo else "%s+%d" % (k, addr - lo)
        return "?"

    def token(self, a):
        if isinstance(a, torch.Tensor):
            return self._addr(a.data_ptr())
        if isinstance(a, C.c_void_p):
            return None if not a.value else "&" + self._addr(a.value)
        if isinstance(a, C.Array):
            return "[%s]" % ", ".join(str(x if a._type_ is not C.c_void_p or x is None else "&" + self._addr(x)) for x in a)
        if type(a).__name__ == "CArgObject":
            return "&" + self.hypers[id(a._obj)]
        return a

    def __call__(self, name, *args):
        assert len(args) == len(_lib.SIGNATURES[name][1]), (name, len(args))
        self.calls.append((name,) + tuple(self.token(a) for a in args))

    def lines(self):
        return ["%s(%s)" % (c[0], ", ".join(str(x) for x in c[1:])) for c in self.calls]


def _ptr_without_the_device_check(t, dtype, name, allow_none=False):
    if t is None:
        if allow_none:
            return C.c_void_p(0)
        raise ValueError(f"{name} is required")
    assert t.dtype == dtype and t.is_contiguous(), name
    return C.c_void_p(t.data_ptr())


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(_lib, "call", r)
    monkeypatch.setattr(_lib, "load", lambda: _FakeLib())
    monkeypatch.setattr(engine, "_stream", lambda: "stream")
    monkeypatch.setattr(engine, "_ptr", _ptr_without_the_device_check)
    monkeypatch.setattr(engine, "workspace", r.workspace)
    monkeypatch.setattr(engine, "torch", _NamingTorch(r))
    return r


def _f(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def _i(*shape):
    return torch.zeros(shape, dtype=torch.int64)


def _trainer(rec, cls, params, **kw):
    """the trainer on the named parameter tensors; its state is named m.<table> / v.<table>, its hyper records by attribute"""
    rec.name(**params)
    tr = cls(*params.values(), **kw)
    rec.forget_allocations()
    for table, st in tr.state.items():
        rec.name(**{"%s.%s" % (k, table): t for k, t in st.items()})
    rec.hypers = {id(getattr(tr, h)): h for h in ("hyper", "hyper_kg", "hyper_bias") if hasattr(tr, h)}
    assert set(tr.state) == set(params) and all(set(st) == ({"m", "v"} if kw["opt"] == "Adam" else set()) for st in tr.state.values())
    return tr


def _step(rec, tr, **feed):
    rec.name(**feed)
    loss = tr.step(*feed.values())
    reduce = [c for c in rec.calls if c[0] == "rc_reduce_sum"][0]
    assert loss.shape == (1,) and "&" + rec.token(loss) == reduce[4]         # the device loss tensor: the first reduce's output
    assert tr.hyper.step == 1
    return rec.lines()


def _call(rec, name, k=0):
    return [c for c in rec.calls if c[0] == name][k]


# ---- FPMC -----------------------------------------------------------------------------------------------------------------------------

def _fpmc(rec, opt):
    tr = _trainer(rec, engine.FpmcTrainer, dict(UI=_f(N_USERS, D), LI=_f(N_ITEMS, D), IU=_f(N_ITEMS, D), IL=_f(N_ITEMS, D)), opt=opt)
    return _step(rec, tr, uid=_i(B), lid=_i(B), iid=_i(B, CN))


FPMC_SGD = [
    "workspace(sort, 4096)",
    "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
    "rc_segment_heads(&#0:i32[6], &#1:i32[6], 6, 0, None, &#2:i32[6], &#3:i32[1], stream)",
    "workspace(sort, 4096)",
    "rc_sort_ids(&uid, 3, &lid, 3, 5, 12, &#4:i32[6], &#5:i32[6], &ws:sort, 8192, stream)",
    "rc_fpmc_fwd_bwd(&UI, &LI, &IU, &IL, &uid, &lid, &iid, 3, 2, 16, 0.3333333333333333, None, &#6:f32[3], &#7:f32[3, 2], &#8:f32[3, 16], &#9:f32[3, 16], stream)",
    "rc_reduce_sum(&#6:f32[3], 3, 0.3333333333333333, &#10:f32[1], stream)",
    "workspace(fpmc_item, 4096)",
    "rc_fpmc_item_update(&IU, None, None, &IL, None, None, 16, &#0:i32[6], &#1:i32[6], 6, &#7:f32[3, 2], &UI, &LI, &uid, &lid, 2, &hyper, None, None, &#2:i32[6], &#3:i32[1], &ws:fpmc_item, 8192, stream)",
    "workspace(seg, 4096)",
    "rc_segmented_update(&UI, None, None, 16, &#4:i32[6], &#5:i32[6], 3, None, &#8:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
    "workspace(seg, 4096)",
    "rc_segmented_update(&LI, None, None, 16, &#4:i32[6]+12, &#5:i32[6]+12, 3, None, &#9:f32[3, 16], None, 1, None, 3, 5, 3, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
]

FPMC_ADAM = [
    "workspace(sort, 4096)",
    "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
    "rc_segment_heads(&#0:i32[6], &#1:i32[6], 6, 0, None, &#2:i32[6], &#3:i32[1], stream)",
    "workspace(sort, 4096)",
    "rc_sort_ids(&uid, 3, &lid, 3, 5, 12, &#4:i32[6], &#5:i32[6], &ws:sort, 8192, stream)",
    "rc_fpmc_fwd_bwd(&UI, &LI, &IU, &IL, &uid, &lid, &iid, 3, 2, 16, 0.3333333333333333, None, &#6:f32[3], &#7:f32[3, 2], &#8:f32[3, 16], &#9:f32[3, 16], stream)",
    "rc_reduce_sum(&#6:f32[3], 3, 0.3333333333333333, &#10:f32[1], stream)",
    "workspace(fpmc_item, 4096)",
    "rc_fpmc_item_update(&IU, &m.IU, &v.IU, &IL, &m.IL, &v.IL, 16, &#0:i32[6], &#1:i32[6], 6, &#7:f32[3, 2], &UI, &LI, &uid, &lid, 2, &hyper, None, None, &#2:i32[6], &#3:i32[1], &ws:fpmc_item, 8192, stream)",
    "workspace(seg, 4096)",
    "rc_segmented_update(&UI, &m.UI, &v.UI, 16, &#4:i32[6], &#5:i32[6], 3, None, &#8:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
    "workspace(seg, 4096)",
    "rc_segmented_update(&LI, &m.LI, &v.LI, 16, &#4:i32[6]+12, &#5:i32[6]+12, 3, None, &#9:f32[3, 16], None, 1, None, 3, 5, 3, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
]


@pytest.mark.parametrize("opt,want", [("SGD", FPMC_SGD), ("Adam", FPMC_ADAM)])
def test_fpmc_step(rec, opt, want):
    assert _fpmc(rec, opt) == want
    # users and last items are sorted jointly, the last items keyed behind the users ...
    assert _call(rec, "rc_sort_ids", 1)[1:7] == ("&uid", B, "&lid", B, N_USERS, N_USERS + N_ITEMS)
    # ... and LI's update takes the second half of that sort: key_base = n_users, occ_base = B (UI's: 0, 0)
    ui, li = _call(rec, "rc_segmented_update", 0), _call(rec, "rc_segmented_update", 1)
    assert (ui[1], ui[14], ui[15]) == ("&UI", 0, 0) and (li[1], li[14], li[15]) == ("&LI", N_USERS, B)


# ---- SLRC+ ----------------------------------------------------------------------------------------------------------------------------

def _slrc(rec, opt):
    params = dict(U=_f(N_USERS, D), I=_f(N_ITEMS, D), user_bias=_f(N_USERS, 1), item_bias=_f(N_ITEMS, 1), global_alpha=_f(1),
                  alphas=_f(N_ITEMS, R), pis=_f(N_ITEMS, R), betas=_f(N_ITEMS, R), sigmas=_f(N_ITEMS, R), mus=_f(N_ITEMS, R))
    assert tuple(params) == engine.SLRC_PARAMS
    tr = _trainer(rec, engine.SlrcTrainer, params, opt=opt)
    return _step(rec, tr, uid=_i(B), iid=_i(B, CN), intervals=_f(B, CN, R))


SLRC_SGD = [
    "workspace(sort, 4096)",
    "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
    "rc_segment_heads(&#0:i32[6], &#1:i32[6], 6, 0, None, &#2:i32[6], &#3:i32[1], stream)",
    "workspace(sort, 4096)",
    "rc_sort_ids(&uid, 3, None, 0, 0, 5, &#4:i32[3], &#5:i32[3], &ws:sort, 8192, stream)",
    "rc_slrc_fwd_bwd(&U, &I, &user_bias, &item_bias, &global_alpha, &alphas, &pis, &betas, &sigmas, &mus, &uid, &iid, &intervals, 3, 2, 16, 2, 0.3333333333333333, None, &#6:f32[3], &#7:f32[3, 2], &#8:f32[3, 16], &#9:f32[3], &#10:f32[6, 10], &#11:f32[3], stream)",
    "rc_reduce_sum(&#6:f32[3], 3, 0.3333333333333333, &#12:f32[1], stream)",
    "workspace(slrc_item, 4096)",
    "rc_slrc_item_update([&I, &item_bias, &alphas, &pis, &betas, &sigmas, &mus], None, None, 16, 2, &#0:i32[6], &#1:i32[6], 6, &#7:f32[3, 2], &#10:f32[6, 10], &U, &uid, 2, &hyper, None, &#2:i32[6], &#3:i32[1], &ws:slrc_item, 8192, stream)",
    "workspace(seg, 4096)",
    "rc_segmented_update(&U, None, None, 16, &#4:i32[3], &#5:i32[3], 3, None, &#8:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
    "rc_slrc_user_bias_update(&user_bias, None, None, &#4:i32[3], &#5:i32[3], 3, &#9:f32[3], &hyper, None, stream)",
    "rc_reduce_sum(&#11:f32[3], 3, 1.0, &#13:f32[1], stream)",
    "rc_dense_update(&global_alpha, &#13:f32[1], None, None, 1, &hyper, stream)",
]

SLRC_ADAM = [
    "workspace(sort, 4096)",
    "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
    "rc_segment_heads(&#0:i32[6], &#1:i32[6], 6, 0, None, &#2:i32[6], &#3:i32[1], stream)",
    "workspace(sort, 4096)",
    "rc_sort_ids(&uid, 3, None, 0, 0, 5, &#4:i32[3], &#5:i32[3], &ws:sort, 8192, stream)",
    "rc_slrc_fwd_bwd(&U, &I, &user_bias, &item_bias, &global_alpha, &alphas, &pis, &betas, &sigmas, &mus, &uid, &iid, &intervals, 3, 2, 16, 2, 0.3333333333333333, None, &#6:f32[3], &#7:f32[3, 2], &#8:f32[3, 16], &#9:f32[3], &#10:f32[6, 10], &#11:f32[3], stream)",
    "rc_reduce_sum(&#6:f32[3], 3, 0.3333333333333333, &#12:f32[1], stream)",
    "workspace(slrc_item, 4096)",
    "rc_slrc_item_update([&I, &item_bias, &alphas, &pis, &betas, &sigmas, &mus], [&m.I, &m.item_bias, &m.alphas, &m.pis, &m.betas, &m.sigmas, &m.mus], [&v.I, &v.item_bias, &v.alphas, &v.pis, &v.betas, &v.sigmas, &v.mus], 16, 2, &#0:i32[6], &#1:i32[6], 6, &#7:f32[3, 2], &#10:f32[6, 10], &U, &uid, 2, &hyper, None, &#2:i32[6], &#3:i32[1], &ws:slrc_item, 8192, stream)",
    "workspace(seg, 4096)",
    "rc_segmented_update(&U, &m.U, &v.U, 16, &#4:i32[3], &#5:i32[3], 3, None, &#8:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
    "rc_slrc_user_bias_update(&user_bias, &m.user_bias, &v.user_bias, &#4:i32[3], &#5:i32[3], 3, &#9:f32[3], &hyper, None, stream)",
    "rc_reduce_sum(&#11:f32[3], 3, 1.0, &#13:f32[1], stream)",
    "rc_dense_update(&global_alpha, &#13:f32[1], &m.global_alpha, &v.global_alpha, 1, &hyper, stream)",
]


@pytest.mark.parametrize("opt,want", [("SGD", SLRC_SGD), ("Adam", SLRC_ADAM)])
def test_slrc_step(rec, opt, want):
    assert _slrc(rec, opt) == want


# ---- CFKG -----------------------------------------------------------------------------------------------------------------------------

def _cfkg(rec, opt):
    tr = _trainer(rec, engine.CfkgTrainer, dict(E=_f(N_USERS + N_ITEMS, D), R=_f(R, D)), margin=0.5, opt=opt)
    return _step(rec, tr, head=_i(2, 4), tail=_i(2, 4), rel=_i(2, 4))


# (allocation #0 is the [B, 4] id block (h, t, h', t'), #1 its transpose: the four id columns of the front kernel are its rows)
CFKG_SGD = [
    "workspace(cfkg_front, 4096)",
    "rc_cfkg_fwd_bwd(&E, &R, &#1:i64[4, 2], &#1:i64[4, 2]+16, &#1:i64[4, 2]+32, &#1:i64[4, 2]+48, &#2:i64[2], 2, 16, 12, 2, 0.5, 0.5, &#3:f32[2], None, &#4:f32[2, 4, 16], &#5:f32[2, 16], &ws:cfkg_front, 8192, stream)",
    "rc_reduce_sum(&#3:f32[2], 2, 0.5, &#6:f32[1], stream)",
    "workspace(sort, 4096)",
    "rc_sort_ids(&#0:i64[2, 4], 8, None, 0, 0, 12, &#7:i32[8], &#8:i32[8], &ws:sort, 8192, stream)",
    "workspace(seg, 4096)",
    "rc_segmented_update(&E, None, None, 16, &#7:i32[8], &#8:i32[8], 8, None, &#4:f32[2, 4, 16], None, 1, None, 8, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
    "rc_dense_update(&R, &#5:f32[2, 16], None, None, 32, &hyper, stream)",
]

CFKG_ADAM = [
    "workspace(cfkg_front, 4096)",
    "rc_cfkg_fwd_bwd(&E, &R, &#1:i64[4, 2], &#1:i64[4, 2]+16, &#1:i64[4, 2]+32, &#1:i64[4, 2]+48, &#2:i64[2], 2, 16, 12, 2, 0.5, 0.5, &#3:f32[2], None, &#4:f32[2, 4, 16], &#5:f32[2, 16], &ws:cfkg_front, 8192, stream)",
    "rc_reduce_sum(&#3:f32[2], 2, 0.5, &#6:f32[1], stream)",
    "workspace(sort, 4096)",
    "rc_sort_ids(&#0:i64[2, 4], 8, None, 0, 0, 12, &#7:i32[8], &#8:i32[8], &ws:sort, 8192, stream)",
    "workspace(seg, 4096)",
    "rc_segmented_update(&E, &m.E, &v.E, 16, &#7:i32[8], &#8:i32[8], 8, None, &#4:f32[2, 4, 16], None, 1, None, 8, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
    "rc_dense_update(&R, &#5:f32[2, 16], &m.R, &v.R, 32, &hyper, stream)",
]


@pytest.mark.parametrize("opt,want", [("SGD", CFKG_SGD), ("Adam", CFKG_ADAM)])
def test_cfkg_step(rec, opt, want):
    assert _cfkg(rec, opt) == want


# ---- Chorus ---------------------------------------------------------------------------------------------------------------------------

def _chorus(rec, opt, gmf, kinds):
    params = dict(U=_f(N_USERS, D), I=_f(N_ITEMS, D), Rel=_f(R, D), betas=_f(N_CAT, R), mus=_f(N_CAT, R), sigmas=_f(N_CAT, R),
                  w=_f(1, D), user_bias=_f(N_USERS, 1), item_bias=_f(N_ITEMS, 1))
    assert tuple(params) == engine.CHORUS_PARAMS
    tr = _trainer(rec, engine.ChorusTrainer, params, kinds=kinds, gmf=gmf, opt=opt)
    lines = _step(rec, tr, uid=_i(B), iid=_i(B, CN), cid=_i(B, CN), intervals=_f(B, CN, R))
    assert tr.hyper_kg.step == 1 and tr.hyper_bias.step == 1                 # the three hyper records step together
    return lines


# (opt, gmf, kinds) -> the step's calls
CHORUS = {
    ("SGD", False, (0, 2)): [
        "workspace(sort, 4096)",
        "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&cid, 6, None, 0, 0, 3, &#2:i32[6], &#3:i32[6], &ws:sort, 8192, stream)",
        "rc_segment_heads(&#2:i32[6], &#3:i32[6], 6, 0, None, &#4:i32[6], &#5:i32[1], stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&uid, 3, None, 0, 0, 5, &#6:i32[3], &#7:i32[3], &ws:sort, 8192, stream)",
        "workspace(chorus_front, 4096)",
        "rc_chorus_fwd_bwd(&U, &I, &Rel, &betas, &sigmas, &mus, None, &user_bias, &item_bias, &uid, &iid, &cid, &intervals, [0, 2], 3, 2, 16, 2, 0.3333333333333333, None, &#13:f32[3], &#14:f32[3, 2], &#8:f32[3, 2], &#9:f32[3, 16], &#10:f32[3], &#11:f32[6, 6], &#12:f32[2, 16], None, None, &ws:chorus_front, 8192, stream)",
        "rc_reduce_sum(&#13:f32[3], 3, 0.3333333333333333, &#15:f32[1], stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&I, None, None, 16, &#0:i32[6], &#1:i32[6], 6, &#8:f32[3, 2], &U, &uid, 2, None, 6, 0, 0, &hyper_kg, None, None, None, 0, &ws:seg, 8192, stream)",
        "rc_slrc_user_bias_update(&item_bias, None, None, &#0:i32[6], &#1:i32[6], 6, &#14:f32[3, 2], &hyper_bias, None, stream)",
        "workspace(chorus_cat, 4096)",
        "rc_chorus_category_update([&betas, &sigmas, &mus], None, None, 3, 2, &#2:i32[6], &#3:i32[6], 6, &#11:f32[6, 6], &hyper, None, &#4:i32[6], &#5:i32[1], &ws:chorus_cat, 8192, stream)",
        "rc_dense_update(&Rel, &#12:f32[2, 16], None, None, 32, &hyper_kg, stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&U, None, None, 16, &#6:i32[3], &#7:i32[3], 3, None, &#9:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
        "rc_slrc_user_bias_update(&user_bias, None, None, &#6:i32[3], &#7:i32[3], 3, &#10:f32[3], &hyper_bias, None, stream)",
    ],
    ("SGD", False, (0, 1)): [
        "workspace(sort, 4096)",
        "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&cid, 6, None, 0, 0, 3, &#2:i32[6], &#3:i32[6], &ws:sort, 8192, stream)",
        "rc_segment_heads(&#2:i32[6], &#3:i32[6], 6, 0, None, &#4:i32[6], &#5:i32[1], stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&uid, 3, None, 0, 0, 5, &#6:i32[3], &#7:i32[3], &ws:sort, 8192, stream)",
        "workspace(chorus_front, 4096)",
        "rc_chorus_fwd_bwd(&U, &I, &Rel, &betas, &sigmas, &mus, None, &user_bias, &item_bias, &uid, &iid, &cid, &intervals, [0, 1], 3, 2, 16, 2, 0.3333333333333333, None, &#13:f32[3], &#14:f32[3, 2], &#8:f32[3, 2], &#9:f32[3, 16], &#10:f32[3], &#11:f32[6, 6], &#12:f32[2, 16], None, None, &ws:chorus_front, 8192, stream)",
        "rc_reduce_sum(&#13:f32[3], 3, 0.3333333333333333, &#15:f32[1], stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&I, None, None, 16, &#0:i32[6], &#1:i32[6], 6, &#8:f32[3, 2], &U, &uid, 2, None, 6, 0, 0, &hyper_kg, None, None, None, 0, &ws:seg, 8192, stream)",
        "rc_slrc_user_bias_update(&item_bias, None, None, &#0:i32[6], &#1:i32[6], 6, &#14:f32[3, 2], &hyper_bias, None, stream)",
        "workspace(chorus_cat, 4096)",
        "rc_chorus_category_update([&betas, None, None], None, None, 3, 2, &#2:i32[6], &#3:i32[6], 6, &#11:f32[6, 6], &hyper, None, &#4:i32[6], &#5:i32[1], &ws:chorus_cat, 8192, stream)",
        "rc_dense_update(&Rel, &#12:f32[2, 16], None, None, 32, &hyper_kg, stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&U, None, None, 16, &#6:i32[3], &#7:i32[3], 3, None, &#9:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
        "rc_slrc_user_bias_update(&user_bias, None, None, &#6:i32[3], &#7:i32[3], 3, &#10:f32[3], &hyper_bias, None, stream)",
    ],
    ("SGD", True, (0, 2)): [
        "workspace(sort, 4096)",
        "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&cid, 6, None, 0, 0, 3, &#2:i32[6], &#3:i32[6], &ws:sort, 8192, stream)",
        "rc_segment_heads(&#2:i32[6], &#3:i32[6], 6, 0, None, &#4:i32[6], &#5:i32[1], stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&uid, 3, None, 0, 0, 5, &#6:i32[3], &#7:i32[3], &ws:sort, 8192, stream)",
        "workspace(chorus_front, 4096)",
        "rc_chorus_fwd_bwd(&U, &I, &Rel, &betas, &sigmas, &mus, &w, None, None, &uid, &iid, &cid, &intervals, [0, 2], 3, 2, 16, 2, 0.3333333333333333, None, &#15:f32[3], &#16:f32[3, 2], &#8:f32[3, 2], &#9:f32[3, 16], &#10:f32[3], &#11:f32[6, 6], &#12:f32[2, 16], &#13:f32[16], &#14:f32[3, 16], &ws:chorus_front, 8192, stream)",
        "rc_reduce_sum(&#15:f32[3], 3, 0.3333333333333333, &#17:f32[1], stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&I, None, None, 16, &#0:i32[6], &#1:i32[6], 6, &#8:f32[3, 2], &#14:f32[3, 16], None, 2, None, 6, 0, 0, &hyper_kg, None, None, None, 0, &ws:seg, 8192, stream)",
        "workspace(chorus_cat, 4096)",
        "rc_chorus_category_update([&betas, &sigmas, &mus], None, None, 3, 2, &#2:i32[6], &#3:i32[6], 6, &#11:f32[6, 6], &hyper, None, &#4:i32[6], &#5:i32[1], &ws:chorus_cat, 8192, stream)",
        "rc_dense_update(&Rel, &#12:f32[2, 16], None, None, 32, &hyper_kg, stream)",
        "rc_dense_update(&w, &#13:f32[16], None, None, 16, &hyper, stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&U, None, None, 16, &#6:i32[3], &#7:i32[3], 3, None, &#9:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
    ],
    ("SGD", True, (0, 1)): [
        "workspace(sort, 4096)",
        "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&cid, 6, None, 0, 0, 3, &#2:i32[6], &#3:i32[6], &ws:sort, 8192, stream)",
        "rc_segment_heads(&#2:i32[6], &#3:i32[6], 6, 0, None, &#4:i32[6], &#5:i32[1], stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&uid, 3, None, 0, 0, 5, &#6:i32[3], &#7:i32[3], &ws:sort, 8192, stream)",
        "workspace(chorus_front, 4096)",
        "rc_chorus_fwd_bwd(&U, &I, &Rel, &betas, &sigmas, &mus, &w, None, None, &uid, &iid, &cid, &intervals, [0, 1], 3, 2, 16, 2, 0.3333333333333333, None, &#15:f32[3], &#16:f32[3, 2], &#8:f32[3, 2], &#9:f32[3, 16], &#10:f32[3], &#11:f32[6, 6], &#12:f32[2, 16], &#13:f32[16], &#14:f32[3, 16], &ws:chorus_front, 8192, stream)",
        "rc_reduce_sum(&#15:f32[3], 3, 0.3333333333333333, &#17:f32[1], stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&I, None, None, 16, &#0:i32[6], &#1:i32[6], 6, &#8:f32[3, 2], &#14:f32[3, 16], None, 2, None, 6, 0, 0, &hyper_kg, None, None, None, 0, &ws:seg, 8192, stream)",
        "workspace(chorus_cat, 4096)",
        "rc_chorus_category_update([&betas, None, None], None, None, 3, 2, &#2:i32[6], &#3:i32[6], 6, &#11:f32[6, 6], &hyper, None, &#4:i32[6], &#5:i32[1], &ws:chorus_cat, 8192, stream)",
        "rc_dense_update(&Rel, &#12:f32[2, 16], None, None, 32, &hyper_kg, stream)",
        "rc_dense_update(&w, &#13:f32[16], None, None, 16, &hyper, stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&U, None, None, 16, &#6:i32[3], &#7:i32[3], 3, None, &#9:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
    ],
    ("Adam", False, (0, 2)): [
        "workspace(sort, 4096)",
        "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&cid, 6, None, 0, 0, 3, &#2:i32[6], &#3:i32[6], &ws:sort, 8192, stream)",
        "rc_segment_heads(&#2:i32[6], &#3:i32[6], 6, 0, None, &#4:i32[6], &#5:i32[1], stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&uid, 3, None, 0, 0, 5, &#6:i32[3], &#7:i32[3], &ws:sort, 8192, stream)",
        "workspace(chorus_front, 4096)",
        "rc_chorus_fwd_bwd(&U, &I, &Rel, &betas, &sigmas, &mus, None, &user_bias, &item_bias, &uid, &iid, &cid, &intervals, [0, 2], 3, 2, 16, 2, 0.3333333333333333, None, &#13:f32[3], &#14:f32[3, 2], &#8:f32[3, 2], &#9:f32[3, 16], &#10:f32[3], &#11:f32[6, 6], &#12:f32[2, 16], None, None, &ws:chorus_front, 8192, stream)",
        "rc_reduce_sum(&#13:f32[3], 3, 0.3333333333333333, &#15:f32[1], stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&I, &m.I, &v.I, 16, &#0:i32[6], &#1:i32[6], 6, &#8:f32[3, 2], &U, &uid, 2, None, 6, 0, 0, &hyper_kg, None, None, None, 0, &ws:seg, 8192, stream)",
        "rc_slrc_user_bias_update(&item_bias, &m.item_bias, &v.item_bias, &#0:i32[6], &#1:i32[6], 6, &#14:f32[3, 2], &hyper_bias, None, stream)",
        "workspace(chorus_cat, 4096)",
        "rc_chorus_category_update([&betas, &sigmas, &mus], [&m.betas, &m.sigmas, &m.mus], [&v.betas, &v.sigmas, &v.mus], 3, 2, &#2:i32[6], &#3:i32[6], 6, &#11:f32[6, 6], &hyper, None, &#4:i32[6], &#5:i32[1], &ws:chorus_cat, 8192, stream)",
        "rc_dense_update(&Rel, &#12:f32[2, 16], &m.Rel, &v.Rel, 32, &hyper_kg, stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&U, &m.U, &v.U, 16, &#6:i32[3], &#7:i32[3], 3, None, &#9:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
        "rc_slrc_user_bias_update(&user_bias, &m.user_bias, &v.user_bias, &#6:i32[3], &#7:i32[3], 3, &#10:f32[3], &hyper_bias, None, stream)",
    ],
    ("Adam", False, (0, 1)): [
        "workspace(sort, 4096)",
        "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&cid, 6, None, 0, 0, 3, &#2:i32[6], &#3:i32[6], &ws:sort, 8192, stream)",
        "rc_segment_heads(&#2:i32[6], &#3:i32[6], 6, 0, None, &#4:i32[6], &#5:i32[1], stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&uid, 3, None, 0, 0, 5, &#6:i32[3], &#7:i32[3], &ws:sort, 8192, stream)",
        "workspace(chorus_front, 4096)",
        "rc_chorus_fwd_bwd(&U, &I, &Rel, &betas, &sigmas, &mus, None, &user_bias, &item_bias, &uid, &iid, &cid, &intervals, [0, 1], 3, 2, 16, 2, 0.3333333333333333, None, &#13:f32[3], &#14:f32[3, 2], &#8:f32[3, 2], &#9:f32[3, 16], &#10:f32[3], &#11:f32[6, 6], &#12:f32[2, 16], None, None, &ws:chorus_front, 8192, stream)",
        "rc_reduce_sum(&#13:f32[3], 3, 0.3333333333333333, &#15:f32[1], stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&I, &m.I, &v.I, 16, &#0:i32[6], &#1:i32[6], 6, &#8:f32[3, 2], &U, &uid, 2, None, 6, 0, 0, &hyper_kg, None, None, None, 0, &ws:seg, 8192, stream)",
        "rc_slrc_user_bias_update(&item_bias, &m.item_bias, &v.item_bias, &#0:i32[6], &#1:i32[6], 6, &#14:f32[3, 2], &hyper_bias, None, stream)",
        "workspace(chorus_cat, 4096)",
        "rc_chorus_category_update([&betas, None, None], [&m.betas, &m.sigmas, &m.mus], [&v.betas, &v.sigmas, &v.mus], 3, 2, &#2:i32[6], &#3:i32[6], 6, &#11:f32[6, 6], &hyper, None, &#4:i32[6], &#5:i32[1], &ws:chorus_cat, 8192, stream)",
        "rc_dense_update(&Rel, &#12:f32[2, 16], &m.Rel, &v.Rel, 32, &hyper_kg, stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&U, &m.U, &v.U, 16, &#6:i32[3], &#7:i32[3], 3, None, &#9:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
        "rc_slrc_user_bias_update(&user_bias, &m.user_bias, &v.user_bias, &#6:i32[3], &#7:i32[3], 3, &#10:f32[3], &hyper_bias, None, stream)",
    ],
    ("Adam", True, (0, 2)): [
        "workspace(sort, 4096)",
        "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&cid, 6, None, 0, 0, 3, &#2:i32[6], &#3:i32[6], &ws:sort, 8192, stream)",
        "rc_segment_heads(&#2:i32[6], &#3:i32[6], 6, 0, None, &#4:i32[6], &#5:i32[1], stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&uid, 3, None, 0, 0, 5, &#6:i32[3], &#7:i32[3], &ws:sort, 8192, stream)",
        "workspace(chorus_front, 4096)",
        "rc_chorus_fwd_bwd(&U, &I, &Rel, &betas, &sigmas, &mus, &w, None, None, &uid, &iid, &cid, &intervals, [0, 2], 3, 2, 16, 2, 0.3333333333333333, None, &#15:f32[3], &#16:f32[3, 2], &#8:f32[3, 2], &#9:f32[3, 16], &#10:f32[3], &#11:f32[6, 6], &#12:f32[2, 16], &#13:f32[16], &#14:f32[3, 16], &ws:chorus_front, 8192, stream)",
        "rc_reduce_sum(&#15:f32[3], 3, 0.3333333333333333, &#17:f32[1], stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&I, &m.I, &v.I, 16, &#0:i32[6], &#1:i32[6], 6, &#8:f32[3, 2], &#14:f32[3, 16], None, 2, None, 6, 0, 0, &hyper_kg, None, None, None, 0, &ws:seg, 8192, stream)",
        "workspace(chorus_cat, 4096)",
        "rc_chorus_category_update([&betas, &sigmas, &mus], [&m.betas, &m.sigmas, &m.mus], [&v.betas, &v.sigmas, &v.mus], 3, 2, &#2:i32[6], &#3:i32[6], 6, &#11:f32[6, 6], &hyper, None, &#4:i32[6], &#5:i32[1], &ws:chorus_cat, 8192, stream)",
        "rc_dense_update(&Rel, &#12:f32[2, 16], &m.Rel, &v.Rel, 32, &hyper_kg, stream)",
        "rc_dense_update(&w, &#13:f32[16], &m.w, &v.w, 16, &hyper, stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&U, &m.U, &v.U, 16, &#6:i32[3], &#7:i32[3], 3, None, &#9:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
    ],
    ("Adam", True, (0, 1)): [
        "workspace(sort, 4096)",
        "rc_sort_ids(&iid, 6, None, 0, 0, 7, &#0:i32[6], &#1:i32[6], &ws:sort, 8192, stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&cid, 6, None, 0, 0, 3, &#2:i32[6], &#3:i32[6], &ws:sort, 8192, stream)",
        "rc_segment_heads(&#2:i32[6], &#3:i32[6], 6, 0, None, &#4:i32[6], &#5:i32[1], stream)",
        "workspace(sort, 4096)",
        "rc_sort_ids(&uid, 3, None, 0, 0, 5, &#6:i32[3], &#7:i32[3], &ws:sort, 8192, stream)",
        "workspace(chorus_front, 4096)",
        "rc_chorus_fwd_bwd(&U, &I, &Rel, &betas, &sigmas, &mus, &w, None, None, &uid, &iid, &cid, &intervals, [0, 1], 3, 2, 16, 2, 0.3333333333333333, None, &#15:f32[3], &#16:f32[3, 2], &#8:f32[3, 2], &#9:f32[3, 16], &#10:f32[3], &#11:f32[6, 6], &#12:f32[2, 16], &#13:f32[16], &#14:f32[3, 16], &ws:chorus_front, 8192, stream)",
        "rc_reduce_sum(&#15:f32[3], 3, 0.3333333333333333, &#17:f32[1], stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&I, &m.I, &v.I, 16, &#0:i32[6], &#1:i32[6], 6, &#8:f32[3, 2], &#14:f32[3, 16], None, 2, None, 6, 0, 0, &hyper_kg, None, None, None, 0, &ws:seg, 8192, stream)",
        "workspace(chorus_cat, 4096)",
        "rc_chorus_category_update([&betas, None, None], [&m.betas, &m.sigmas, &m.mus], [&v.betas, &v.sigmas, &v.mus], 3, 2, &#2:i32[6], &#3:i32[6], 6, &#11:f32[6, 6], &hyper, None, &#4:i32[6], &#5:i32[1], &ws:chorus_cat, 8192, stream)",
        "rc_dense_update(&Rel, &#12:f32[2, 16], &m.Rel, &v.Rel, 32, &hyper_kg, stream)",
        "rc_dense_update(&w, &#13:f32[16], &m.w, &v.w, 16, &hyper, stream)",
        "workspace(seg, 4096)",
        "rc_segmented_update(&U, &m.U, &v.U, 16, &#6:i32[3], &#7:i32[3], 3, None, &#9:f32[3, 16], None, 1, None, 3, 0, 0, &hyper, None, None, None, 0, &ws:seg, 8192, stream)",
    ],
}


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
@pytest.mark.parametrize("gmf", [False, True], ids=["bpr", "gmf"])
@pytest.mark.parametrize("kinds", [[0, 2], [0, 1]], ids=["substitute", "complement"])
def test_chorus_step(rec, opt, gmf, kinds):
    assert _chorus(rec, opt, gmf, kinds) == CHORUS[opt, gmf, tuple(kinds)]
    # without a 'substitute' relation sigmas and mus have no gradient: their W slots are null, their state still travels
    W = _call(rec, "rc_chorus_category_update")[1]
    assert W == ("[&betas, &sigmas, &mus]" if 2 in kinds else "[&betas, None, None]")


# ---- the per-shape workspaces ---------------------------------------------------------------------------------------------------------

# class, get()'s shape arguments, the same with one changed, the size query, the query's arguments for the first, rounds up to 256
WORKSPACES = [
    (engine.DirectAUWorkspace, (3, 16), (4, 16), "rc_directau_workspace_bytes", (16, 3), False),
    (engine.ContraWorkspace, (3, 16), (3, 32), "rc_contra_workspace_bytes", (16, 3), False),
    (engine.BuirWorkspace, (3, 16), (4, 16), "rc_buir_workspace_bytes", (16, 3), False),
    (engine.ComiRecWorkspace, (16, 8, 4, 5, 3), (16, 8, 4, 5, 6), "rc_comirec_workspace_bytes", (16, 8, 4, 5, 3), True),
    (engine.AutoIntWorkspace, (3, 6, 16, 8, 2), (3, 6, 16, 8, 4), "rc_autoint_workspace_bytes", (3, 6, 16, 8, 2), True),
    (engine.DCNv2Workspace, (3, 32, 8, 2), (5, 32, 8, 2), "rc_dcnv2_mix_layer_bwd_workspace_bytes", (3, 32, 8, 2), True),
    (engine.ListEncWorkspace, (3, 5, 16, 2, 32), (3, 6, 16, 2, 32), "rc_listenc_block_bwd_workspace_bytes", (3, 5, 16, 2, 32), True),
    (engine.FinalMLPWorkspace, ("gate", (6, 2, 24, 8, 12, 3, 4, 16, 6)), ("gate", (6, 2, 24, 8, 12, 3, 4, 16, 1)),
     "rc_finalmlp_gate_workspace_bytes", (6, 2, 24, 8, 12, 3, 4, 16, 6), True),
    (engine.FinalMLPWorkspace, ("fusion", (6, 12, 16, 2)), ("gate", (6, 12, 16, 2)), "rc_finalmlp_fusion_workspace_bytes",
     (6, 12, 16, 2), True),
]


@pytest.mark.parametrize("answer", [100, 4096])
@pytest.mark.parametrize("cls,shape,other,query,query_args,floor", WORKSPACES, ids=lambda x: getattr(x, "__name__", None))
def test_shape_workspace(monkeypatch, cls, shape, other, query, query_args, floor, answer):
    lib = _FakeLib(answer=answer)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    ws = cls()
    assert ws._bufs == {}
    buf = ws.get(*shape, "cpu")
    assert lib.queries == [(query,) + query_args]
    assert buf.dtype == torch.uint8 and buf.device.type == "cpu" and buf.dim() == 1
    assert buf.numel() == (max(answer, 256) if floor else answer)
    # the same shape again: the same tensor object, no second query -- a captured step replays on this memory
    assert ws.get(*shape, "cpu") is buf and ws.get(*shape, torch.device("cpu")) is buf
    assert len(lib.queries) == 1 and len(ws._bufs) == 1
    # another shape, another device: buffers of their own, and the first one stays
    b2, b3 = ws.get(*other, "cpu"), ws.get(*shape, "meta")
    assert b2 is not buf and b3 is not buf and b3.device.type == "meta" and b2.data_ptr() != buf.data_ptr()
    assert len(lib.queries) == 3 and lib.queries[2] == lib.queries[0] and len(ws._bufs) == 3
    assert ws.get(*shape, "cpu") is buf and ws.get(*other, "cpu") is b2 and len(ws._bufs) == 3


# ---- the shape checks -----------------------------------------------------------------------------------------------------------------

CHECKS = [
    ("lgcn_check_shape", (16, 2), "LightGCN"), ("lgcn_check_shape", (16, 2, 10, 20), "LightGCN"),
    ("directau_check_shape", (16,), "DirectAU"), ("comirec_check_shape", (16, 8, 4, 5), "ComiRec"),
    ("contra_check_shape", (16, 3), "ContraRec"), ("buir_check_shape", (16,), "BUIR"),
    ("autoint_check_shape", (6, 16, 8, 2), "AutoInt"), ("dcnv2_check_shape", (32, 8, 2), "DCNv2"),
    ("listenc_check_shape", (5, 16, 2, 32), "list encoder"),
    ("finalmlp_check_shape", (6, 4, 8, 12, 4, 16, 12, 16, 2), "FinalMLP"),
    ("finalmlp_check_shape", (6, 4, 8, 12, 4, 16, 12, 16, 2, 0.1, 0.2), "FinalMLP"),
    ("fpmc_check_shape", (16,), "FPMC"), ("slrc_check_shape", (16, 2, 2), "SLRCPlus"), ("cfkg_check_shape", (16,), "CFKG"),
    ("din_check_shape", (16, 5, [32, 16]), "DIN attention"), ("din_check_shape", (16, 5, [32], 0.5), "DIN attention"),
    ("kda_check_shape", (16, 5, 2, 3), "KDA aggregation"), ("chorus_check_shape", (16, 2), "Chorus"),
]


@pytest.mark.parametrize("fn,args,label", CHECKS, ids=[c[0] for c in CHECKS])
def test_shape_check_raises_the_librarys_reason_under_the_models_label(monkeypatch, fn, args, label):
    monkeypatch.setattr(_lib, "load", lambda: _FakeLib(status=-4, reason=b"d = 17 is not a multiple of 4"))
    with pytest.raises(ValueError) as e:
        getattr(engine, fn)(*args)
    assert str(e.value) == label + " on the HIP engine: d = 17 is not a multiple of 4"
    monkeypatch.setattr(_lib, "load", lambda: _FakeLib())
    assert getattr(engine, fn)(*args) is None


def test_finalmlp_fusion_check_shape_probes_the_size_query(monkeypatch):
    """the sixteenth: no check entry point of its own -- a size query that answers 0 is the refusal"""
    lib = _FakeLib(answer=0, reason=b"num_heads does not divide y_dim")
    monkeypatch.setattr(_lib, "load", lambda: lib)
    with pytest.raises(ValueError) as e:
        engine.finalmlp_fusion_check_shape(12, 16, 5)
    assert str(e.value) == "FinalMLP on the HIP engine: num_heads does not divide y_dim"
    assert lib.queries == [("rc_finalmlp_fusion_workspace_bytes", 1, 12, 16, 5)]
    monkeypatch.setattr(_lib, "load", lambda: _FakeLib())
    assert engine.finalmlp_fusion_check_shape(12, 16, 4) is None
