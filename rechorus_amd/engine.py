"""Tensor-level access to the HIP engine: torch tensors are only typed device buffers
(`data_ptr()`), every FLOP happens in librechorus_hip.so on torch's current HIP stream.

Nothing here falls back to torch arithmetic: a missing library, a CPU tensor or an
unsupported shape raises.
"""
import collections
import ctypes as C
import os

import torch

from . import _lib
from ._lib import OptHyper, OPT_BY_NAME


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, dtype, name, allow_none=False):
    if t is None:
        if allow_none:
            return C.c_void_p(0)
        raise ValueError(f"{name} is required")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device}); the HIP engine has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return C.c_void_p(t.data_ptr())


def make_hyper(opt="SGD", lr=1e-3, l2=0.0, beta1=0.9, beta2=0.999, eps=None, step=1):
    """rc_opt_hyper with torch.optim's defaults (Adam eps 1e-8, Adagrad eps 1e-10, Adadelta rho 0.9 / eps 1e-6;
    Adadelta's rho travels in beta1 and is built for dense steps only)."""
    if opt not in OPT_BY_NAME:
        raise ValueError(f"optimizer {opt!r} not supported by the HIP engine (SGD, Adam, Adagrad, Adadelta)")
    if eps is None:
        eps = {"Adagrad": 1e-10, "Adadelta": 1e-6}.get(opt, 1e-8)
    return OptHyper(OPT_BY_NAME[opt], 0, float(lr), float(l2), float(beta1), float(beta2),
                    float(eps), int(step))


_ws_cache = {}
_ws_retired = []


def workspace(nbytes, device, tag="default"):
    """Cached uint8 scratch buffer (grow-only) per (device, tag).  A buffer that is outgrown is RETIRED, not
    freed: a captured hipGraph (rechorus_amd/graph.py) holds raw pointers into the buffers that were current
    at capture time, and a later, larger request (another batch shape, an evaluation pass) must not pull
    that memory from under its replays.  Growth is geometric, so retired buffers total less than the
    live one."""
    key = (str(device), tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _ws_retired.append(buf)
            nbytes = max(int(nbytes), 2 * buf.numel())
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def new_opt_state(t, opt):
    """the row-wise optimizers' state of one tensor: {} (SGD), {"m"} (Adagrad's sum of squares) or {"m", "v"} (Adam's moments)"""
    st = {"m": torch.zeros_like(t)} if opt in ("Adam", "Adagrad") else {}
    if opt == "Adam":
        st["v"] = torch.zeros_like(t)
    return st


# ---- the argument runs of the row-update entry points ---------------------------------------------------------------------------

def _table_args(W, m, v, need_W=False, tag=""):
    """(W, m, v) of one table (all null in dense-gradient mode), or of two where W, m and v are (table a, table b) pairs"""
    if isinstance(W, tuple):
        return _table_args(W[0], m[0], v[0], need_W, "_a") + _table_args(W[1], m[1], v[1], need_W, "_b")
    f32 = torch.float32
    return _ptr(W, f32, "W" + tag, not need_W), _ptr(m, f32, "m" + tag, True), _ptr(v, f32, "v" + tag, True)


def _source_args(coef, src, src_index, div, src2, n_split, default=None, need_src=True, need_src2=False):
    """(coef, src, src_index, div, src2, n_split): occurrence o < n_split brings coef[o] * src[src_index[o / div]] (no coef: 1, no
    src_index: row o / div), occurrence o >= n_split the plain row src2[o - n_split].  default: what an omitted n_split means
    to the caller -- the conventions differ, so every call site states its own"""
    f32 = torch.float32
    return (_ptr(coef, f32, "coef", True), _ptr(src, f32, "src", not need_src), _ptr(src_index, torch.int64, "src_index", True),
            int(div), _ptr(src2, f32, "src2", not need_src2), int(default if n_split is None else n_split))


def _ws_args(ws):
    """the tail of every entry point with a workspace: (scratch pointer, its size, torch's current stream)"""
    return C.c_void_p(ws.data_ptr()), ws.numel(), _stream()


def _hyper_ref(hyper):
    return C.byref(hyper) if hyper is not None else None


def _check_shape(label, entry, *ints, extra=()):
    """the body of every *_check_shape function: the library's host-side check `entry` on the integers (and whatever else `extra`
    brings: floats, a host array); its refusal is raised as a ValueError that names the model and gives the library's reason"""
    lib = _lib.load()
    if getattr(lib, entry)(*(int(x) for x in ints), *extra) != _lib.RC_OK:
        raise ValueError(label + " on the HIP engine: " + lib.rc_last_error_string().decode())


def _step_outputs(B, Cn, dev, want_pred):
    """(pred [B, C] | None, loss_vec [B], gpred [B, C]) of a fused front kernel, allocated in this order"""
    f32 = torch.float32
    pred = torch.empty((B, Cn), dtype=f32, device=dev) if want_pred else None
    return pred, torch.empty(B, dtype=f32, device=dev), torch.empty((B, Cn), dtype=f32, device=dev)


class _ShapeWorkspace:
    """The scratch of one model's kernels: one uint8 buffer per (shape, device), allocated at the size the library's query gives
    and never freed or replaced while the owner lives -- a captured hipGraph replays on its address.  A subclass is data:
    _query   the library's size query
    _shape   the names of get()'s shape arguments; get(*shape, device) takes them in this order
    _order   the same names in the order the query takes them
    _floor   the smallest allocation in bytes (256 where an empty workspace must still have an address)
    `generation` counts the forwards that stamped the workspace (stamp(): DirectAU's and ContraRec's forward wrappers), so that a
    backward can tell whether another forward has overwritten what it reads."""
    _query, _shape, _order, _floor = None, (), None, 0

    def __init__(self):
        self._bufs = {}
        self.generation = 0

    def stamp(self):
        self.generation += 1
        return self.generation

    def _buffer(self, query, key, args, device):
        key += (torch.device(device),)
        buf = self._bufs.get(key)
        if buf is None:
            nbytes = getattr(_lib.load(), query)(*args)
            buf = self._bufs[key] = torch.empty(max(nbytes, self._floor), dtype=torch.uint8, device=device)
        return buf

    def get(self, *args, **kw):
        names = self._shape + ("device",)
        given = dict(zip(names, args), **kw)
        if len(args) + len(kw) != len(names) or set(given) != set(names):
            raise TypeError(f"{type(self).__name__}.get takes ({', '.join(names)})")
        shape = {k: int(given[k]) for k in self._shape}
        return self._buffer(self._query, tuple(shape.values()), [shape[k] for k in self._order or self._shape], given["device"])


# ---- forward ---------------------------------------------------------------------------

def gather_rows(W, ids):
    """nn.Embedding forward: W[ids] (reference: models/general/BPRMF.py:39-40)."""
    ids_flat = ids.reshape(-1)
    d = W.shape[1]
    out = torch.empty((ids_flat.numel(), d), dtype=torch.float32, device=W.device)
    _lib.call("rc_gather_rows", _ptr(W, torch.float32, "W"), d, _ptr(ids_flat, torch.int64, "ids"),
              ids_flat.numel(), _ptr(out, torch.float32, "out"), _stream())
    return out.view(*ids.shape, d)


def gather_rows_pair(Wa, Wb, ids):
    """(Wa[ids] | Wb[ids]) as one [n, 2 d] block (rc_gather_rows_pair): two tables that share the ids"""
    ids_flat = ids.reshape(-1)
    d = Wa.shape[1]
    if Wb.shape[1] != d or d % 4:
        raise ValueError("gather_rows_pair: two tables of the same width, a multiple of 4")
    out = torch.empty((ids_flat.numel(), 2 * d), dtype=torch.float32, device=Wa.device)
    _lib.call("rc_gather_rows_pair", _ptr(Wa, torch.float32, "Wa"), _ptr(Wb, torch.float32, "Wb"), d, _ptr(ids_flat, torch.int64, "ids"),
              ids_flat.numel(), _ptr(out, torch.float32, "out"), _stream())
    return out


def gather_dot(U, I, uid, iid):
    """pred[b,c] = <U[uid[b]], I[iid[b,c]]> (reference: models/general/BPRMF.py:39-42)."""
    B, Cn = iid.shape
    d = U.shape[1]
    if I.shape[1] != d:
        raise ValueError("user and item tables need the same emb_size")
    pred = torch.empty((B, Cn), dtype=torch.float32, device=U.device)
    _lib.call("rc_gather_dot_fwd", _ptr(U, torch.float32, "U"), _ptr(I, torch.float32, "I"),
              _ptr(uid, torch.int64, "uid"), _ptr(iid, torch.int64, "iid"), B, Cn, d,
              _ptr(pred, torch.float32, "pred"), _stream())
    return pred


def weighted_row_sum(W, ids, coef):
    """out[b] = sum_c coef[b,c] * W[ids[b,c]]  (user-row gradient of the GMF dot)."""
    B, Cn = ids.shape
    d = W.shape[1]
    out = torch.empty((B, d), dtype=torch.float32, device=W.device)
    _lib.call("rc_weighted_row_sum", _ptr(W, torch.float32, "W"), _ptr(ids, torch.int64, "ids"),
              _ptr(coef, torch.float32, "coef"), B, Cn, d, _ptr(out, torch.float32, "out"), _stream())
    return out


# ---- loss ------------------------------------------------------------------------------

def reduce_sum(x, scale=1.0):
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    _lib.call("rc_reduce_sum", _ptr(x, torch.float32, "x"), x.numel(), float(scale),
              _ptr(out, torch.float32, "out"), _stream())
    return out


def bpr_loss(pred, inv_b=None, need_grad=True):
    """GeneralModel.loss (models/BaseModel.py:182-185) -> (loss[1], loss_vec[B], gpred|None)."""
    B, Cn = pred.shape
    if inv_b is None:
        inv_b = 1.0 / B
    loss_vec = torch.empty(B, dtype=torch.float32, device=pred.device)
    gpred = torch.empty_like(pred) if need_grad else None
    _lib.call("rc_bpr_loss_fwd_bwd", _ptr(pred, torch.float32, "pred"), B, Cn, float(inv_b),
              _ptr(loss_vec, torch.float32, "loss_vec"),
              _ptr(gpred, torch.float32, "gpred", allow_none=True), _stream())
    return reduce_sum(loss_vec, inv_b), loss_vec, gpred


def bprmf_fwd_bwd(U, I, uid, iid, inv_b=None, want_pred=True):
    """Fused gather + dot + BPR loss + backward to rows.
    Returns (pred|None, loss_vec[B], gpred[B,C], ugrad[B,d])."""
    B, Cn = iid.shape
    d = U.shape[1]
    if inv_b is None:
        inv_b = 1.0 / B
    dev = U.device
    pred, loss_vec, gpred = _step_outputs(B, Cn, dev, want_pred)
    ugrad = torch.empty((B, d), dtype=torch.float32, device=dev)
    _lib.call("rc_bprmf_fwd_bwd", _ptr(U, torch.float32, "U"), _ptr(I, torch.float32, "I"),
              _ptr(uid, torch.int64, "uid"), _ptr(iid, torch.int64, "iid"), B, Cn, d, float(inv_b),
              _ptr(pred, torch.float32, "pred", allow_none=True),
              _ptr(loss_vec, torch.float32, "loss_vec"), _ptr(gpred, torch.float32, "gpred"),
              _ptr(ugrad, torch.float32, "ugrad"), _stream())
    return pred, loss_vec, gpred, ugrad


# ---- sort + segmented update --------------------------------------------------------------

def sort_ids(ids, n_rows, ids_b=None, key_base_b=0):
    """Stable sort of a flat id list -> (keys uint32-as-int32 tensor, perm).
    ids_b: a second list sorted jointly with the first -- its ids are keyed key_base_b + id, its occurrences numbered behind the
    first list's, and n_rows bounds the joint keys."""
    ids_flat = ids.reshape(-1)
    b_flat = ids_b.reshape(-1) if ids_b is not None else None
    n_a, n_b = ids_flat.numel(), (b_flat.numel() if b_flat is not None else 0)
    n = n_a + n_b
    dev = ids.device
    keys = torch.empty(n, dtype=torch.int32, device=dev)  # bit pattern is uint32
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    nbytes = _lib.load().rc_sort_workspace_bytes(n)
    ws = workspace(nbytes, dev, "sort")
    _lib.call("rc_sort_ids", _ptr(ids_flat, torch.int64, "ids"), n_a, None if b_flat is None else _ptr(b_flat, torch.int64, "ids_b"), n_b,
              int(key_base_b), int(n_rows), _ptr(keys, torch.int32, "keys"), _ptr(perm, torch.int32, "perm"),
              *_ws_args(ws))
    return keys, perm


def bucket_plan(ids_a, range_a, ids_b=None, range_b=0, list_single_a=True):
    """rc_bucket_plan: occurrences of the ids grouped by row without a device-wide sort.
    -> dict(rows_a int32[n_rows_a, 4] (row, start, n, 0), rows_b, occ int32[n_a + n_b], single uint8[n_a] | None)
    (the uint32 fields are returned as int32 bit patterns; row counts are read back, so this wrapper synchronises --
    the training step uses the plan through rc_bprmf_train_step without any host round trip)."""
    a = ids_a.reshape(-1)
    dev = a.device
    n_a = a.numel()
    b = ids_b.reshape(-1) if ids_b is not None else None
    n_b = b.numel() if b is not None else 0
    lib = _lib.load()
    if not lib.rc_bucket_plan_supported(n_a, n_b, int(range_a), int(range_b)):
        raise _lib.RechorusHipError("rc_bucket_plan_supported", -4, "id ranges too wide for one bucket level")
    rows_a = torch.zeros((max(n_a, 1), 4), dtype=torch.int32, device=dev)
    rows_b = torch.zeros((max(n_b, 1), 4), dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    occ = torch.full((max(n_a + n_b, 1),), -1, dtype=torch.int32, device=dev)
    single = None
    if not list_single_a:
        single = torch.empty(max(lib.rc_bucket_plan_flags_bytes(n_a), 1), dtype=torch.uint8, device=dev)
    ws = workspace(lib.rc_bucket_plan_workspace_bytes(n_a, n_b), dev, "plan")
    _lib.call("rc_bucket_plan", _ptr(a, torch.int64, "ids_a") if n_a else None, n_a, int(range_a),
              _ptr(b, torch.int64, "ids_b") if n_b else None, n_b, int(range_b), 1 if list_single_a else 0,
              C.c_void_p(single.data_ptr()) if single is not None else None,
              C.c_void_p(rows_a.data_ptr()), C.c_void_p(cnt.data_ptr()),
              C.c_void_p(rows_b.data_ptr()), C.c_void_p(cnt[1:].data_ptr()),
              C.c_void_p(occ.data_ptr()), *_ws_args(ws))
    na, nb = (int(x) for x in cnt.tolist())
    return {"rows_a": rows_a[:na], "rows_b": rows_b[:nb], "occ": occ[:n_a + n_b],
            "single": None if single is None else single[:n_a]}


def bucket_multi_bitmap(ids, n_rows):
    """rc_bucket_multi_bitmap: int32 words, bit (id & 31) of word id >> 5 = 1 iff row id occurs at least twice in `ids`
    (words of id ranges the batch does not touch are unspecified: the buffer is NOT zero-filled)."""
    a = ids.reshape(-1)
    lib = _lib.load()
    n = a.numel()
    bm = torch.empty(max(lib.rc_bucket_bitmap_bytes(int(n_rows)) // 4, 1), dtype=torch.int32, device=a.device)
    ws = workspace(lib.rc_bucket_plan_workspace_bytes(n, 0), a.device, "plan")
    _lib.call("rc_bucket_multi_bitmap", _ptr(a, torch.int64, "ids") if n else None, n, int(n_rows), C.c_void_p(bm.data_ptr()),
              *_ws_args(ws))
    return bm


class Plan:
    """Device-side result of rc_bucket_plan (no host round trip: the row counts stay in device memory and the consumers
    read them there).  Buffers are cached per (device, tag) and reused every step -- two plans that are alive at the same
    time need different tags.  list_single_a=False: rows of list a that occur once are not listed but flagged in
    self.single (uint8 per position), for consumers that update them elsewhere (rc_owner_backward).
    Negative ids take no part."""

    def __init__(self, ids_a, range_a, ids_b=None, range_b=0, tag="plan", list_single_a=True):
        a = ids_a.reshape(-1)
        b = ids_b.reshape(-1) if ids_b is not None else None
        dev = a.device
        self.n_a, self.n_b = a.numel(), (b.numel() if b is not None else 0)
        lib = _lib.load()
        if not lib.rc_bucket_plan_supported(self.n_a, self.n_b, int(range_a), int(range_b)):
            raise _lib.RechorusHipError("rc_bucket_plan_supported", -4, "no plan geometry for these id ranges / list lengths")
        n = self.n_a + self.n_b
        na16, nb16 = 16 * max(self.n_a, 1), 16 * max(self.n_b, 1)
        r256 = lambda x: (x + 255) // 256 * 256
        o_b = r256(na16)
        o_occ = o_b + r256(nb16)
        o_cnt = o_occ + r256(4 * max(n, 1))
        o_single = o_cnt + 256
        n_single = 0 if list_single_a else max(int(lib.rc_bucket_plan_flags_bytes(self.n_a)), 1)
        buf = workspace(o_single + n_single, dev, tag + ".out")
        self.rows_a, self.rows_b = buf[:na16], buf[o_b:o_b + nb16]
        self.occ, self.cnt = buf[o_occ:o_occ + 4 * max(n, 1)], buf[o_cnt:o_cnt + 8]
        self.single = None if list_single_a else buf[o_single:o_single + n_single][:self.n_a]
        self.tag, self.device = tag, dev
        ws = workspace(lib.rc_bucket_plan_workspace_bytes(self.n_a, self.n_b), dev, tag + ".ws")
        p = lambda t: C.c_void_p(t.data_ptr())
        _lib.call("rc_bucket_plan", _ptr(a, torch.int64, "ids_a") if self.n_a else None, self.n_a, int(range_a),
                  _ptr(b, torch.int64, "ids_b") if self.n_b else None, self.n_b, int(range_b), 1 if list_single_a else 0,
                  None if list_single_a else p(buf[o_single:]),
                  p(self.rows_a), p(self.cnt), p(self.rows_b), p(self.cnt[4:]), p(self.occ), p(ws), ws.numel(), _stream())
        self._ws = ws
        self.upd_counters = None    # prezero_update_counters: {side: counters zero-filled ahead for that side's next update_pair}
        if _PLAN_CHECK:     # RC_PLAN_CHECK=1: every plan reads its status word back (a host sync per plan: debugging only)
            self.check()

    def status(self):
        """the plan's status word (rc_bucket_plan_status_ptr; synchronises): 0 ok, 1 an id outside its table, 2 hashed bucket overflow"""
        if self.n_a + self.n_b == 0:
            return 0
        addr = _lib.load().rc_bucket_plan_status_ptr(C.c_void_p(self._ws.data_ptr()), self.n_a, self.n_b)
        off = (addr - self._ws.data_ptr()) // 4
        return int(self._ws.view(torch.int32)[off].item())

    def check(self):
        st = self.status()
        if st:
            raise _lib.RechorusHipError("rc_bucket_plan", -1, {1: "an id lies outside its table (nn.Embedding would raise)",
                                                               2: "a hashed bucket overflowed: the plan is incomplete"}.get(st, str(st)))

    def row_sums(self, side, out, coef=None, src=None, src_index=None, div=1, src2=None, n_split=None):
        """rc_plan_row_sums on list `side`: out[row] = summed gradient row of every listed row (other rows untouched)"""
        d = out.shape[1]
        n = self.n_a + self.n_b
        if n == 0:
            return out
        ws = workspace(_lib.load().rc_plan_update_workspace_bytes(n, d), out.device, self.tag + ".upd")
        _lib.call("rc_plan_row_sums", _ptr(out, torch.float32, "out"), d, *self._records(side),
                  *self._sources(coef, src, src_index, div, src2, n_split), *_ws_args(ws))
        return out

    def distinct(self, side):
        """-> (uniq int64 [list length] (the first *count entries are valid), inverse int64 [list length], count int32 [1] on the
        device): the distinct ids of the list in the plan's record order and every position's index into them"""
        rows, cnt, base = self._side(side)
        n_list = self.n_a if side == "a" else self.n_b
        uniq = torch.empty(max(n_list, 1), dtype=torch.int64, device=self.device)
        inverse = torch.empty(max(n_list, 1), dtype=torch.int64, device=self.device)
        p = lambda t: C.c_void_p(t.data_ptr())
        _lib.call("rc_plan_distinct", p(rows), p(cnt), p(self.occ), base, n_list, p(uniq), p(inverse), _stream())
        return uniq, inverse[:n_list], cnt[:4].view(torch.int32)

    def _side(self, side):
        return (self.rows_a, self.cnt, 0) if side == "a" else (self.rows_b, self.cnt[4:], self.n_a)

    def _records(self, side):
        """(row records of list `side`, their count, the occurrence list, its length) as the update entry points take them"""
        rows, cnt, _ = self._side(side)
        return C.c_void_p(rows.data_ptr()), C.c_void_p(cnt.data_ptr()), C.c_void_p(self.occ.data_ptr()), self.n_a + self.n_b

    def _sources(self, coef, src, src_index, div, src2, n_split):
        """gradient sources as in segmented_update2 (positions of list b start at n_a).  An omitted n_split: every occurrence takes
        `src` -- or, where only src2 is given, every occurrence takes src2"""
        return _source_args(coef, src, src_index, div, src2, n_split, default=self.n_a + self.n_b if src2 is None else 0,
                            need_src=False)

    def update_pair(self, side, Wa, Wb, src_a, src_b, hyper, ma=None, va=None, mb=None, vb=None, ws_tag=""):
        """rc_plan_update_pair on list `side` ('a' | 'b'): two tables sharing the ids, per-occurrence gradient rows.
        ws_tag: suffix of the scratch buffer's cache key -- two updates that run at the same time on two streams need two.
        src_b=None: src_a is ONE block [n, >= 2 d] whose rows hold (gradient of table a | gradient of table b) side by side
        (the block is read where it lies, no contiguous halves)"""
        d = Wa.shape[1]
        f32 = torch.float32
        if src_b is None:
            if src_a.dim() != 2 or src_a.stride(1) != 1 or src_a.shape[1] < 2 * d or src_a.stride(0) % 4:
                raise ValueError("update_pair: a block source is [n, >= 2 d] with unit column stride and a row stride that is a multiple of 4")
            srcs = (C.c_void_p(src_a.data_ptr()), None, int(src_a.stride(0)))
        else:
            srcs = (_ptr(src_a, f32, "src_a"), _ptr(src_b, f32, "src_b"), 0)
        base = self._side(side)[2]
        ws = workspace(_lib.load().rc_plan_update_workspace_bytes(self.n_a + self.n_b, 2 * d), Wa.device, self.tag + ".upd" + ws_tag)
        # ticket counters that were zero-filled with the plan (prezero_update_counters: beside other work, on the plan's stream);
        # one use each -- the memset in front of the update, a launch on the step's critical path, is left out
        zc = self.upd_counters
        c = zc.pop(side) if (zc is not None and side in zc) else None
        if c is not None:
            c.record_stream(torch.cuda.current_stream(c.device))
        _lib.call("rc_plan_update_pair", *_table_args((Wa, Wb), (ma, mb), (va, vb), need_W=True), d, *self._records(side),
                  *srcs, base, C.byref(hyper), C.c_void_p(c.data_ptr()) if c is not None else None, *_ws_args(ws))

    def prezero_update_counters(self):
        """zero-fill the ticket counters of one later update_pair per side NOW, on the current stream (the plan's: beside the work the
        plan is built beside) -- update_pair then runs without its own memset"""
        z = torch.zeros(16, dtype=torch.int32, device=self.occ.device)
        self.upd_counters = {"a": z[:8], "b": z[8:]}

    def update(self, side, W, hyper, m=None, v=None, coef=None, src=None, src_index=None, div=1, src2=None, n_split=None):
        """rc_plan_update on list `side`: the optimizer step of every listed row from its summed gradient row"""
        d = W.shape[1]
        ws = workspace(_lib.load().rc_plan_update_workspace_bytes(self.n_a + self.n_b, d), W.device, self.tag + ".upd")
        _lib.call("rc_plan_update", *_table_args(W, m, v, need_W=True), d, *self._records(side),
                  *self._sources(coef, src, src_index, div, src2, n_split), C.byref(hyper), *_ws_args(ws))


def plan_supported(n_a, n_b, range_a, range_b):
    return bool(_lib.load().rc_bucket_plan_supported(int(n_a), int(n_b), int(range_a), int(range_b)))


def segment_heads(keys, perm, only_multi=False, want_single=True, want_heads=True):
    """One pass over sorted ids -> (single uint8[n]|None, heads int32[n]|None, n_heads int32[1]|None)."""
    n = keys.numel()
    dev = keys.device
    single = torch.empty(n, dtype=torch.uint8, device=dev) if want_single else None
    heads = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if want_heads else None
    n_heads = torch.zeros(1, dtype=torch.int32, device=dev) if want_heads else None
    _lib.call("rc_segment_heads", _ptr(keys, torch.int32, "keys"), _ptr(perm, torch.int32, "perm"), n,
              1 if only_multi else 0, _ptr(single, torch.uint8, "single", True),
              _ptr(heads, torch.int32, "heads", True), _ptr(n_heads, torch.int32, "n_heads", True),
              _stream())
    return single, heads, n_heads


def mark_singletons(keys, perm):
    """uint8 flag per occurrence: 1 iff its row occurs exactly once in the batch."""
    return segment_heads(keys, perm, want_heads=False)[0]


def bprmf_fwd_bwd_update(U, I, uid, iid, single, hyper, mI=None, vI=None, inv_b=None, want_pred=False, multi=None):
    """Fused fwd/loss/bwd that also applies the optimizer to single-occurrence item rows: `single` = uint8 flag per batch
    position (segment_heads), or `multi` = the bitmap over item ids of bucket_multi_bitmap (single = None)."""
    B, Cn = iid.shape
    d = U.shape[1]
    if inv_b is None:
        inv_b = 1.0 / B
    dev = U.device
    f32 = torch.float32
    pred, loss_vec, gpred = _step_outputs(B, Cn, dev, want_pred)
    ugrad = torch.empty((B, d), dtype=f32, device=dev)
    _lib.call("rc_bprmf_fwd_bwd_update", _ptr(U, f32, "U"), _ptr(I, f32, "I"),
              _ptr(mI, f32, "mI", True), _ptr(vI, f32, "vI", True),
              _ptr(uid, torch.int64, "uid"), _ptr(iid, torch.int64, "iid"),
              _ptr(single, torch.uint8, "single", True), _ptr(multi, torch.int32, "multi", True),
              B, Cn, d, float(inv_b), C.byref(hyper),
              _ptr(pred, f32, "pred", True), _ptr(loss_vec, f32, "loss_vec"),
              _ptr(gpred, f32, "gpred"), _ptr(ugrad, f32, "ugrad"), _stream())
    return pred, loss_vec, gpred, ugrad


def segmented_update(keys, perm, src, hyper=None, W=None, m=None, v=None, coef=None,
                     src_index=None, div=1, dense_grad=None, skip_singletons=False, heads=None,
                     n_heads=None, src2=None, n_split=None, key_base=0, occ_base=0):
    """rc_segmented_update: per distinct row r, grad_r = sum coef[o]*src[srow(o)], then either
    write dense_grad[r] or apply the optimizer to W[r] (and m, v) in place.
    n_split (with src2): occurrences >= n_split take plain rows src2[o - n_split].
    key_base, occ_base: keys / perm are a slice of a joint sort (sort_ids with a second list) -- what the slice's keys and
    occurrence numbers start at."""
    n_occ = keys.numel()
    d = src.shape[-1]
    ws = workspace(_lib.load().rc_segmented_workspace_bytes(n_occ, d), keys.device, "seg")
    # an omitted n_split: every occurrence takes `src`; a given one needs its src2
    _lib.call("rc_segmented_update", *_table_args(W, m, v), d, _ptr(keys, torch.int32, "keys"), _ptr(perm, torch.int32, "perm"), n_occ,
              *_source_args(coef, src, src_index, div, src2, n_split, default=n_occ, need_src2=n_split is not None),
              int(key_base), int(occ_base), _hyper_ref(hyper), _ptr(dense_grad, torch.float32, "dense_grad", allow_none=True),
              _ptr(heads, torch.int32, "heads", True), _ptr(n_heads, torch.int32, "n_heads", True),
              _lib.RC_SEG_SKIP_SINGLETONS if skip_singletons else 0, *_ws_args(ws))


def segmented_update_pair(keys, perm, src_a, src_b, hyper=None, W=(None, None), m=(None, None), v=(None, None),
                          dense_grad=(None, None), heads=None, n_heads=None):
    """rc_segmented_update_pair: two tables with the same ids (NeuMF's mf / mlp embeddings) in one pass.
    src_a, src_b [n_occ, d] per-occurrence gradient rows; W / m / v / dense_grad are (table a, table b) pairs."""
    n_occ = keys.numel()
    d = src_a.shape[-1]
    f32 = torch.float32
    ws = workspace(_lib.load().rc_segmented_workspace_bytes(n_occ, 2 * d), keys.device, "seg")
    _lib.call("rc_segmented_update_pair", *_table_args(tuple(W), tuple(m), tuple(v)), d,
              _ptr(keys, torch.int32, "keys"), _ptr(perm, torch.int32, "perm"), n_occ, _ptr(src_a, f32, "src_a"),
              _ptr(src_b, f32, "src_b"), _hyper_ref(hyper),
              _ptr(dense_grad[0], f32, "dense_grad_a", True), _ptr(dense_grad[1], f32, "dense_grad_b", True),
              _ptr(heads, torch.int32, "heads", True), _ptr(n_heads, torch.int32, "n_heads", True), *_ws_args(ws))


def segmented_pair_supported(d):
    return 2 * d in (16, 32, 64, 128, 256)


_EDB_PLAN_MIN = int(os.environ.get("RC_EDB_PLAN_MIN", "8192"))
_EDB_SMALL = os.environ.get("RC_EDB_SMALL", "1") != "0"   # embedding_dense_backward of a small id list: rc_small_row_sums
_EDB_SMALL_MAX = int(os.environ.get("RC_EDB_SMALL_MAX", "8192"))
# A/B switch: RC_TABLE_UPDATE=sort puts NeuMF's table update behind the radix sort instead of the bucket plan (hashed buckets:
# 0.33 M lookups over 10 M - 100 M rows).  SasrecTrainer's update is always sort-driven: 0.6 M occurrences over 8.7 K rows are
# all hot rows, where it measured faster (table_update 0.27 ms against 0.44 ms through the narrow-bucket plan,
# profiles/r03d_bench_sasrec*.json)
_USE_PLAN = os.environ.get("RC_TABLE_UPDATE", "auto") != "sort"
# sorted ids of a table whose rows collect many occurrences each: rc_segmented_update_rows (RC_SEG_ROWS=0: the head-list route)
_SEG_ROWS = os.environ.get("RC_SEG_ROWS", "1") != "0"
_PLAN_CHECK = os.environ.get("RC_PLAN_CHECK", "0") == "1"        # every engine.Plan verifies its status word (host sync; debugging)
_NEUMF_OVERLAP = os.environ.get("RC_NEUMF_OVERLAP", "1") != "0"   # NeumfTrainer: bucket plan beside the head kernels
_NEUMF_FUSED = os.environ.get("RC_NEUMF_FUSED", "1") != "0"       # NeumfTrainer: rc_neumf_train_step (A/B against the three-kernel step)
# SasrecTrainer runs its step on two streams (SasrecTrainer._step_item_stream) from this many candidate + history occurrences
# of the batch on
_SAS_OVERLAP_MIN = int(os.environ.get("RC_SAS_OVERLAP_MIN", "131072"))
_SEG_ROWS_MIN_PER_ROW = int(os.environ.get("RC_SEG_ROWS_MIN_PER_ROW", "8"))
# SasrecTrainer on the one-wave-per-row route: row bounds from a counting sort of item_id + history_items (RowsPlan) instead of the
# radix sort and its tensor glue (RC_SAS_ROWS_PLAN=0: the sorted route, same results bit for bit)
_SAS_ROWS_PLAN = os.environ.get("RC_SAS_ROWS_PLAN", "1") != "0"


def unique_ids(ids, n_rows, tag="unique"):
    """distinct ids + inverse index through the bucket plan (rc_bucket_plan + rc_plan_distinct) -- what
    torch.unique(ids, return_inverse=True) gives, except that the distinct ids come in the plan's order, not sorted.
    Reads the count back (one host sync, like torch.unique): callers on a hot path run it on a side stream."""
    flat = ids.reshape(-1)
    if flat.numel() == 0:
        return flat.clone(), flat.clone()
    if not plan_supported(flat.numel(), 0, n_rows, 0):   # no plan geometry for this list: torch's sort-based unique (sorted ids)
        return torch.unique(flat, return_inverse=True)
    uniq, inverse, cnt = Plan(flat, n_rows, tag=tag).distinct("a")
    return uniq[:int(cnt.item())], inverse


def unique_ids_begin(ids, n_rows, tag="unique"):
    """unique_ids without the host sync: -> (uniq_full int64 [n] (the first count entries are valid), inverse, count int32 [1] on the
    device -- a copy: the plan's own counter is overwritten by the next plan with this tag), or None where the list has no plan
    geometry (the caller falls back to unique_ids).  Several lists' counts can then be read back with ONE synchronisation."""
    flat = ids.reshape(-1)
    if flat.numel() == 0 or not plan_supported(flat.numel(), 0, n_rows, 0):
        return None
    uniq, inverse, cnt = Plan(flat, n_rows, tag=tag).distinct("a")
    return uniq, inverse, cnt[:1].clone()


def small_route_ok(n_ids, n_rows, d):
    """embedding_dense_backward(route="small") takes rc_small_row_sums for this shape"""
    return bool(_EDB_SMALL and 0 < n_ids <= _EDB_SMALL_MAX and _lib.load().rc_small_row_sums_supported(int(n_ids), int(n_rows), int(d)))


def embedding_dense_backward(grad_out, ids, n_rows, route=None, presorted=None, small_again=False, small_tag="edb_small"):
    """aten::embedding_dense_backward: G [n_rows, d] = index_add of the per-occurrence gradient rows, in ascending
    position order per row (no float atomics) -- bucket plan + rc_plan_row_sums; radix sort + segmented sum where no
    plan geometry exists.  presorted = sort_ids(ids, n_rows) of a caller that sorted the same ids already (route "sort").
    route "small" with small_again=True: the caller vouches that the preceding call on workspace `small_tag` grouped these very
    ids (a second table family gathered with the same ids): only the row sums run (rc_small_row_sums_planned)."""
    d = grad_out.shape[-1]
    flat = ids.reshape(-1)
    G = torch.zeros((n_rows, d), dtype=torch.float32, device=grad_out.device)
    if flat.numel() == 0:
        return G
    go = grad_out.reshape(-1, d).contiguous()
    # route="small": a small id list WITHOUT very hot rows (the reference's own batch sizes: user / candidate ids, the fields of a
    # CTR row) in two launches -- 128 workgroups group the ids in LDS, one lane-group per touched row sums its occurrences
    # (rc_small_row_sums).  Up to 8,192 ids a plan workgroup's buffers hold the whole list, so the grouping cannot leave LDS; a row
    # with thousands of occurrences (the padding id of a padded history: measured 0.27 against 0.11 s per SASRec epoch) is still
    # summed by ONE wave there, which is why the caller has to ask for this route
    n_ids = flat.numel()
    if route == "small" and small_route_ok(n_ids, n_rows, d):
        ws = workspace(_lib.load().rc_small_row_sums_workspace_bytes(n_ids), go.device, small_tag)
        src, out, ws_args = _ptr(go, torch.float32, "grad_out"), _ptr(G, torch.float32, "G"), _ws_args(ws)
        if small_again:
            _lib.call("rc_small_row_sums_planned", n_ids, int(n_rows), src, d, out, *_NO_PAIR, *_NO_NUMERIC, None, None, None, *ws_args)
        else:
            _lib.call("rc_small_row_sums", _ptr(flat, torch.int64, "ids"), n_ids, int(n_rows), src, d, out, *_NO_PAIR, *_NO_NUMERIC, *ws_args)
        return G
    # (below a few thousand ids both routes are a handful of latency-bound launches; the plan pays off with the batch)
    # route="sort": id lists with very hot rows (the categorical fields of the CTR models: 131,072 occurrences of 7 weekdays) --
    # a plan bucket counts its ids with LDS atomics, which such a row serialises (15.8 ms per DeepFM step at B = 131,072)
    if route != "sort" and d in (16, 32, 64, 128, 256) and flat.numel() >= _EDB_PLAN_MIN and plan_supported(flat.numel(), 0, n_rows, 0):
        return Plan(flat, n_rows, tag="edb").row_sums("a", G, src2=go)
    keys, perm = presorted if presorted is not None else sort_ids(flat, n_rows)
    segmented_update(keys, perm, go, dense_grad=G)
    return G


SMALL_NUMERIC_MAX = 4      # numeric fields that can ride in the small route's row-sums launch (kSmallNumeric)
_NO_PAIR = (None, None)                                          # src1, out1
_NO_NUMERIC = (None, None, None, None, 0, 0, 0, 0, None, None)   # values, per_row, kind, field, n_numeric, F, B, C, dW, dw1


def _numeric_arrays(values, fields, dev, d=None, want_dw1=True):
    """the host arrays that describe numeric fields to the library (rc_numeric_field_grads' values / per_row / kind / field / dW /
    dw1) and fresh outputs: -> ((val_arr, per_row, kind_arr, field_arr), dW [J, d, 1] | None, dW_arr, dw1 [J, 1, 1] | None, dw1_arr)"""
    J, f32 = len(values), torch.float32
    dW = torch.empty((J, d, 1), dtype=f32, device=dev) if d is not None else None
    dw1 = torch.empty((J, 1, 1), dtype=f32, device=dev) if want_dw1 else None
    arrays = ((C.c_void_p * J)(*[_ptr(x, x.dtype, "values").value for x in values]),
              (C.c_int * J)(*[1 if x.dim() == 1 else 0 for x in values]),
              (C.c_int * J)(*[field_kind(x) for x in values]),
              (C.c_int * J)(*[int(f) for f in fields]))
    ptrs = lambda t: None if t is None else (C.c_void_p * J)(*[t[j].data_ptr() for j in range(J)])
    return arrays, dW, ptrs(dW), dw1, ptrs(dw1)


def _riding_numeric(who, numeric, d, shape, dev):
    """numeric = (values, fields, ...) | None of the small route, shape = (F, B, n_cand)
    -> (rc_small_row_sums' ten numeric arguments, dW list | None, dw1 list | None)"""
    F, B, n_cand = (int(x) for x in shape)
    if numeric is None:
        return (None, None, None, None, 0, F, B, n_cand, None, None), None, None
    values, fields = numeric[:2]
    J = len(values)
    if not (16 <= d <= 128 and d % 4 == 0 and 1 <= J <= SMALL_NUMERIC_MAX):
        raise ValueError("%s: the numeric fields ride with d in 16 .. 128 and at most %d of them" % (who, SMALL_NUMERIC_MAX))
    arrays, dW, dW_arr, dw1, dw1_arr = _numeric_arrays(values, fields, dev, d)
    return (*arrays, J, F, B, n_cand, dW_arr, dw1_arr), [dW[j] for j in range(J)], [dw1[j] for j in range(J)]


def small_row_sums_pair(cid, n_rows, src_a, src_b, into=None, numeric=None):
    """two dense gradients [n_rows, d_a], [n_rows, d_b] of per-occurrence rows src_a [n, d_a], src_b [n, d_b] that share their ids:
    ONE zero fill (both live in one buffer), ONE grouping: rc_small_row_sums with the second source riding (d_b = 1, d_a >= 16),
    else rc_small_row_sums, then rc_small_row_sums_planned for the second on the same workspace.
    into: a float buffer of n_rows * (d_a + d_b) elements that is NOT zero-filled -- only the rows of `cid` are written (the
    kernels assign row sums), for a consumer that reads only those (dense_update_rows(touched=True))
    numeric = (values, fields, F, n_cand): the weight gradients of the numeric fields of the same gradient blocks (src_a = gV
    [rows * F, d], src_b = gL [rows * F, 1]) by extra workgroups of the row-sums launch -> (Ga, Gb, dW list, dw1 list)"""
    n, f32 = cid.numel(), torch.float32
    d_a, d_b = src_a.shape[1], src_b.shape[1]
    G = torch.zeros(n_rows * (d_a + d_b), dtype=f32, device=src_a.device) if into is None else into
    Ga, Gb = G[:n_rows * d_a].view(n_rows, d_a), G[n_rows * d_a:].view(n_rows, d_b)
    ws = workspace(_lib.load().rc_small_row_sums_workspace_bytes(n), src_a.device, "edb_small_pair")
    ws_args = _ws_args(ws)
    rides = d_b == 1 and d_a >= 16      # the one-float-wide table rides in the vectors' row-sums launch
    if numeric is not None and not rides:
        raise ValueError("small_row_sums_pair: the numeric fields ride with d in 16 .. 128 beside a one-float-wide second source")
    shape = (0, 0, 0) if numeric is None else (numeric[2], numeric[0][0].shape[0], numeric[3])      # F, B, n_cand
    num_args, dW, dw1 = _riding_numeric("small_row_sums_pair", numeric, d_a, shape, src_a.device)
    pair = (_ptr(src_b, f32, "src_b"), C.c_void_p(Gb.data_ptr()))
    _lib.call("rc_small_row_sums", _ptr(cid.reshape(-1), torch.int64, "ids"), n, int(n_rows), _ptr(src_a, f32, "src_a"), d_a,
              C.c_void_p(Ga.data_ptr()), *(pair if rides else _NO_PAIR), *num_args, *ws_args)
    if not rides:
        _lib.call("rc_small_row_sums_planned", n, int(n_rows), pair[0], d_b, pair[1], *_NO_PAIR, *_NO_NUMERIC, None, None, None, *ws_args)
    return (Ga, Gb) if numeric is None else (Ga, Gb, dW, dw1)


def small_row_sums_planned(plan_ws, n, n_rows, src_a, src_b, d, shape, into=None, numeric=None, fm=None):
    """small_row_sums_pair on a grouping that gather_fields(plan=True) built during the forward pass (rc_small_row_sums_planned: ONE
    launch): src_a [n, d] | None, src_b [n, 1]; shape = (F, B, n_cand) with n = B * n_cand * F; numeric = (values, fields, F, n_cand)
    as small_row_sums_pair;
    fm = (V [rows, F, d], S [rows, d], g [rows]): the FM pairwise term's backward is added to src_a's rows where they are read
    (src_a may then be None) -> (Ga, Gb) or (Ga, Gb, dW list, dw1 list)"""
    dev, f32 = src_b.device, torch.float32
    G = torch.zeros(n_rows * (d + 1), dtype=f32, device=dev) if into is None else into
    Ga, Gb = G[:n_rows * d].view(n_rows, d), G[n_rows * d:].view(n_rows, 1)
    num_args, dW, dw1 = _riding_numeric("small_row_sums_planned", numeric, d, shape, dev)
    fm_V, fm_S, fm_g = (None, None, None) if fm is None else fm
    _lib.call("rc_small_row_sums_planned", n, int(n_rows), _ptr(src_a, f32, "src_a", True), int(d), C.c_void_p(Ga.data_ptr()),
              _ptr(src_b, f32, "src_b"), C.c_void_p(Gb.data_ptr()), *num_args,
              _ptr(fm_V, f32, "fm_V", True), _ptr(fm_S, f32, "fm_S", True), _ptr(fm_g, f32, "fm_g", True),
              C.c_void_p(plan_ws.data_ptr()), plan_ws.numel(), _stream())
    return (Ga, Gb) if numeric is None else (Ga, Gb, dW, dw1)


def dense_update(W, G, hyper, m=None, v=None):
    """Exact torch.optim step over a whole tensor (helpers/BaseRunner.py:206)."""
    _lib.call("rc_dense_update", _ptr(W, torch.float32, "W"), _ptr(G, torch.float32, "G"),
              _ptr(m, torch.float32, "m", allow_none=True),
              _ptr(v, torch.float32, "v", allow_none=True), W.numel(), C.byref(hyper), _stream())


def dense_update_multi(items, opt, step_dev=None, increment=True):
    """items: list of (W, G, hyper, m | None, v | None) -> one launch per 36 tensors (rc_dense_update_multi).
    step_dev: int64 device tensor [1] holding Adam's step count (hipGraph-capturable mode): it is incremented
    on the stream (unless the caller already did: increment=False), then read by the update kernel"""
    T = len(items)
    if T == 0:
        return
    f32 = torch.float32
    Wa = (C.c_void_p * T)(*[_ptr(w, f32, "W").value for w, _, _, _, _ in items])
    Ga = (C.c_void_p * T)(*[_ptr(g, f32, "G").value for _, g, _, _, _ in items])
    Ma = (C.c_void_p * T)(*[_ptr(m, f32, "m", True).value for _, _, _, m, _ in items])
    Va = (C.c_void_p * T)(*[_ptr(v, f32, "v", True).value for _, _, _, _, v in items])
    na = (C.c_int64 * T)(*[w.numel() for w, _, _, _, _ in items])
    ha = (OptHyper * T)(*[h for _, _, h, _, _ in items])
    if step_dev is not None and increment:
        _lib.call("rc_step_increment", _ptr(step_dev, torch.int64, "step_dev"), _stream())
    _lib.call("rc_dense_update_multi", Wa, Ga, Ma, Va, na, ha, T, _ptr(step_dev, torch.int64, "step_dev", True), _stream())


def dense_update_rows(items, step_dev, touched=2, max_blocks=0):
    """items: list of (W, G | None, hyper, m, v, flags | None, row_w) -> rc_dense_update_rows_dev: Adam over W without a dense
    gradient -- touched=2: every row, g = G's row where the row's int32 flag equals the step and 0 elsewhere (the rest of G is
    never read); touched=1 / 0: only the stamped rows (from G) / only the others (g = 0).  flags None = the whole tensor from G.
    The step count was already incremented for this step.  max_blocks > 0: grid cap."""
    T = len(items)
    if T == 0:
        return
    f32 = torch.float32
    Wa = (C.c_void_p * T)(*[_ptr(it[0], f32, "W").value for it in items])
    Ga = (C.c_void_p * T)(*[_ptr(it[1], f32, "G", True).value for it in items])
    Ma = (C.c_void_p * T)(*[_ptr(it[3], f32, "m").value for it in items])
    Va = (C.c_void_p * T)(*[_ptr(it[4], f32, "v").value for it in items])
    na = (C.c_int64 * T)(*[it[0].numel() for it in items])
    Fa = (C.c_void_p * T)(*[_ptr(it[5], torch.int32, "flags", True).value for it in items])
    ra = (C.c_int * T)(*[int(it[6]) for it in items])
    ha = (OptHyper * T)(*[it[2] for it in items])
    _lib.call("rc_dense_update_rows_dev", Wa, Ga, Ma, Va, na, Fa, ra, ha, T, int(touched), int(max_blocks),
              _ptr(step_dev, torch.int64, "step_dev"), _stream())


# ---- whole BPRMF step -----------------------------------------------------------------------

class BprmfTrainer:
    """Row-wise-optimizer BPRMF training on device tables U [n_users,d], I [n_items,d].

    One `step(uid, iid)` = one iteration of BaseRunner.fit's batch loop
    (helpers/BaseRunner.py:193-206) for models/general/BPRMF.py, as one C-ABI call.
    """

    def __init__(self, U, I, opt="SGD", lr=1e-3, l2=0.0, beta1=0.9, beta2=0.999, eps=None):
        if U.shape[1] != I.shape[1]:
            raise ValueError("user and item tables need the same emb_size")
        self.U, self.I = U, I
        self.d = U.shape[1]
        self.opt = opt
        self.hyper = make_hyper(opt, lr, l2, beta1, beta2, eps, step=0)
        sU, sI = new_opt_state(U, opt), new_opt_state(I, opt)
        self.mU, self.vU, self.mI, self.vI = sU.get("m"), sU.get("v"), sI.get("m"), sI.get("v")
        self.loss = torch.zeros(1, dtype=torch.float32, device=U.device)
        self._ws = None
        self._ws_shape = None
        # look-ahead across steps: the library records what it prepared in THIS caller-owned ticket (no hidden state)
        self._ticket = _lib.StepTicket()
        self._gen = 0            # generation ids handed out for announced batches
        self._announced = None   # (uid, iid, uid._version, iid._version, generation) of the batch announced last

    def _workspace(self, B, Cn):
        if self._ws_shape != (B, Cn):
            nbytes = _lib.load().rc_bprmf_step_workspace_bytes(B, Cn, self.d)
            if nbytes == 0:
                raise _lib.RechorusHipError("rc_bprmf_step_workspace_bytes", -1, "bad shape")
            if self._ws is None or self._ws.numel() < nbytes:
                if self._ws is not None:
                    self._forget_ahead()
                    _ws_retired.append(self._ws)  # a captured hipGraph may still point into it
                self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.U.device)
            self._ws_shape = (B, Cn)
        return self._ws

    def _forget_ahead(self):
        """a plan prepared by step(next_batch=...) lives in this trainer's workspace: drop it before the memory can be reused"""
        self._announced = None
        if getattr(self, "_ticket", None) is not None and self._ticket.generation != 0:
            try:
                _lib.call("rc_bprmf_step_ahead_reset", C.byref(self._ticket), _stream())
            except Exception:  # interpreter shutdown: the library / torch may be gone already
                pass

    def __del__(self):
        self._forget_ahead()

    def _generation_of(self, uid, iid):
        """generation id of (uid, iid) if it IS the batch announced by the previous step: the same tensor objects (strong
        references are held, so an address cannot have been reused) with unchanged version counters (an in-place refill
        through torch bumps them).  0 = unknown: the step plans the batch itself."""
        a = self._announced
        if a is not None and a[0] is uid and a[1] is iid and a[2] == uid._version and a[3] == iid._version:
            return a[4]
        return 0

    def step(self, uid, iid, inv_b=None, pred=None, phase_ms=None, next_batch=None, generation=None, next_generation=None):
        """Runs one training step; returns the device loss tensor (shape [1], no sync).
        phase_ms: optional ctypes float[8] to receive per-phase hipEvent timings.
        next_batch = (uid, iid) of the FOLLOWING step (same shapes): the bucket plan of those ids is prepared beside this
        step's row updates (rc_bprmf_train_step_ahead); the tensors must stay alive and unchanged until that step.
        generation / next_generation: the caller's ids of this / the following batch's CONTENTS (non-zero ints that
        change with every new batch) -- needed when batches are written into the same buffers by something torch's
        version counters do not see (a kernel writing through data_ptr()); left None, the trainer identifies the
        announced batch by tensor identity + version.  Pass them always or never."""
        B, Cn = iid.shape
        if inv_b is None:
            inv_b = 1.0 / B
        ws = self._workspace(B, Cn)
        self.hyper.step += 1
        f32 = torch.float32
        if generation is None:
            generation = self._generation_of(uid, iid)
        nu = ni = None
        ngen = 0
        if next_batch is not None and tuple(next_batch[1].shape) == (B, Cn) and tuple(next_batch[0].shape) == (B,):
            nu, ni = next_batch
            if next_generation is None:
                self._gen += 1
                ngen = self._gen
            else:
                ngen = int(next_generation)
        self._announced = (nu, ni, nu._version, ni._version, ngen) if nu is not None else None
        _lib.call("rc_bprmf_train_step_ahead",
                  _ptr(self.U, f32, "U"), _ptr(self.I, f32, "I"),
                  _ptr(self.mU, f32, "mU", True), _ptr(self.vU, f32, "vU", True),
                  _ptr(self.mI, f32, "mI", True), _ptr(self.vI, f32, "vI", True),
                  _ptr(uid, torch.int64, "uid"), _ptr(iid, torch.int64, "iid"), int(generation),
                  _ptr(nu, torch.int64, "next_uid", True), _ptr(ni, torch.int64, "next_iid", True), ngen,
                  C.byref(self._ticket), B, Cn, self.d,
                  self.U.shape[0], self.I.shape[0], C.byref(self.hyper), float(inv_b),
                  _ptr(self.loss, f32, "loss"), _ptr(pred, f32, "pred", True),
                  *_ws_args(ws),
                  phase_ms if phase_ms is not None else None)
        return self.loss

    def profile_step(self, uid, iid, next_batch=None):
        """One step with hipEvent phase timing -> dict of milliseconds (synchronises).  With next_batch (and this batch
        announced by the previous step) the profiled step is a step of the steady state: its plan was prepared ahead, the
        plan of the following batch runs on the second stream beside its phases."""
        buf = (C.c_float * 8)()
        self.step(uid, iid, phase_ms=buf, next_batch=next_batch)
        names = ["sort_items", "sort_users", "fused_fwd_bwd", "loss_mean", "item_update",
                 "user_update", "total", "segment_heads"]
        return {n: float(buf[i]) for i, n in enumerate(names)}


# ---- NeuMF head ----------------------------------------------------------------------------------

def neumf_supported(d, l1):
    return bool(_lib.load().rc_neumf_supported(int(d), int(l1)))


def _neumf_ptrs(P):
    f32 = torch.float32
    return [_ptr(P[k], f32, k) for k in ("mf_u", "mf_i", "mlp_u", "mlp_i", "W1", "b1", "w_out")]


def _drop_args(drop_p, seed):
    """(p, device pointer to the 64-bit mask seed); seed = int64 tensor [1] on the device, read by the kernels"""
    if not drop_p:
        return C.c_float(0.0), C.c_void_p(0)
    if seed is None:
        raise ValueError("dropout needs a device seed tensor (int64 [1])")
    return C.c_float(float(drop_p)), _ptr(seed, torch.int64, "seed")


_deferred_inc = None      # [counter, folded?]: an increment somebody has promised to make before its next reader runs


def defer_increment(counter):
    """The caller owes `counter[0] += 1` some time before its own later kernel reads the counter, and nothing in between reads it:
    the next step_increment of ANOTHER counter takes it along in the same launch (rc_step_increment2: in a replayed graph a launch
    costs ~4.6 us whatever it does; a DeepFM step at B = 1,024 bumps the tower's dropout seed and Adam's step count).  The caller
    settles with take_deferred before that later kernel."""
    global _deferred_inc
    _deferred_inc = [counter, False]


def take_deferred(counter):
    """settle a defer_increment: True = some step_increment folded it in (the counter is incremented), False = nobody did (the caller
    increments itself).  Either way the promise is gone."""
    global _deferred_inc
    d, _deferred_inc = _deferred_inc, None
    return d is not None and d[0] is counter and d[1]


_bumped_early = []        # counters a carrier launch has already incremented for their owner's NEXT step_increment call


def clear_bumped_early():
    """forget early increments nobody collected (a step that raised between the carrier launch and the owner's step_increment)"""
    del _bumped_early[:]


def pending_deferred():
    """the counter of an unsettled defer_increment that no launch has taken along yet, or None -- a launch with a slot for a counter
    it does not read may take it (fold_deferred after the launch is enqueued)"""
    d = _deferred_inc
    return d[0] if (d is not None and not d[1]) else None


def fold_deferred(counter):
    d = _deferred_inc
    if d is not None and d[0] is counter:
        d[1] = True


def step_increment(counter):
    """counter[0] += 1 on the device (rc_step_increment): Adam's step, the dropout seed; capturable"""
    for k, c in enumerate(_bumped_early):
        if c is counter:      # an earlier launch of this step (the field gather) incremented it on the owner's behalf
            del _bumped_early[k]
            return
    d = _deferred_inc
    if d is not None and not d[1] and d[0] is not counter and d[0].device == counter.device:
        _lib.call("rc_step_increment2", _ptr(counter, torch.int64, "counter"), _ptr(d[0], torch.int64, "deferred counter"), _stream())
        d[1] = True
        return
    _lib.call("rc_step_increment", _ptr(counter, torch.int64, "counter"), _stream())


def neumf_fwd(P, uid, iid, drop_p=0.0, seed=None):
    """P: dict mf_u, mf_i, mlp_u, mlp_i [rows,d], W1 [l1,2d], b1 [l1], w_out [d+l1] -> pred [B,C]
    (models/general/NeuMF.py:61-75).  drop_p > 0: training-mode dropout on the hidden layer, mask drawn from
    the counter-based stream keyed by seed[0]."""
    B, Cn = iid.shape
    d, l1 = P["mf_u"].shape[1], P["W1"].shape[0]
    pred = torch.empty((B, Cn), dtype=torch.float32, device=iid.device)
    _lib.call("rc_neumf_fwd", *_neumf_ptrs(P), _ptr(uid, torch.int64, "uid"), _ptr(iid, torch.int64, "iid"),
              B, Cn, d, l1, *_drop_args(drop_p, seed), _ptr(pred, torch.float32, "pred"), _stream())
    return pred


def neumf_bwd(P, uid, iid, gpred, drop_p=0.0, seed=None):
    """-> (per-occurrence row grads dict g_mf_u, g_mf_i, g_mlp_u, g_mlp_i [B*C,d], dense grads dict W1, b1, w_out);
    drop_p / seed as given to the forward this is the backward of (the mask is regenerated, not stored)"""
    B, Cn = iid.shape
    d, l1 = P["mf_u"].shape[1], P["W1"].shape[0]
    dev, f32 = iid.device, torch.float32
    rows = {k: torch.empty((B * Cn, d), dtype=f32, device=dev) for k in ("g_mf_u", "g_mf_i", "g_mlp_u", "g_mlp_i")}
    dense = {"W1": torch.empty_like(P["W1"]), "b1": torch.empty_like(P["b1"]), "w_out": torch.empty_like(P["w_out"])}
    ws = workspace(_lib.load().rc_neumf_workspace_bytes(B, Cn, d, l1), dev, "neumf")
    _lib.call("rc_neumf_bwd", *_neumf_ptrs(P), _ptr(uid, torch.int64, "uid"), _ptr(iid, torch.int64, "iid"),
              _ptr(gpred, f32, "gpred"), B, Cn, d, l1, *_drop_args(drop_p, seed),
              *[_ptr(rows[k], f32, k) for k in ("g_mf_u", "g_mf_i", "g_mlp_u", "g_mlp_i")],
              _ptr(dense["W1"], f32, "dW1"), _ptr(dense["b1"], f32, "db1"), _ptr(dense["w_out"], f32, "dw_out"),
              *_ws_args(ws))
    return rows, dense


def neumf_train_step_supported(Cn, d, l1):
    return bool(_lib.load().rc_neumf_train_step_supported(int(Cn), int(d), int(l1)))


def neumf_head_kernel_selected(Cn, d, l1):
    """the one-kernel NeuMF head (forward + BPR loss + backward: rc_neumf_train_step, rc_neumf_head_fwd_bwd) is switched on and
    has an instance for Cn candidates per tuple"""
    return bool(_NEUMF_FUSED and Cn >= 2 and neumf_train_step_supported(Cn, d, l1))


def neumf_fused_step_selected(Cn, d, l1, opt="SGD"):
    """would NeumfTrainer.step take the one-kernel step (rc_neumf_train_step) for Cn candidates per tuple?  Everything its
    selection tests except the batch's plan geometry (known only with the batch).  (Its table updates are pair updates from the
    bucket plan; every width the kernel exists for has one.)"""
    return bool(_USE_PLAN and opt in ("SGD", "Adam", "Adagrad") and neumf_head_kernel_selected(Cn, d, l1))


def neumf_mark_rows(iid, n_items, marks, unmark=False):
    """rc_neumf_mark_rows / rc_neumf_unmark_rows on torch's current stream: the single / multi-occurrence flags of a batch's item ids"""
    _lib.call("rc_neumf_unmark_rows" if unmark else "rc_neumf_mark_rows", _ptr(iid, torch.int64, "iid"), iid.numel(), int(n_items),
              C.c_void_p(marks.data_ptr()), _stream())


def neumf_train_step(P, state, uid, iid, hyper, marks, out, inv_b=None, pred=None, marked=False, drop_p=0.0, seed=None):
    """rc_neumf_train_step: forward + BPR loss + backward + in-place update of single-occurrence item rows.
    state: {table: {"m": .., "v": ..}} of the optimizer; marks: uint8 buffer of rc_neumf_train_step_marks_bytes(n_items), zeroed
    once (every call leaves it ready for the next; marked=True: prepared by neumf_mark_rows for this very batch, cleared by the caller); out: dict of preallocated buffers loss_vec [B], g_mf_i / g_mlp_i [B C, d], gu_mf / gu_mlp [B, d], W1 / b1 / w_out
    gradients.  drop_p > 0: training-mode dropout on the hidden layer inside the kernel (`seed` int64 [1]
    on the device, the mask stream of neumf_fwd / neumf_bwd).  Returns nothing: the caller finishes the step with the plan's pair
    updates and the dense update."""
    B, Cn = iid.shape
    d, l1 = P["mf_u"].shape[1], P["W1"].shape[0]
    f32 = torch.float32
    lib = _lib.load()
    ws = workspace(lib.rc_neumf_train_step_workspace_bytes(B, Cn, d, l1), iid.device, "neumf_step")
    st = lambda t, k: _ptr(state[t].get(k), f32, k + "_" + t, True)
    head = [_ptr(P["mf_u"], f32, "mf_u"), _ptr(P["mf_i"], f32, "mf_i"), _ptr(P["mlp_u"], f32, "mlp_u"),
            _ptr(P["mlp_i"], f32, "mlp_i"), st("mf_i", "m"), st("mf_i", "v"), st("mlp_i", "m"), st("mlp_i", "v"),
            _ptr(P["W1"], f32, "W1"), _ptr(P["b1"], f32, "b1"), _ptr(P["w_out"], f32, "w_out"),
            _ptr(uid, torch.int64, "uid"), _ptr(iid, torch.int64, "iid"), B, Cn, d, l1, int(P["mf_i"].shape[0]),
            C.c_void_p(marks.data_ptr())]
    tail = [_ptr(out["loss_vec"], f32, "loss_vec"), _ptr(pred, f32, "pred", True),
            _ptr(out["g_mf_i"], f32, "g_mf_i"), _ptr(out["g_mlp_i"], f32, "g_mlp_i"), _ptr(out["gu_mf"], f32, "gu_mf"),
            _ptr(out["gu_mlp"], f32, "gu_mlp"), _ptr(out["W1"], f32, "dW1"), _ptr(out["b1"], f32, "db1"),
            _ptr(out["w_out"], f32, "dw_out"), *_ws_args(ws)]
    inv = float(1.0 / B if inv_b is None else inv_b)
    _lib.call("rc_neumf_train_step", *head, 1 if marked else 0, C.byref(hyper), inv, *_drop_args(drop_p, seed), *tail)


def neumf_head_fwd_bwd(urows, irows, W1, b1, w_out, B, Cn, inv_b, want_pred=False):
    """rc_neumf_head_fwd_bwd on fetched row blocks: urows [B, 2d] = [mf_u | mlp_u] of every tuple's user, irows [B C, 2d] =
    [mf_i | mlp_i] of every candidate (the layout the sharded step's exchanges deliver).  -> (loss_vec [B], gu [B, 2d],
    gi [B C, 2d], {W1, b1, w_out gradients}, pred | None): the gradient blocks in the same [mf | mlp] layout, ready to travel back."""
    d2 = urows.shape[1]
    d, l1 = d2 // 2, W1.shape[0]
    dev, f32 = urows.device, torch.float32
    if irows.shape != (B * Cn, d2) or urows.shape[0] != B:
        raise ValueError("neumf_head_fwd_bwd: row blocks do not match B, C")
    key = ("nhead", B, Cn, d2, str(dev))
    ids = _ws_cache.get(key)
    if ids is None:   # positional ids: tuple b uses user row b and item rows b C .. b C + C - 1
        ids = _ws_cache[key] = (torch.arange(B, device=dev), torch.arange(B * Cn, device=dev).view(B, Cn))
    loss_vec = torch.empty(B, dtype=f32, device=dev)
    gu = torch.empty((B, d2), dtype=f32, device=dev)
    gi = torch.empty((B * Cn, d2), dtype=f32, device=dev)
    pred = torch.empty((B, Cn), dtype=f32, device=dev) if want_pred else None
    dense = {"W1": torch.empty_like(W1), "b1": torch.empty_like(b1), "w_out": torch.empty_like(w_out)}
    ws = workspace(_lib.load().rc_neumf_train_step_workspace_bytes(B, Cn, d, l1), dev, "neumf_step")
    _ptr(urows, f32, "urows"); _ptr(irows, f32, "irows")
    off = lambda t, k: C.c_void_p(t.data_ptr() + 4 * k)
    _lib.call("rc_neumf_head_fwd_bwd", off(urows, 0), off(urows, d), d2, off(irows, 0), off(irows, d), d2,
              _ptr(W1, f32, "W1"), _ptr(b1, f32, "b1"), _ptr(w_out, f32, "w_out"), _ptr(ids[0], torch.int64, "uid"),
              _ptr(ids[1], torch.int64, "iid"), B, Cn, d, l1, float(inv_b), _ptr(loss_vec, f32, "loss_vec"),
              _ptr(pred, f32, "pred", True), off(gi, 0), off(gi, d), d2, off(gu, 0), off(gu, d), d2,
              _ptr(dense["W1"], f32, "dW1"), _ptr(dense["b1"], f32, "db1"), _ptr(dense["w_out"], f32, "dw_out"),
              *_ws_args(ws))
    return loss_vec, gu, gi, dense, pred


def neumf_zhead_supported(Cn, d, l1):
    return bool(_lib.load().rc_neumf_zhead_supported(int(Cn), int(d), int(l1)))


def neumf_zhead(urows, irows, W1, b1, w_out, B, Cn, inv_b, want_pred=False):
    """the head of a sharded NeuMF step whose item half of the hidden layer came from the rows' owners (csrc/neumf_zhead.hip):
    urows [B, 2d] = [mf_u | mlp_u], irows [B C, d + l1] = [mf_i | zi = W1i mlp_i].  zu = W1u mlp_u + b1 and the backward of the
    user half are GEMMs (rc_linear_fwd / rc_linear_bwd), everything per candidate is rc_neumf_zhead_fwd_bwd.
    -> (loss_vec [B], gu [B, 2d] = [d mf_u | d mlp_u], gi [B C, d + l1] = [d mf_i | dz], {W1u [l1, d], b1, w_out gradients}, pred | None)"""
    d = urows.shape[1] // 2
    l1 = W1.shape[0]
    dev, f32 = urows.device, torch.float32
    if irows.shape != (B * Cn, d + l1) or urows.shape != (B, 2 * d):
        raise ValueError("neumf_zhead: row blocks do not match B, C, d, hidden")
    W1u = W1[:, :d].contiguous()
    mlp_u = urows[:, d:].contiguous()
    zu = linear_fwd(mlp_u, W1u, b1)
    loss_vec = torch.empty(B, dtype=f32, device=dev)
    gu = torch.empty((B, 2 * d), dtype=f32, device=dev)
    gi = torch.empty((B * Cn, d + l1), dtype=f32, device=dev)
    dzu = torch.empty((B, l1), dtype=f32, device=dev)
    dw_out = torch.empty(d + l1, dtype=f32, device=dev)
    pred = torch.empty((B, Cn), dtype=f32, device=dev) if want_pred else None
    ws = workspace(_lib.load().rc_neumf_zhead_workspace_bytes(d, l1), dev, "neumf_zhead")
    _lib.call("rc_neumf_zhead_fwd_bwd", _ptr(urows, f32, "urows"), 2 * d, _ptr(zu, f32, "zu"), _ptr(irows, f32, "irows"), d + l1,
              _ptr(w_out, f32, "w_out"), B, Cn, d, l1, float(inv_b), _ptr(loss_vec, f32, "loss_vec"), _ptr(pred, f32, "pred", True),
              _ptr(gi, f32, "gi"), d + l1, _ptr(gu, f32, "gu"), 2 * d, _ptr(dzu, f32, "dzu"), _ptr(dw_out, f32, "dw_out"),
              *_ws_args(ws))
    dmlp_u, dW1u, db1 = linear_bwd(mlp_u, W1u, None, dzu, ws_tag="zhead_bwd")
    gu[:, d:] = dmlp_u
    return loss_vec, gu, gi, {"W1u": dW1u, "b1": db1, "w_out": dw_out}, pred


class _PhaseTimer:
    """Optional per-phase timing of a trainer step with events on the launch stream (torch's current stream is the
    stream every kernel of the step is enqueued on).  trainer.timing = {} switches it on; read with phases_ms()."""

    def __init__(self, owner, name):
        self.t = getattr(owner, "timing", None)
        self.name = name

    def __enter__(self):
        if self.t is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.t is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            self.t.setdefault(self.name, []).append((self.a, b))


def _step_hypers(tr):
    """(the hyper-parameters of trainer tr's current step, the same without weight decay: parameters named 'bias')"""
    return make_hyper(tr.opt, lr=tr.lr, l2=tr.l2, step=tr.step_count), make_hyper(tr.opt, lr=tr.lr, l2=0.0, step=tr.step_count)


def phases_ms(trainer):
    """MEDIAN milliseconds per phase of the steps recorded since trainer.timing = {} (synchronises).  (The mean until round 6: one
    eager step of twenty that meets an allocation on a side stream -- 68 ms once -- made a 0.05 ms phase read 3.4 ms.)"""
    torch.cuda.synchronize()
    out = {}
    for k, v in (trainer.timing or {}).items():
        t = sorted(a.elapsed_time(b) for a, b in v)
        out[k] = t[len(t) // 2] if len(t) % 2 else 0.5 * (t[len(t) // 2 - 1] + t[len(t) // 2])
    return out


class NeumfTrainer:
    """One BaseRunner.fit iteration for NeuMF (single hidden layer) on device tensors:
    forward (MFMA) -> BPR loss -> backward (MFMA) -> row-wise segmented update of the four tables
    -> dense optimizer step of W1, b1, w_out.  P as in neumf_fwd; updated in place.
    dropout > 0: hidden-layer dropout with a fresh mask per step (device seed counter, bumped every step)."""

    _n_trainers = 0
    PAIRS = {"a": ("mf_i", "mlp_i"), "b": ("mf_u", "mlp_u")}    # bucket-plan list -> the two tables that share its ids

    def __init__(self, P, opt="Adam", lr=1e-3, l2=0.0, rowwise=True, dropout=0.0, seed=0):
        self.P, self.opt, self.lr, self.l2, self.rowwise = P, opt, lr, l2, rowwise
        self.dropout = float(dropout)
        self.seed = torch.tensor([seed], dtype=torch.int64, device=P["W1"].device) if self.dropout > 0 else None
        self.state = {k: new_opt_state(t, opt) for k, t in P.items()}
        self.step_count = 0
        self.loss = None
        self.timing = None                  # {} switches the per-phase events on (_PhaseTimer, phases_ms)
        self._side = self._side2 = None     # streams of the steps that run on more than one (created with the first such step)
        self._sum_idx = (None, None, None)  # three-kernel step: (B, C, device), positions and ones of the per-tuple user sums
        self._marks = None                  # fused step: two flag buffers, this batch's and (prepared beside this step's updates) the next one's
        self._fused_out = (None, None)      # ((B, C, device), the kernel's output buffers)
        self._ahead = None                  # what the previous step prepared for an announced batch (_prepare_next)
        NeumfTrainer._n_trainers += 1
        self._serial = NeumfTrainer._n_trainers     # plan workspaces are cached by tag: one set per trainer

    def __del__(self):
        try:
            # the trainer's plan workspaces leave the cache -- once the side streams that wrote them have drained (a block freed
            # with side-stream work in flight could be handed out again on the main stream)
            for st in (getattr(self, "_side", None), getattr(self, "_side2", None)):
                if st is not None:
                    st.synchronize()
            for key in [k for k in _ws_cache if isinstance(k[1], str) and k[1].startswith("neumf%d." % self._serial)]:
                _ws_cache.pop(key, None)
        except Exception:
            pass

    def step(self, uid, iid, next_batch=None):
        """next_batch = (uid, iid) of the FOLLOWING call (the very tensors it will bring, unmodified until then): the fused step
        builds their bucket plan beside this step's table updates, off the critical path."""
        P = self.P
        Cn = iid.shape[1]
        d, l1 = P["mf_u"].shape[1], P["W1"].shape[0]
        self.step_count += 1
        if self.seed is not None:
            step_increment(self.seed)
        # (every width a NeuMF kernel exists for -- 32, 64, 128 -- has a pair update kernel: no width test here)
        use_plan = self.rowwise and _USE_PLAN and plan_supported(iid.numel(), uid.numel(), P["mf_i"].shape[0], P["mf_u"].shape[0])
        if use_plan and neumf_fused_step_selected(Cn, d, l1, self.opt):
            return self._step_fused(uid, iid, next_batch)
        if not neumf_supported(d, l1):
            # (a tower that exists only inside the one-kernel step, e.g. hidden 16: say why this call cannot take it instead of
            # failing with RC_ERR_UNSUPPORTED inside rc_neumf_fwd)
            raise RuntimeError("NeumfTrainer: emb_size {} / hidden {} is a shape of the one-kernel step (rc_neumf_train_step) only, which this call "
                               "cannot take: {} candidates per tuple (needs >= 2 and the kernel's LDS budget: rc_neumf_train_step_supported), "
                               "plan {} (RC_TABLE_UPDATE, row-wise updates, a plan geometry for {} + {} ids), RC_NEUMF_FUSED={} -- use --engine "
                               "dense for this configuration".format(d, l1, Cn, "on" if use_plan else "off",
                                                                      iid.numel(), uid.numel(), int(_NEUMF_FUSED)))
        return self._step_three_kernels(uid, iid, use_plan)

    def _new_plan(self, uid, iid, buf=None):
        """the bucket plan of both id lists (items: list a); buf: for the fused step, which updates single-occurrence item rows
        itself -- they are flagged, not listed -- and alternates between two sets of plan buffers"""
        n_i, n_u = self.P["mf_i"].shape[0], self.P["mf_u"].shape[0]
        if buf is None:
            return Plan(iid, n_i, uid, n_u, tag="neumf")
        return Plan(iid, n_i, uid, n_u, tag="neumf%d.%d" % (self._serial, buf), list_single_a=False)

    def _update_pair(self, plan, side, ga, gb, h, ws_tag=""):
        """the row-wise step of the two tables behind plan list `side` from their per-occurrence gradient rows"""
        ta, tb = self.PAIRS[side]
        sa, sb = self.state[ta], self.state[tb]
        plan.update_pair(side, self.P[ta], self.P[tb], ga, gb, h, ma=sa.get("m"), va=sa.get("v"), mb=sb.get("m"), vb=sb.get("v"),
                         ws_tag=ws_tag)

    def _dense_step(self, grads, h, h0):
        with _PhaseTimer(self, "dense_update"):
            dense_update_multi([(self.P[k], grads[k], h0 if k == "b1" else h, self.state[k].get("m"), self.state[k].get("v"))
                                for k in ("W1", "b1", "w_out")], self.opt)

    def _step_three_kernels(self, uid, iid, use_plan):
        """rc_neumf_fwd, rc_bpr_loss_fwd_bwd, rc_neumf_bwd, then the table updates from the bucket plan (use_plan) or behind a sort"""
        P = self.P
        B, Cn = iid.shape
        # the bucket plan needs only the ids: on a second stream it runs beside the head kernels (large batches; a small step is
        # bound by the host's launch rate and the stream switches cost more than they return)
        overlap = use_plan and _NEUMF_OVERLAP and iid.is_cuda and iid.numel() >= _SAS_OVERLAP_MIN
        plan = plan_done = main = None
        if overlap:
            if self._side is None:
                self._side = torch.cuda.Stream(device=iid.device)
            main, side = torch.cuda.current_stream(iid.device), self._side
            side.wait_stream(main)   # the batch is ready; last step's readers of the plan buffers are done
            with torch.cuda.stream(side):
                plan = self._new_plan(uid, iid)
                plan_done = side.record_event()
        with _PhaseTimer(self, "head_fwd"):
            pred = neumf_fwd(P, uid, iid, self.dropout, self.seed)
        with _PhaseTimer(self, "loss"):
            self.loss, _, gpred = bpr_loss(pred)
        with _PhaseTimer(self, "head_bwd"):
            rows, dense = neumf_bwd(P, uid, iid, gpred, self.dropout, self.seed)
        h, h0 = _step_hypers(self)
        if use_plan:
            # ONE bucket plan of both id lists (round 3: hashed buckets where the id space is wide and sparse -- 0.33 M item
            # lookups over 10 M - 100 M rows -- so the cost follows the keys, not the id range; round 2's id-range
            # buckets cost as much as the radix sort here and the sort stayed), then one pair update per side: the
            # mf / mlp tables of a side share ids, records and positions.
            with _PhaseTimer(self, "sort"):
                if overlap:
                    main.wait_event(plan_done)
                else:
                    plan = self._new_plan(uid, iid)
            with _PhaseTimer(self, "table_update"):
                # The user side is planned per TUPLE: the head kernel's per-candidate user gradients are summed over a tuple's
                # candidates first (fixed order c = 0..C-1), so a hot user contributes B_u occurrences, not C * B_u.
                key = (B, Cn, str(uid.device))
                if self._sum_idx[0] != key:
                    self._sum_idx = (key, torch.arange(B * Cn, device=uid.device).view(B, Cn), torch.ones((B, Cn), device=uid.device))
                _, pos, ones = self._sum_idx
                gu_a, gu_b = weighted_row_sum(rows["g_mf_u"], pos, ones), weighted_row_sum(rows["g_mlp_u"], pos, ones)
                self._update_pair(plan, "b", gu_a, gu_b, h)
                self._update_pair(plan, "a", rows["g_mf_i"], rows["g_mlp_i"], h)
        else:
            self._step_tables_sorted(uid.repeat_interleave(Cn), iid, rows, h)
        self._dense_step(dense, h, h0)
        return self.loss

    def _step_tables_sorted(self, uid_occ, iid, rows, h):
        """the table updates behind a radix sort (dense-gradient mode = the reference's exact optimizer semantics, id spaces no
        plan geometry covers)"""
        P = self.P
        with _PhaseTimer(self, "sort"):
            ku, pu = sort_ids(uid_occ, P["mf_u"].shape[0])
            ki, pi = sort_ids(iid, P["mf_i"].shape[0])
            # the mf / mlp tables of a side share ids: one sort, ONE head list and ONE update pass serve both
            _, hu, nhu = segment_heads(ku, pu, want_single=False)
            _, hi, nhi = segment_heads(ki, pi, want_single=False)
        with _PhaseTimer(self, "table_update"):
            for side, ga, gb, keys, perm, hd, nh in (("b", "g_mf_u", "g_mlp_u", ku, pu, hu, nhu), ("a", "g_mf_i", "g_mlp_i", ki, pi, hi, nhi)):
                ta, tb = self.PAIRS[side]
                sa, sb = self.state[ta], self.state[tb]
                if self.rowwise:
                    segmented_update_pair(keys, perm, rows[ga], rows[gb], hyper=h, W=(P[ta], P[tb]), m=(sa.get("m"), sb.get("m")),
                                          v=(sa.get("v"), sb.get("v")), heads=hd, n_heads=nh)
                else:
                    G = (torch.zeros_like(P[ta]), torch.zeros_like(P[tb]))
                    segmented_update_pair(keys, perm, rows[ga], rows[gb], dense_grad=G, heads=hd, n_heads=nh)
                    dense_update(P[ta], G[0], h, sa.get("m"), sa.get("v"))
                    dense_update(P[tb], G[1], h, sb.get("m"), sb.get("v"))

    @staticmethod
    def _batch_key(uid, iid):
        """identity of a batch's id tensors (storage, shape and torch's in-place version counters): a plan prepared for them is
        used only if the following call brings exactly these tensors, untouched"""
        return (uid.data_ptr(), iid.data_ptr(), tuple(uid.shape), tuple(iid.shape), uid._version, iid._version)

    def _step_fused(self, uid, iid, next_batch=None):
        """The step on rc_neumf_train_step (csrc/neumf_step.hip): ONE kernel for forward, loss, backward and the in-place update
        of single-occurrence item rows, then two pair updates from the bucket plan of the batch (item side: multi-occurrence rows
        only; user side: one gradient row per tuple) on two streams.  The fused kernel leaves no register for a co-resident wave,
        so a plan built beside it would wait for its workgroups to retire: the plan of the NEXT batch is built beside this
        step's table updates instead (next_batch), the batch's own plan only when nobody announced it."""
        B = iid.shape[0]
        dev = iid.device
        out = self._fused_buffers(*iid.shape, dev)
        two_streams = _NEUMF_OVERLAP and iid.numel() >= _SAS_OVERLAP_MIN
        main = torch.cuda.current_stream(dev)
        if two_streams and self._side is None:
            self._side, self._side2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        plan, plan_done, marks_done, buf = self._claim_ahead(uid, iid, main)
        if plan is None and two_streams:
            plan, plan_done = self._plan_on_side(uid, iid, buf, main)
        h, h0 = _step_hypers(self)
        self._fused_kernel(uid, iid, h, buf, out, marks_done, main, two_streams)
        loss_done = None
        if two_streams:
            loss_done = self._side_stream_work(iid, next_batch, buf, marks_done is not None, out, main)
            self._side2.wait_stream(main)
        else:
            with _PhaseTimer(self, "loss"):
                self.loss = reduce_sum(out["loss_vec"], 1.0 / B)
        with _PhaseTimer(self, "sort"):
            if plan is None:
                plan = self._new_plan(uid, iid, buf)
            elif plan_done is not None:
                main.wait_event(plan_done)
        with _PhaseTimer(self, "table_update"):
            self._fused_table_updates(plan, plan_done, out, h, main, two_streams)
        self._dense_step(out, h, h0)
        if loss_done is not None:
            main.wait_event(loss_done)      # (long complete: the caller reads the loss on this stream)
        return self.loss

    def _fused_buffers(self, B, Cn, dev):
        """the flag buffers (once) and the fused kernel's outputs (per batch shape) -> the outputs"""
        P = self.P
        d = P["mf_u"].shape[1]
        if self._marks is None:
            nbytes = max(int(_lib.load().rc_neumf_train_step_marks_bytes(P["mf_i"].shape[0])), 1)
            self._marks = [torch.zeros(nbytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        key = (B, Cn, str(dev))
        if self._fused_out[0] != key:
            e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
            self._fused_out = (key, {"loss_vec": e(B), "g_mf_i": e(B * Cn, d), "g_mlp_i": e(B * Cn, d), "gu_mf": e(B, d), "gu_mlp": e(B, d),
                                     "W1": torch.empty_like(P["W1"]), "b1": torch.empty_like(P["b1"]), "w_out": torch.empty_like(P["w_out"])})
        return self._fused_out[1]

    def _claim_ahead(self, uid, iid, main):
        """-> (plan, plan_done, marks_done, buf) prepared for THIS batch by the previous step, or (None, None, None, 0).
        Which of the two flag buffers / plan workspaces this step uses travels WITH the announcement (not with step_count:
        a non-fused step in between, or a second trainer, must not shift it); with nothing pending both buffers are clean."""
        ahead, self._ahead = self._ahead, None
        if ahead is None:
            return None, None, None, 0
        if ahead["key"] == self._batch_key(uid, iid):
            return ahead["plan"], ahead["plan_done"], ahead["marks_done"], ahead["buf"]
        # a batch was announced and another one came: its prepared flags have to go before that buffer is marked again
        with torch.cuda.stream(self._side):
            neumf_mark_rows(ahead["iid"], self.P["mf_i"].shape[0], self._marks[ahead["buf"]], unmark=True)
        main.wait_stream(self._side)
        return None, None, None, 0    # (the announced id tensors, kept for the side stream's reads, go with `ahead`)

    def _plan_on_side(self, uid, iid, buf, main):
        """this batch's plan, which nobody prepared, on the side stream beside the fused kernel -> (plan, event: plan complete)"""
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side):
            plan = self._new_plan(uid, iid, buf)
            plan.prezero_update_counters()
            plan_done = self._side.record_event()
        iid.record_stream(self._side)
        uid.record_stream(self._side)
        return plan, plan_done

    def _fused_kernel(self, uid, iid, h, buf, out, marks_done, main, two_streams):
        """rc_neumf_train_step on flag buffer `buf`, whose flags the kernel itself or -- marks_done -- the previous step set"""
        with _PhaseTimer(self, "fused_step"):
            if marks_done is not None:      # flags prepared beside the previous step's updates
                main.wait_event(marks_done)
            neumf_train_step(self.P, self.state, uid, iid, h, self._marks[buf], out, marked=marks_done is not None, drop_p=self.dropout,
                             seed=self.seed)
        if marks_done is not None and not two_streams:
            # prepared flags are ALWAYS cleared by the step that consumed them -- also a short step (a ragged last batch of an
            # epoch announced by a large one) that runs on one stream: a flag left behind would make a later single occurrence
            # of that row look like a multiple one, and its update would be dropped
            neumf_mark_rows(iid, self.P["mf_i"].shape[0], self._marks[buf], unmark=True)

    def _side_stream_work(self, iid, next_batch, buf, clear_marks, out, main):
        """on the side stream, beside this step's table updates: the loss, the prepared flags this step consumed cleared
        (clear_marks), the announced batch's flags and plan (kept in self._ahead for the step that brings it) -> event: loss complete"""
        n_i = self.P["mf_i"].shape[0]
        self._side.wait_stream(main)    # behind the fused kernel: beside the updates below
        with torch.cuda.stream(self._side):
            # the batch mean of the per-tuple losses (one workgroup) FIRST on the plan's stream: nothing of this step waits for it
            # (main joins it at the very end), and the streams that carry the two table updates start those at once.  (Round 5
            # had it in front of the user-side update: 28 us on the critical path of the step.)
            self.loss = reduce_sum(out["loss_vec"], 1.0 / iid.shape[0])
            loss_done = self._side.record_event()
            if clear_marks:
                neumf_mark_rows(iid, n_i, self._marks[buf], unmark=True)
                iid.record_stream(self._side)   # the runner drops the batch when step() returns; the allocator must not
                                                # hand its block out while the side stream still reads it
            if next_batch is not None:
                # the following batch's flags and plan; their buffers alternate with this batch's
                nu, ni = next_batch
                neumf_mark_rows(ni, n_i, self._marks[buf ^ 1])
                nmarks_done = self._side.record_event()
                nplan = self._new_plan(nu, ni, buf ^ 1)
                nplan.prezero_update_counters()
                ni.record_stream(self._side)
                nu.record_stream(self._side)
                self._ahead = {"key": self._batch_key(nu, ni), "plan": nplan, "plan_done": self._side.record_event(),
                               "marks_done": nmarks_done, "iid": ni, "buf": buf ^ 1}
        return loss_done

    def _fused_table_updates(self, plan, plan_done, out, h, main, two_streams):
        """item side: the multi-occurrence rows (the fused kernel updated the others); user side: one gradient row per tuple"""
        if two_streams:   # item tables and user tables are disjoint: the two updates run side by side
            if plan_done is not None:
                self._side2.wait_event(plan_done)
            with torch.cuda.stream(self._side2):
                self._update_pair(plan, "b", out["gu_mf"], out["gu_mlp"], h, ws_tag="b")
            self._update_pair(plan, "a", out["g_mf_i"], out["g_mlp_i"], h, ws_tag="a")
            main.wait_stream(self._side2)
        else:
            self._update_pair(plan, "a", out["g_mf_i"], out["g_mlp_i"], h, ws_tag="a")
            self._update_pair(plan, "b", out["gu_mf"], out["gu_mlp"], h, ws_tag="b")


# ---- dense layers (csrc/mlp.hip) -------------------------------------------------------------------------

def linear_fwd(X, W, b=None, relu=False, drop_p=0.0, seed=None, site=0):
    """Y = drop(relu(X W^T + b)) on the fp32 MFMA GEMM (rc_linear_fwd); X [M, K], W [N, K] (nn.Linear.weight), b [N] | None.
    drop_p > 0: training-mode dropout keyed by seed[0] (int64 [1] on the device) and the layer index `site`."""
    f32 = torch.float32
    M, K = X.shape
    N = W.shape[0]
    Y = torch.empty((M, N), dtype=f32, device=X.device)
    ws = workspace(_lib.load().rc_linear_fwd_workspace_bytes(M, N, K), X.device, "linear_fwd")   # split-K planes of a small batch
    _lib.call("rc_linear_fwd", _ptr(X, f32, "X"), _ptr(W, f32, "W"), _ptr(b, f32, "b", True), M, N, K, 1 if relu else 0,
              *_drop_args(drop_p, seed), C.c_uint32(int(site)), _ptr(Y, f32, "Y"), *_ws_args(ws))
    return Y


def linear_bwd(X, W, Y, dY, drop_p=0.0, need_dx=True, need_db=True, x_act=False, x_drop_p=0.0, need_dw=True, ws_tag="linear_bwd"):
    """backward of linear_fwd -> (dX | None, dW, db | None).  Y: the layer's saved output when it went through
    relu (+ dropout) -- it is its own mask -- or None for a plain Linear (or when dY is already masked, see below).
    x_act: X is the drop(relu(.)) output of the layer below (dropout x_drop_p): dX comes out multiplied by that layer's mask
    in the product's epilogue, and the layer below is called with Y=None.
    need_dw=False: only dX (the weight gradient comes from a second call, e.g. on another stream with its own ws_tag)."""
    f32 = torch.float32
    M, K = X.shape
    N = W.shape[0]
    dev = X.device
    dX = torch.empty((M, K), dtype=f32, device=dev) if need_dx else None
    dW = torch.empty((N, K), dtype=f32, device=dev) if need_dw else None
    db = torch.empty(N, dtype=f32, device=dev) if (need_db and need_dw) else None
    ws = workspace(_lib.load().rc_linear_bwd_workspace_bytes(M, N, K), dev, ws_tag)
    _lib.call("rc_linear_bwd", _ptr(X, f32, "X"), _ptr(W, f32, "W"), _ptr(Y, f32, "Y", True), _ptr(dY, f32, "dY"), M, N, K,
              C.c_float(float(drop_p)), 1 if (x_act and need_dx) else 0, C.c_float(float(x_drop_p)), _ptr(dX, f32, "dX", True),
              _ptr(dW, f32, "dW", True), _ptr(db, f32, "db", True), *_ws_args(ws))
    return dX, dW, db


_TOWER_TAIL = os.environ.get("RC_TOWER_TAIL", "1") != "0"      # A/B switch: the tail of a tower as two kernels (csrc/tower_tail.hip)
_TOWER_TAIL_MAX_M = int(os.environ.get("RC_TOWER_TAIL_MAX_M", "8192"))    # larger batches fill the GEMM tiles (B = 16,384: 0.875 ms with the tail kernels, 0.839 without)


def tower_tail_supported(M, K, N2):
    """the last hidden layer [K -> N2] + the output layer [N2 -> 1] of a tower run as rc_tower_tail_fwd / _bwd"""
    return bool(_TOWER_TAIL and 1 <= M <= _TOWER_TAIL_MAX_M and _lib.load().rc_tower_tail_supported(int(M), int(K), int(N2)))


def tower_tail_fwd(X, W2, b2, w3, b3, drop_p=0.0, seed=None, site=0):
    """-> (H2 [M, N2] = drop(relu(X W2^T + b2)), z [M, 1] = H2 w3^T + b3); w3 [1, N2] (nn.Linear(N2, 1).weight), b3 [1] | None;
    dropout mask as linear_fwd with layer index `site`"""
    f32 = torch.float32
    M, K = X.shape
    N2 = W2.shape[0]
    H2 = torch.empty((M, N2), dtype=f32, device=X.device)
    z = torch.empty((M, 1), dtype=f32, device=X.device)
    _lib.call("rc_tower_tail_fwd", _ptr(X, f32, "X"), _ptr(W2, f32, "W2"), _ptr(b2, f32, "b2", True), _ptr(w3, f32, "w3"), _ptr(b3, f32, "b3", True),
              M, K, N2, *_drop_args(drop_p, seed), C.c_uint32(int(site)), _ptr(H2, f32, "H2"), _ptr(z, f32, "z"), _stream())
    return H2, z


def tower_tail_bwd(X, W2, w3, H2, dz, drop_p=0.0, need_dx=True, x_act=False, x_drop_p=0.0, need_db2=True, need_db3=True):
    """backward of tower_tail_fwd given dz [M, 1] -> (dX | None, dW2, db2 | None, dW3 [1, N2], db3 [1] | None); x_act: X is the
    drop(relu(.)) output of the layer below and dX comes out multiplied by its mask (as linear_bwd)"""
    f32 = torch.float32
    M, K = X.shape
    N2 = W2.shape[0]
    dev = X.device
    dX = torch.empty((M, K), dtype=f32, device=dev) if need_dx else None
    dW2 = torch.empty((N2, K), dtype=f32, device=dev)
    db2 = torch.empty(N2, dtype=f32, device=dev) if need_db2 else None
    dW3 = torch.empty((1, N2), dtype=f32, device=dev)
    db3 = torch.empty(1, dtype=f32, device=dev) if need_db3 else None
    ws = workspace(_lib.load().rc_tower_tail_workspace_bytes(M, K, N2), dev, "tower_tail")
    _lib.call("rc_tower_tail_bwd", _ptr(X, f32, "X"), _ptr(W2, f32, "W2"), _ptr(w3, f32, "w3"), _ptr(H2, f32, "H2"), _ptr(dz, f32, "dz"), M, K, N2,
              C.c_float(float(drop_p)), 1 if (x_act and need_dx) else 0, C.c_float(float(x_drop_p)), _ptr(dX, f32, "dX", True),
              _ptr(dW2, f32, "dW2"), _ptr(db2, f32, "db2", True), _ptr(dW3, f32, "dw3"), _ptr(db3, f32, "db3", True),
              *_ws_args(ws))
    return dX, dW2, db2, dW3, db3


# ---- SASRec encoder ---------------------------------------------------------------------------------

SAS_LAYER_KEYS = ("Wq", "bq", "Wk", "bk", "Wv", "bv", "ln1w", "ln1b", "W1", "b1", "W2", "b2", "ln2w", "ln2b")
SAS_NO_DECAY = ("bq", "bk", "bv", "ln1b", "b1", "b2", "ln2b")  # names containing 'bias' (BaseModel.py:64-73)


SASREC_CORE_MAX_HIS = 64   # history_max every encoder path covers; up to 128: one block without dropout (the batch encoder's one-row path)


def sasrec_supported(d, n_layers, n_heads, L, dropout=0.0):
    """the fused encoder covers the shape (rc_sasrec_supported); training-mode dropout needs the all-rows kernels (history <= 64)"""
    if dropout > 0.0 and int(L) > SASREC_CORE_MAX_HIS:
        return False
    return bool(_lib.load().rc_sasrec_supported(int(d), int(n_layers), int(n_heads), int(L)))


def _sas_ptr_table(layers):
    tab = (C.c_void_p * (14 * len(layers)))()
    for l, lay in enumerate(layers):
        for k, name in enumerate(SAS_LAYER_KEYS):
            tab[14 * l + k] = _ptr(lay[name], torch.float32, f"layer{l}.{name}").value
    return tab


class SasSaved:
    """what one forward pass keeps for its backward: layer inputs only (`sequence` kernels, the backward recomputes
    the rest) or every intermediate activation over the compact row space (`batch` kernels)"""

    def __init__(self, impl, data, B, n_layers, L, d):
        self.impl, self.data, self.B, self.n_layers, self.L, self.d = impl, data, B, n_layers, L, d


SASREC_BATCH_MIN_ROWS = 4096  # B * history_max from which the batch-level kernels are used (launch-bound below)


def _sasrec_one_row_encoder(d, n_heads, n_layers, L):
    """the batch encoder's K / V-free last-row path (csrc/sas_last_row.hpp; sb_last_row_mode) serves the WHOLE encoder:
    one block, no dropout, head count 1 / 2 / 4, history_max 3 .. 128"""
    if d is None or int(os.environ.get("RC_SAS_LAST_ROW", "2")) < 2:
        return False
    return (n_layers == 1 and d in (32, 64) and n_heads in (1, 2, 4) and 3 <= L <= 128 and L >= n_heads + 1
            and (d // n_heads) % (d * d // 256) == 0)


def _sasrec_impl(B, L, impl, d=None, n_heads=None, n_layers=None):
    """auto: the batch-level kernels whenever their one-row path is the whole encoder (4 + 7 launches that touch each history
    row once: 0.18 against 0.28 ms per step at B = 256, history_max = 20, and ahead at every size measured, B = 128 .. 4096);
    otherwise the per-sequence kernels (3 launches per pass) while the whole batch is ONE round of resident workgroups in the
    32-row geometry (B <= 512, history_max <= 32), the batch-level kernels (~35 launches, 2-3x the throughput) beyond"""
    impl = impl or os.environ.get("RC_SASREC_IMPL", "auto")
    if impl == "auto":
        if _sasrec_one_row_encoder(d, n_heads, n_layers, L):
            return "batch"
        if B * L < SASREC_BATCH_MIN_ROWS or (B <= 512 and L <= 32):
            return "sequence"
        return "batch"
    if impl not in ("batch", "sequence"):
        raise ValueError("SASRec impl must be auto | batch | sequence, got {!r}".format(impl))
    return impl


def sasrec_fwd(item_emb, pos_emb, layers, n_heads, hist, lengths, save=False, impl=None, drop_p=0.0, seed=None):
    """-> (hv [B,d], SasSaved|None): encoder output at position length-1 (SASRec.py:58-76).
    impl: 'sequence' (csrc/sasrec.hip, one workgroup per sequence), 'batch' (csrc/sasrec_batch.hip, row-space
    kernels), default by batch size.  drop_p > 0: training-mode dropout of both residual branches of every layer
    (utils/layers.py:104-117), mask from the counter-based stream keyed by seed[0] (int64 [1] on the device); only
    the batch-level kernels carry it (rc_sasrec_batch_fwd), so dropout selects them."""
    B, L = hist.shape
    d = item_emb.shape[1]
    dev, f32 = hist.device, torch.float32
    hv = torch.empty((B, d), dtype=f32, device=dev)
    lib = _lib.load()
    if drop_p > 0.0:
        if impl == "sequence":
            raise ValueError("SASRec dropout is implemented by the batch-level kernels only (impl='batch')")
        impl = "batch"
    impl = _sasrec_impl(B, L, impl, *((d, int(n_heads), len(layers)) if drop_p == 0.0 else ()))
    if impl == "batch":
        # eval passes reuse one scratch state; training passes own theirs until the backward has run
        n_state = lib.rc_sasrec_batch_state_floats(B, L, d, len(layers))
        state = (torch.empty(n_state, dtype=f32, device=dev) if save
                 else workspace(4 * n_state, dev, "sasrec_state").view(f32)[:n_state])
        ws = workspace(lib.rc_sasrec_batch_workspace_bytes(B, L, d, len(layers)), dev, "sasrec_batch")
        _lib.call("rc_sasrec_batch_fwd", _ptr(item_emb, f32, "item_emb"), _ptr(pos_emb, f32, "pos_emb"),
                  _sas_ptr_table(layers), len(layers), int(n_heads), _ptr(hist, torch.int64, "hist"),
                  _ptr(lengths, torch.int64, "lengths"), B, L, d, *_drop_args(drop_p, seed), _ptr(hv, f32, "hv"),
                  _ptr(state, f32, "state"), *_ws_args(ws))
        return hv, (SasSaved("batch", state, B, len(layers), L, d) if save else None)
    xsave = torch.empty((B, len(layers), L, d), dtype=f32, device=dev) if save else None
    ws = workspace(lib.rc_sasrec_workspace_bytes(B, d, len(layers)), dev, "sasrec")
    _lib.call("rc_sasrec_fwd", _ptr(item_emb, f32, "item_emb"), _ptr(pos_emb, f32, "pos_emb"),
              _sas_ptr_table(layers), len(layers), int(n_heads), _ptr(hist, torch.int64, "hist"),
              _ptr(lengths, torch.int64, "lengths"), B, L, d, _ptr(hv, f32, "hv"),
              _ptr(xsave, f32, "xsave", True), *_ws_args(ws))
    return hv, (SasSaved("sequence", xsave, B, len(layers), L, d) if save else None)


def _sas_dense_views(dense, n_layers, d):
    grads = []
    for l in range(n_layers):
        off, g = 0, {}
        for name in SAS_LAYER_KEYS:
            n = d * d if name.startswith("W") else d
            g[name] = dense[l, off:off + n].view(d, d) if name.startswith("W") else dense[l, off:off + n]
            off += n
        grads.append(g)
    return grads


def sasrec_bwd(layers, n_heads, lengths, saved, dhv, drop_p=0.0, seed=None, split=False):
    """-> (g_hist [B,L,d], list of per-layer dicts of dense gradients); `saved` from sasrec_fwd(save=True);
    drop_p / seed as given to the forward this is the backward of (the mask is regenerated, not stored).
    split=True (batch-level kernels): only the launches up to the one that completes g_hist are enqueued (rc_sasrec_batch_bwd_part,
    part 1) -> (g_hist, grads, finish): the caller forks whatever waits for g_hist alone, then calls finish() on the same stream
    for the rest (the dense gradient views are complete after it)"""
    B, n_layers, L, d = saved.B, saved.n_layers, saved.L, saved.d
    dev, f32 = dhv.device, torch.float32
    g_hist = torch.empty((B, L, d), dtype=f32, device=dev)
    lib = _lib.load()
    pl = lib.rc_sasrec_dense_param_count(d)
    dense = torch.empty((n_layers, pl), dtype=f32, device=dev)
    if saved.impl == "batch":
        ws = workspace(lib.rc_sasrec_batch_workspace_bytes(B, L, d, n_layers), dev, "sasrec_batch")
        if split:
            args = (_sas_ptr_table(layers), n_layers, int(n_heads), _ptr(lengths, torch.int64, "lengths"), B, L, d, *_drop_args(drop_p, seed),
                    _ptr(saved.data, f32, "state"), _ptr(dhv, f32, "dhv"), _ptr(g_hist, f32, "g_hist"), _ptr(dense, f32, "dense"),
                    C.c_void_p(ws.data_ptr()), ws.numel())
            _lib.call("rc_sasrec_batch_bwd_part", *args, 1, _stream())
            keep = (layers, lengths, saved, dhv, g_hist, dense, ws)      # alive until part 2 is enqueued
            return g_hist, _sas_dense_views(dense, n_layers, d), (lambda: (_lib.call("rc_sasrec_batch_bwd_part", *args, 2, _stream()), keep)[0])
        _lib.call("rc_sasrec_batch_bwd", _sas_ptr_table(layers), n_layers, int(n_heads),
                  _ptr(lengths, torch.int64, "lengths"), B, L, d, *_drop_args(drop_p, seed), _ptr(saved.data, f32, "state"),
                  _ptr(dhv, f32, "dhv"), _ptr(g_hist, f32, "g_hist"), _ptr(dense, f32, "dense"), C.c_void_p(ws.data_ptr()),
                  ws.numel(), _stream())
    else:
        if drop_p > 0.0:
            raise ValueError("SASRec dropout needs the batch-level kernels")
        ws = workspace(lib.rc_sasrec_workspace_bytes(B, d, n_layers), dev, "sasrec")
        _lib.call("rc_sasrec_bwd", _sas_ptr_table(layers), n_layers, int(n_heads), _ptr(lengths, torch.int64, "lengths"),
                  B, L, d, _ptr(saved.data, f32, "xsave"), _ptr(dhv, f32, "dhv"), _ptr(g_hist, f32, "g_hist"),
                  _ptr(dense, f32, "dense"), *_ws_args(ws))
    if split:
        return g_hist, _sas_dense_views(dense, n_layers, d), (lambda: None)
    return g_hist, _sas_dense_views(dense, n_layers, d)


def sasrec_pos_grad(g_hist, lengths, n_pos):
    """dense gradient [n_pos, d] of the position table from the history-row gradients g_hist [B, L, d]
    (position id = length - index, SASRec.py:64)"""
    B, L, d = g_hist.shape
    out = torch.empty((n_pos, d), dtype=torch.float32, device=g_hist.device)
    ws = workspace(_lib.load().rc_sasrec_pos_grad_workspace_bytes(B, L, d), g_hist.device, "sasrec_pos")
    _lib.call("rc_sasrec_pos_grad", _ptr(g_hist, torch.float32, "g_hist"), _ptr(lengths, torch.int64, "lengths"), B, L, d,
              int(n_pos), _ptr(out, torch.float32, "grad_pos"), *_ws_args(ws))
    return out


# ---- shape-generic sequence-encoder layers (csrc/seq_layers.hip) ------------------------------------------------------

def seq_offsets(lengths, L):
    """off int32 [B + 1]: exclusive prefix sums of min(len_b, L) -- valid row counts and compact row indices of the padded batch"""
    B = lengths.numel()
    off = torch.empty(B + 1, dtype=torch.int32, device=lengths.device)
    _lib.call("rc_seq_offsets", _ptr(lengths, torch.int64, "lengths"), B, int(L), _ptr(off, torch.int32, "off"), _stream())
    return off


def seq_embed(item_emb, pos_emb, hist, lengths):
    """X [B * L, d] = item rows + position rows (position id = length - index) on valid rows, 0 on the padding (SASRec.py:58-66)"""
    B, L = hist.shape
    d = item_emb.shape[1]
    f32, i64 = torch.float32, torch.int64
    X = torch.empty((B * L, d), dtype=f32, device=hist.device)
    _lib.call("rc_seq_embed_fwd", _ptr(item_emb, f32, "item_emb"), _ptr(pos_emb, f32, "pos_emb"), _ptr(hist, i64, "hist"),
              _ptr(lengths, i64, "lengths"), B, L, d, _ptr(X, f32, "X"), _stream())
    return X


def seq_pick_last(X, lengths, B, L):
    """hv [B, d] = X[b * L + len_b - 1] (SASRec.py:76)"""
    d = X.shape[1]
    hv = torch.empty((B, d), dtype=torch.float32, device=X.device)
    _lib.call("rc_seq_pick_last_fwd", _ptr(X, torch.float32, "X"), _ptr(lengths, torch.int64, "lengths"), B, int(L), d, _ptr(hv, torch.float32, "hv"), _stream())
    return hv


def seq_pick_last_bwd(dhv, lengths, B, L):
    d = dhv.shape[1]
    dX = torch.empty((B * L, d), dtype=torch.float32, device=dhv.device)
    _lib.call("rc_seq_pick_last_bwd", _ptr(dhv, torch.float32, "dhv"), _ptr(lengths, torch.int64, "lengths"), B, int(L), d, _ptr(dX, torch.float32, "dX"), _stream())
    return dX


def seq_pos_grad(dX, lengths, B, L, n_pos):
    """dense gradient [n_pos, d] of the position table from the rows' gradients dX [B * L, d] (position id = length - index)"""
    d = dX.shape[1]
    out = torch.empty((n_pos, d), dtype=torch.float32, device=dX.device)
    _lib.call("rc_seq_pos_grad", _ptr(dX, torch.float32, "dX"), _ptr(lengths, torch.int64, "lengths"), B, int(L), d, int(n_pos),
              _ptr(out, torch.float32, "grad_pos"), _stream())
    return out


def seq_attention_supported(L, dk):
    return bool(_lib.load().rc_seq_attention_supported(int(L), int(dk)))


def _seq_attn_head(Q, K, V, off, mask, causal, B, L, H):
    f32 = torch.float32
    dk = Q.shape[1] // H
    mb = 0
    if mask is not None:
        if mask.dtype != torch.uint8 or mask.shape[-2:] != (L, L) or mask.numel() not in (L * L, B * L * L):
            raise ValueError("seq_attention: mask must be uint8 [L, L] or [B, L, L]")
        mb = 1 if mask.numel() == B * L * L and B > 1 else 0
    return (_ptr(Q, f32, "Q"), _ptr(K, f32, "K"), _ptr(V, f32, "V"), _ptr(off, torch.int32, "off", True), _ptr(mask, torch.uint8, "mask", True),
            mb, 1 if causal else 0, B, L, H, dk)


def seq_attention_fwd(Q, K, V, off, B, L, H, mask=None, causal=True):
    """Q, K, V [B * L, H * dk] -> (ctx [B * L, H * dk], lse [B, H, L])  (utils/layers.py:52-63, per head)"""
    f32 = torch.float32
    ctx = torch.empty_like(Q)
    lse = torch.empty((B, H, L), dtype=f32, device=Q.device)
    _lib.call("rc_seq_attention_fwd", *_seq_attn_head(Q, K, V, off, mask, causal, B, L, H), _ptr(ctx, f32, "ctx"), _ptr(lse, f32, "lse"), _stream())
    return ctx, lse


def seq_attention_bwd(Q, K, V, off, B, L, H, lse, dctx, mask=None, causal=True):
    """-> (dQ, dK, dV); probabilities recomputed from lse"""
    f32 = torch.float32
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(Q), torch.empty_like(Q)
    Dv = torch.empty((B, H, L), dtype=f32, device=Q.device)
    _lib.call("rc_seq_attention_bwd", *_seq_attn_head(Q, K, V, off, mask, causal, B, L, H), _ptr(lse, f32, "lse"), _ptr(dctx, f32, "dctx"),
              _ptr(Dv, f32, "Dv"), _ptr(dQ, f32, "dQ"), _ptr(dK, f32, "dK"), _ptr(dV, f32, "dV"), _stream())
    return dQ, dK, dV


def seq_add_layernorm_fwd(A, R, w, b, off, L, drop_p=0.0, seed=None, site=0):
    """Y = LayerNorm(dropout(A) + R) over the rows of A [rows, d] -> (Y, xhat, rstd)  (utils/layers.py:110,117)"""
    f32 = torch.float32
    rows, d = A.shape
    Y, xhat = torch.empty_like(A), torch.empty_like(A)
    rstd = torch.empty(rows, dtype=f32, device=A.device)
    _lib.call("rc_seq_add_layernorm_fwd", _ptr(A, f32, "A"), _ptr(R, f32, "R", True), _ptr(w, f32, "w"), _ptr(b, f32, "b"),
              _ptr(off, torch.int32, "off", True), rows, int(L), d, *_drop_args(drop_p, seed), C.c_uint32(int(site)), _ptr(Y, f32, "Y"),
              _ptr(xhat, f32, "xhat"), _ptr(rstd, f32, "rstd"), _stream())
    return Y, xhat, rstd


def seq_add_layernorm_bwd(dY, xhat, rstd, w, off, L, drop_p=0.0, seed=None, site=0, need_dA=True, need_dR=True):
    """-> (dA | None, dR | None, dw [d], db [d])"""
    f32 = torch.float32
    rows, d = dY.shape
    dA = torch.empty_like(dY) if need_dA else None
    dR = torch.empty_like(dY) if need_dR else None
    dw, db = torch.empty(d, dtype=f32, device=dY.device), torch.empty(d, dtype=f32, device=dY.device)
    ws = workspace(_lib.load().rc_seq_add_layernorm_bwd_workspace_bytes(d), dY.device, "seq_ln_bwd")
    _lib.call("rc_seq_add_layernorm_bwd", _ptr(dY, f32, "dY"), _ptr(xhat, f32, "xhat"), _ptr(rstd, f32, "rstd"), _ptr(w, f32, "w"),
              _ptr(off, torch.int32, "off", True), rows, int(L), d, *_drop_args(drop_p, seed), C.c_uint32(int(site)), _ptr(dA, f32, "dA", True),
              _ptr(dR, f32, "dR", True), _ptr(dw, f32, "dw"), _ptr(db, f32, "db"), *_ws_args(ws))
    return dA, dR, dw, db


def seg_rows_route(n_occ, n_rows, d):
    """True iff segmented_update2 takes rc_segmented_update_rows (one wave per table row: every row collects many occurrences).
    That route ignores keys >= n_rows, which lets a caller park occurrences that must not take part (padding) behind the table."""
    return _SEG_ROWS and d in (16, 32, 64, 128, 256) and n_occ >= _SEG_ROWS_MIN_PER_ROW * n_rows


def segmented_update2(keys, perm, src, src2, n_split, hyper=None, W=None, m=None, v=None, coef=None,
                      src_index=None, div=1, dense_grad=None, step_dev=None):
    """rc_segmented_update with a second source: occurrences >= n_split take plain rows src2[o - n_split].
    step_dev: int64 device tensor [1] with Adam's step count (hipGraph-capturable; one-wave-per-row route only)"""
    n_occ = keys.numel()
    d = src.shape[-1]
    f32 = torch.float32
    table = W if W is not None else dense_grad
    n_rows = table.shape[0]
    if seg_rows_route(n_occ, n_rows, d):
        # every row collects many occurrences (a small catalogue under a large batch): one wave per table row
        ws = workspace(_lib.load().rc_segmented_rows_workspace_bytes(n_rows, n_occ, d), keys.device, "seg_rows")
        _lib.call("rc_segmented_update_rows", *_table_args(W, m, v), d, n_rows, _ptr(keys, torch.int32, "keys"),
                  _ptr(perm, torch.int32, "perm"), n_occ, *_source_args(coef, src, src_index, div, src2, n_split, need_src2=True),
                  _hyper_ref(hyper), _ptr(step_dev, torch.int64, "step_dev", True), _ptr(dense_grad, f32, "dense_grad", True),
                  *_ws_args(ws))
        return
    if step_dev is not None:
        raise RuntimeError("segmented_update2(step_dev=...): the device-side step count is carried by the one-wave-per-row "
                           "update only (seg_rows_route: a small catalogue under a large batch)")
    segmented_update(keys, perm, src, hyper, W, m, v, coef, src_index, div, dense_grad, src2=src2, n_split=n_split)


def rows_plan_supported(n_rows, n_occ, d):
    return bool(_lib.load().rc_rows_plan_supported(int(n_rows), int(n_occ), int(d)))


_rows_plan_zeroed = set()


class RowsPlan:
    """rc_rows_plan_build: the occurrences of a small table's rows grouped by row, straight from the batch's id tensors
    (ids_a [.., C] then ids_b [B, L]; lengths_b marks the padding slots of ids_b, which take no part) -- three launches, no sort;
    update(): rc_rows_plan_update, the one-wave-per-row reduction of segmented_update2 on that grouping (bit-identical to it)."""

    def __init__(self, ids_a, ids_b, lengths_b, n_rows, d, tag="rows_plan"):
        self.n_a, self.n_b = ids_a.numel(), (ids_b.numel() if ids_b is not None else 0)
        self.n_occ, self.n_rows, self.d = self.n_a + self.n_b, int(n_rows), int(d)
        dev = ids_a.device
        lib = _lib.load()
        self.ws = workspace(lib.rc_rows_plan_workspace_bytes(self.n_rows, self.n_occ, self.d), dev, tag)
        if self.ws.data_ptr() not in _rows_plan_zeroed:   # status counter; everything else is written before it is read
            self.ws.zero_()
            _rows_plan_zeroed.add(self.ws.data_ptr())
        L = ids_b.shape[-1] if (ids_b is not None and lengths_b is not None) else 1
        _lib.call("rc_rows_plan_build", _ptr(ids_a, torch.int64, "ids_a"), self.n_a, _ptr(ids_b, torch.int64, "ids_b", True), self.n_b,
                  _ptr(lengths_b, torch.int64, "lengths_b", True), int(L), self.n_rows, self.d, *_ws_args(self.ws))

    def update(self, src, hyper=None, W=None, m=None, v=None, coef=None, src_index=None, div=1, src2=None, dense_grad=None,
               step_dev=None):
        # (occurrences from n_a on -- the second id tensor's -- take src2; the plan's own workspace, not a cached one)
        _lib.call("rc_rows_plan_update", *_table_args(W, m, v), self.d, self.n_rows, self.n_occ,
                  *_source_args(coef, src, src_index, div, src2, self.n_a), _hyper_ref(hyper),
                  _ptr(step_dev, torch.int64, "step_dev", True), _ptr(dense_grad, torch.float32, "dense_grad", True), *_ws_args(self.ws))

    def views(self):
        """(keys, perm, start, end, status) as int32 tensors copied out of the workspace (tests)"""
        ptrs = [C.c_void_p() for _ in range(5)]
        _lib.call("rc_rows_plan_views", C.c_void_p(self.ws.data_ptr()), self.n_rows, self.n_occ, self.d, *[C.byref(p) for p in ptrs])
        base = self.ws.data_ptr()
        words = self.ws.view(torch.int32)
        sizes = [self.n_occ + 1, self.n_occ + 1, self.n_rows, self.n_rows, 1]
        return tuple(words[(p.value - base) // 4:(p.value - base) // 4 + n].clone() for p, n in zip(ptrs, sizes))


class _SortedRows(collections.namedtuple("_SortedRows", "keys perm n_split")):
    """RowsPlan.update's call shape on the sorted route: (keys, perm) of sort_ids over candidate + history ids, and n_split, the
    occurrence the history rows (src2) begin at"""

    def update(self, src, src2=None, **kw):
        segmented_update2(self.keys, self.perm, src, src2, self.n_split, **kw)


class SasrecTrainer:
    """One BaseRunner.fit iteration for SASRec on device tensors.
    P = {"item_emb": [n_items,d], "pos_emb": [max_his+1,d], "layers": [dict(SAS_LAYER_KEYS) ...]}.
    dropout > 0: both residual branches of every layer dropped with a fresh mask per step (device seed counter,
    bumped every step; batch-level kernels)."""

    GRAPH_WARMUP = 2   # eager steps per batch shape before the capture: workspaces and optimizer state exist by then

    def __init__(self, P, n_heads, opt="Adam", lr=1e-3, l2=0.0, rowwise=False, dropout=0.0, seed=0, graph=False):
        """graph=True: from the third step of a batch shape on, the step (about 45 launches on two streams, no host
        synchronisation, grids that depend on shapes only) is replayed from a hipGraph with the batch copied into static
        buffers -- at config 3 the eager step is bound by the host's launch rate (0.42 ms enqueue against 0.27 ms of GPU work).
        Same kernels, same results.  With Adam the step count is kept in device memory (capturable semantics: bias corrections
        formed in the kernels) and the item table must take the one-wave-per-row update (seg_rows_route), rowwise=True.
        The loss tensor a replayed step returns is the graph's own buffer: the next replay overwrites it (clone it to keep it)."""
        self.P, self.n_heads, self.opt, self.lr, self.l2, self.rowwise = P, n_heads, opt, lr, l2, rowwise
        self.dropout = float(dropout)
        self.seed = torch.tensor([seed], dtype=torch.int64, device=P["item_emb"].device) if self.dropout > 0 else None
        self.step_count = 0
        self.loss = None
        self.state = {}
        self._side = None
        self.graph = bool(graph)
        # Adam under replay: the step count lives in device memory (torch.optim.Adam(capturable=True) semantics); carried by the
        # row-wise one-wave-per-row item update and the multi-tensor dense step
        self._step_dev = None
        if self.graph and opt == "Adam":
            if not rowwise:
                raise ValueError("SasrecTrainer(graph=True, opt='Adam') needs rowwise=True (the dense item-table step takes the "
                                 "step count as a kernel argument)")
            self._step_dev = torch.zeros(1, dtype=torch.int64, device=P["item_emb"].device)
        self._graphs, self._graph_seen = {}, {}
        self.timing = None      # {} switches the per-phase events on (_PhaseTimer, phases_ms); a timed step is not replayed
        self._rows_by = {}      # (B, device) -> arange(B): the "user" row of every candidate tuple in _score_loss

    def _st(self, t):
        st = self.state.get(t.data_ptr())
        if st is None:
            st = self.state[t.data_ptr()] = new_opt_state(t, self.opt)
        return st

    def _side_stream(self, dev):
        """the trainer's second stream: the id sort (needs only the batch) runs beside the encoder, the position-table
        gradient beside the item-table update -- all of them latency-bound launches that leave most of the chip idle"""
        if self._side is None:
            self._side = torch.cuda.Stream(device=dev)
        return self._side

    def _dev_step_route(self, hist, iid):
        """Adam with the step count in device memory: carried by the one-wave-per-row item update (seg_rows_route) only"""
        if self._step_dev is None:
            return False
        I = self.P["item_emb"]
        return seg_rows_route(iid.numel() + hist.numel(), I.shape[0], I.shape[1])

    def step(self, hist, lengths, iid):
        if not (self.graph and hist.is_cuda) or self.timing is not None \
                or (self._step_dev is not None and not self._dev_step_route(hist, iid)):
            return self._step(hist, lengths, iid)
        from . import graph as hgraph
        if not hgraph.usable():
            raise RuntimeError("SasrecTrainer(graph=True): hipGraph replay needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 before HIP "
                               "initialises (rechorus_amd/graph.py); import rechorus_amd before touching the GPU")
        # lr / l2 / the optimizer are kernel arguments frozen into a captured step: they are part of the key
        key = (tuple(hist.shape), tuple(iid.shape), self.opt, float(self.lr), float(self.l2))
        entry = self._graphs.get(key)
        if entry is None:
            seen = self._graph_seen.get(key, 0)
            if seen < self.GRAPH_WARMUP:
                self._graph_seen[key] = seen + 1
                return self._step(hist, lengths, iid)
            # one flat id buffer, the three inputs are views into it: the per-step copy is one launch
            flat = torch.cat([hist.reshape(-1), lengths.reshape(-1), iid.reshape(-1)])
            n0, n1 = hist.numel(), hist.numel() + lengths.numel()
            static = (flat[:n0].view(hist.shape), flat[n0:n1].view(lengths.shape), flat[n1:].view(iid.shape), flat)
            torch.cuda.synchronize(hist.device)
            g = torch.cuda.CUDAGraph()
            cap = torch.cuda.Stream(device=hist.device)
            with torch.cuda.stream(cap):
                with torch.cuda.graph(g, stream=cap):
                    self._step(*static[:3])
            self.step_count -= 1   # the capture recorded a step, it did not train one (its device-side increments are graph nodes)
            entry = self._graphs[key] = (g, static, self.loss)
            torch.cuda.synchronize(hist.device)
            # (the capture recorded the step without running it: this batch is trained by the replay below)
        g, static, loss = entry
        _lib.call("rc_stage_batch", _ptr(hist, torch.int64, "hist"), hist.numel(), _ptr(lengths, torch.int64, "lengths"), lengths.numel(),
                  _ptr(iid, torch.int64, "iid"), iid.numel(), _ptr(static[3], torch.int64, "static"), _stream())
        g.replay()
        # the host's count follows every trained step -- replayed or eager -- so that a batch shape that leaves the captured route
        # (the short last batch of an epoch) steps Adam with the right bias corrections
        self.step_count += 1
        self.loss = loss
        return loss

    def _sorted_occurrences(self, hist, lengths, iid):
        """candidate + history ids, sorted.  On the one-wave-per-row route the padding slots of the history windows (id 0, zero
        gradient rows: half of B * history_max occurrences of ONE row, a 400-chunk hot row) are parked behind the table (key =
        n_items, ignored there) except the first of them, which keeps row 0 among the touched rows exactly as before -- a sum of
        zero rows is zero either way."""
        I = self.P["item_emb"]
        n_items, d = I.shape
        L = hist.shape[1]
        n_occ = iid.numel() + hist.numel()
        if not seg_rows_route(n_occ, n_items, d):
            return sort_ids(torch.cat([iid.reshape(-1), hist.reshape(-1)]), n_items)
        pad = (torch.arange(L, device=hist.device)[None, :] >= lengths[:, None]).reshape(-1)
        hid = torch.where(pad, hist.new_full((), n_items), hist.reshape(-1))
        first_pad = pad.to(torch.int32).argmax().reshape(1)   # position of the first padding slot (0 if there is none)
        hid.scatter_(0, first_pad, hist.reshape(-1).gather(0, first_pad))   # (tensor-indexed assignment would read the index back: a host sync)
        return sort_ids(torch.cat([iid.reshape(-1), hid]), n_items + 1)

    def _group_ids(self, hist, lengths, iid, rows_plan):
        """the batch's candidate + history occurrences grouped by item row -> an object whose update(src, ...) runs the item
        table's step on that grouping: a RowsPlan (counting sort of the id tensors) or the sorted ids behind its call shape"""
        I = self.P["item_emb"]
        if rows_plan:
            return RowsPlan(iid, hist, lengths, I.shape[0], I.shape[1], tag="sasrec_rows")
        return _SortedRows(*self._sorted_occurrences(hist, lengths, iid), n_split=iid.numel())

    def _item_table_update(self, group, hv, gpred, g_hist, h, step_dev, Cn):
        """candidate occurrences (g * hv, rebuilt on the fly) + history occurrences (g_hist rows) of the item table, grouped by
        `group` (_group_ids): row-wise optimizer step, or dense gradient + dense step"""
        I = self.P["item_emb"]
        st = self._st(I)
        src = dict(coef=gpred.reshape(-1), div=Cn, src2=g_hist.view(-1, I.shape[1]))
        if self.rowwise:
            group.update(hv, hyper=h, W=I, m=st.get("m"), v=st.get("v"), step_dev=step_dev, **src)
        else:
            G = torch.zeros_like(I)
            group.update(hv, dense_grad=G, **src)
            dense_update(I, G, h, st.get("m"), st.get("v"))

    def _dense_step(self, g_hist, lengths, dgrads, h, h0, step_dev):
        """the position table's gradient, then position table + every block parameter in one launch"""
        P = self.P
        Pe, layers = P["pos_emb"], P["layers"]
        Gp = sasrec_pos_grad(g_hist, lengths, Pe.shape[0])
        st = self._st(Pe)
        items = [(Pe, Gp, h, st.get("m"), st.get("v"))]
        for lay, g in zip(layers, dgrads):
            for name in SAS_LAYER_KEYS:
                st = self._st(lay[name])
                items.append((lay[name], g[name].contiguous(), h0 if name in SAS_NO_DECAY else h, st.get("m"), st.get("v")))
        dense_update_multi(items, self.opt, step_dev=step_dev, increment=False)

    def _encode(self, hist, lengths):
        P = self.P
        return sasrec_fwd(P["item_emb"], P["pos_emb"], P["layers"], self.n_heads, hist, lengths, save=True, drop_p=self.dropout, seed=self.seed)

    def _score_loss(self, hv, iid):
        # scores, BPR loss, d loss / d pred and d loss / d hv in ONE pass over the candidate rows: the fused BPRMF kernel
        # with the encoder output as the "user" row (SASRec.py:80-81, BaseModel.py:182-185); three launches and two
        # more passes over the [B, C] rows before
        # (one tensor per batch size, kept for the trainer's life: a captured step holds its ADDRESS -- replacing it when another
        #  batch size comes by, e.g. the short last batch of an epoch, would leave the graph of the first size reading freed memory)
        key_rows = (hv.shape[0], str(hv.device))
        if key_rows not in self._rows_by:
            self._rows_by[key_rows] = torch.arange(hv.shape[0], device=hv.device)
        _, loss_vec, gpred, dhv = bprmf_fwd_bwd(hv, self.P["item_emb"], self._rows_by[key_rows], iid, want_pred=False)
        return loss_vec, gpred, dhv

    def _step(self, hist, lengths, iid):
        I = self.P["item_emb"]
        self.step_count += 1
        h, h0 = _step_hypers(self)
        if self.seed is not None:
            step_increment(self.seed)
        if self._step_dev is not None:
            step_increment(self._step_dev)
        n_occ = iid.numel() + hist.numel()
        # Adam under replay: the kernels read the step count from device memory where the route carries it (else this step takes
        # the host's count -- both advance every step -- and is not captured)
        step_dev = self._step_dev if self._dev_step_route(hist, iid) else None
        # one wave per table row with the rows' bounds from a counting sort of the id tensors themselves (no radix sort, no glue)
        rows_plan = (_SAS_ROWS_PLAN and hist.is_cuda and seg_rows_route(n_occ, I.shape[0], I.shape[1])
                     and rows_plan_supported(I.shape[0], n_occ, I.shape[1]))
        # (small batches are bound by the host's launch rate: the extra stream switches cost more than the overlap returns --
        #  B = 256: 0.39 against 0.30 ms; B = 4096: 0.66 against 0.72 ms)
        if hist.is_cuda and n_occ >= _SAS_OVERLAP_MIN:
            return self._step_item_stream(hist, lengths, iid, h, h0, step_dev, rows_plan)
        return self._step_one_stream(hist, lengths, iid, h, h0, step_dev, rows_plan)

    def _step_one_stream(self, hist, lengths, iid, h, h0, step_dev, rows_plan):
        B, Cn = iid.shape
        with _PhaseTimer(self, "encoder_fwd"):
            hv, xsave = self._encode(hist, lengths)
        with _PhaseTimer(self, "score_loss"):
            loss_vec, gpred, dhv = self._score_loss(hv, iid)
            self.loss = reduce_sum(loss_vec, 1.0 / B)
        with _PhaseTimer(self, "encoder_bwd"):
            g_hist, dgrads = sasrec_bwd(self.P["layers"], self.n_heads, lengths, xsave, dhv, drop_p=self.dropout, seed=self.seed)
        with _PhaseTimer(self, "table_update"):
            self._item_table_update(self._group_ids(hist, lengths, iid, rows_plan), hv, gpred, g_hist, h, step_dev, Cn)
        with _PhaseTimer(self, "dense_update"):   # position table (tiny) and the block parameters: dense gradient, dense step
            self._dense_step(g_hist, lengths, dgrads, h, h0, step_dev)
        return self.loss

    def _step_item_stream(self, hist, lengths, iid, h, h0, step_dev, rows_plan):
        """The step on two streams, one of which owns everything about the ITEM TABLE: the grouping of the batch's ids beside the
        encoder, then -- as soon as the history rows' gradient is complete (rc_sasrec_batch_bwd_part) -- the table update, while the
        other stream finishes the encoder's parameter gradients, the position gradient and the dense step.  One fork, one
        hand-over (g_hist ready), one join.  (Round 5: the table update ran on the encoder's stream behind a second join, the
        position gradient on the side: two more cross-queue edges of ~11 us each on the critical path of a replayed step.)
        The encoder rides the caller's stream (in a captured step: the launch stream, the other branch starts behind a cross-queue
        barrier), the item-table work the side stream.  The other way round -- the table update's kernels last on the launch stream,
        where the graph ends without waiting for another queue -- measured 0.225 against 0.219 ms per replayed step at config 3
        (profiles/r09_sasrec_two_stream_schedules.txt)."""
        B, Cn = iid.shape
        enc = torch.cuda.current_stream(hist.device)
        tab = self._side_stream(hist.device)
        # the batch is ready; last step's users of the side stream's buffers are done (the step ends with a join)
        tab.wait_event(enc.record_event())
        with _PhaseTimer(self, "encoder_fwd"):
            hv, xsave = self._encode(hist, lengths)
        with torch.cuda.stream(tab):
            group = self._group_ids(hist, lengths, iid, rows_plan)
        with _PhaseTimer(self, "score_loss"):
            loss_vec, gpred, dhv = self._score_loss(hv, iid)
        with _PhaseTimer(self, "encoder_bwd"):
            g_hist, dgrads, finish_bwd = sasrec_bwd(self.P["layers"], self.n_heads, lengths, xsave, dhv, drop_p=self.dropout,
                                                    seed=self.seed, split=True)
        ready = enc.record_event()     # g_hist, gpred, hv: what the table update reads
        with _PhaseTimer(self, "dense_update"):
            finish_bwd()               # the encoder's parameter gradients ...
            self._dense_step(g_hist, lengths, dgrads, h, h0, step_dev)     # ... the position table's, and the dense step of both
        # the batch mean of the losses last on this stream: it ends ~20 us before the item-table stream does, and 5 us in front of
        # the table update were 5 us of the step
        self.loss = reduce_sum(loss_vec, 1.0 / B)
        with torch.cuda.stream(tab):
            tab.wait_event(ready)
            with _PhaseTimer(self, "table_update"):
                self._item_table_update(group, hv, gpred, g_hist, h, step_dev, Cn)
        enc.wait_stream(tab)             # the step's one join
        return self.loss


# ---- list-wise softmax cross-entropy -------------------------------------------------------------------

def softmax_ce(pred, target, max_pos, need_grad=True):
    """ImpressionModel.loss with loss_n='softmaxCE' (models/BaseImpressionModel.py:96-107).
    pred [B,n] fp32, target [B,n] int64 in {1,0,-1}; -> (loss [1], gpred | None)"""
    B, n = pred.shape
    dev, f32 = pred.device, torch.float32
    loss_vec = torch.empty(B, dtype=f32, device=dev)
    h_sum = torch.empty(1, dtype=f32, device=dev)
    gpred = torch.empty_like(pred) if need_grad else None
    _lib.call("rc_softmax_ce_fwd_bwd", _ptr(pred, f32, "pred"), _ptr(target, torch.int64, "target"), B, n, int(max_pos),
              _ptr(loss_vec, f32, "loss_vec"), _ptr(h_sum, f32, "h_sum"), _ptr(gpred, f32, "gpred", True), _stream())
    return reduce_sum(loss_vec, 1.0), gpred


def list_bpr(pred, target, max_pos, hard=False, need_grad=True):
    """ImpressionModel.loss with loss_n 'BPR' / 'BPRhard' (models/BaseImpressionModel.py:50-89)
    -> (loss [1], gpred | None)"""
    B, n = pred.shape
    f32 = torch.float32
    loss_vec = torch.empty(B, dtype=f32, device=pred.device)
    gpred = torch.empty_like(pred) if need_grad else None
    _lib.call("rc_list_bpr_fwd_bwd", _ptr(pred, f32, "pred"), _ptr(target, torch.int64, "target"), B, n, int(max_pos),
              1 if hard else 0, 1.0 / B, _ptr(loss_vec, f32, "loss_vec"), _ptr(gpred, f32, "gpred", True), _stream())
    return reduce_sum(loss_vec, 1.0 / B), gpred


LIST_KINDS = {"BPR": 0, "BPRhard": 1, "BPRafter": 2, "BPRhardafter": 3, "BPRbefore": 4, "BPRhardbefore": 5, "listnet": 6,
              "softmaxCE": 7, "attention_rank": 8, "BPRsimple": 9}


def list_kind(loss_n):
    """ImpressionModel's --loss_n -> rc_list_kind, by the reference's own substring rules (models/BaseImpressionModel.py:50-89:
    any name containing 'BPR'; 'hard' / 'after' / 'before' / 'simple' anywhere in it, in the reference's elif order); None
    for unknown names"""
    if "BPR" in loss_n:
        if "simple" in loss_n and "after" not in loss_n and "before" not in loss_n:
            return LIST_KINDS["BPRsimple"]
        base = "BPRhard" if "hard" in loss_n else "BPR"
        return LIST_KINDS[base + ("after" if "after" in loss_n else ("before" if "before" in loss_n else ""))]
    return LIST_KINDS.get(loss_n)


def list_loss(pred, target, max_pos, kind, need_grad=True):
    """rc_list_loss_fwd_bwd: any list-wise loss of ImpressionModel.loss -> (loss [1] -- [B] unreduced for 'BPR...simple' --,
    gpred | None); kind from list_kind()"""
    B, n = pred.shape
    dev, f32 = pred.device, torch.float32
    loss_vec = torch.empty(B, dtype=f32, device=dev)
    h_sum = torch.empty(1, dtype=f32, device=dev)
    gpred = torch.empty_like(pred) if need_grad else None
    _lib.call("rc_list_loss_fwd_bwd", _ptr(pred, f32, "pred"), _ptr(target, torch.int64, "target"), B, n, int(max_pos), int(kind),
              1.0 if kind == LIST_KINDS["BPRsimple"] else 1.0 / B, _ptr(loss_vec, f32, "loss_vec"), _ptr(h_sum, f32, "h_sum"),
              _ptr(gpred, f32, "gpred", True), _stream())
    if kind == LIST_KINDS["BPRsimple"]:
        return loss_vec, gpred        # unreduced rows [B] (reference :83); gpred[b] = d loss_vec[b] / d pred[b]
    return reduce_sum(loss_vec, 1.0 / B if kind <= 5 else 1.0), gpred


# ---- factorization-machine term, BCE ----------------------------------------------------------------------

def fm_second_order(V):
    """V [..., F, d] stacked field vectors -> 0.5*sum_k((sum_f v)^2 - sum_f v^2), shape [...]
    (models/context/FM.py:61, DeepFM.py:22-23)"""
    F, d = V.shape[-2], V.shape[-1]
    n = V.numel() // (F * d)
    out = torch.empty(V.shape[:-2], dtype=torch.float32, device=V.device)
    _lib.call("rc_fm_second_order_fwd", _ptr(V, torch.float32, "V"), n, F, d, _ptr(out, torch.float32, "out"), _stream())
    return out


def fm_second_order_bwd(V, gout, add=None):
    """d fm_second_order / dV times gout, plus `add` (the same vectors' gradient through another consumer) when given"""
    F, d = V.shape[-2], V.shape[-1]
    n = V.numel() // (F * d)
    dV = torch.empty_like(V)
    _lib.call("rc_fm_second_order_bwd", _ptr(V, torch.float32, "V"), _ptr(gout, torch.float32, "gout"), n, F, d,
              _ptr(add, torch.float32, "add", True), _ptr(dV, torch.float32, "dV"), _stream())
    return dV


def bce_ranking(pred, need_grad=True):
    """ContextModel.loss with loss_n 'BCE' (models/BaseContextModel.py:53-56) -> (loss [1], gpred | None)"""
    B, Cn = pred.shape
    f32 = torch.float32
    loss_vec = torch.empty(B, dtype=f32, device=pred.device)
    gpred = torch.empty_like(pred) if need_grad else None
    _lib.call("rc_bce_ranking_fwd_bwd", _ptr(pred, f32, "pred"), B, Cn, 1.0 / B, _ptr(loss_vec, f32, "loss_vec"),
              _ptr(gpred, f32, "gpred", True), _stream())
    return reduce_sum(loss_vec, 1.0 / B), gpred


FIELD_IDS, FIELD_F32, FIELD_F64, FIELD_I64 = 0, 1, 2, 3   # enum rc_field_kind


def field_kind(values):
    """rc_field_kind of a numeric feature's value tensor (what `feed_dict[f].float()` of models/context/FM.py:47-48 starts from)"""
    kind = {torch.float32: FIELD_F32, torch.float64: FIELD_F64, torch.int64: FIELD_I64}.get(values.dtype)
    if kind is None:
        raise ValueError("numeric field values must be float32, float64 or int64, got {}".format(values.dtype))
    return kind


# gather_fields' result; the parts that were not asked for are None.  offsets: row_offset per field + the total row count
FieldGather = collections.namedtuple("FieldGather", "out out1 cid offsets fm_term fm_sum plan_ws")


def gather_fields(tables, ids, n_cand, want_cid=True, tables1=None, mark=None, kinds=None, numeric_key=-1, fm=False, plan=False, bump=None):
    """tables: list of F [vocab_f, d] tensors; ids: list of F int64 tensors, [B] (per-row field) or [B, C]
    -> FieldGather(out [B, C, F, d], out1, cid [B, C, F], offsets, fm_term, fm_sum, plan_ws): all field lookups in one launch
    (rc_gather_fields; with fm / plan rc_gather_fields_fused).
    tables1: F [vocab_f, 1] tables looked up with the same ids -> out1 [B, C, F, 1]
    mark = (row_flags int32 [sum of vocab sizes], step_dev int64 [1]): the looked-up rows are stamped with the number of the
    step in progress, step_dev + 1 (for dense_update_rows)
    kinds: per field FIELD_IDS or the value type of a NUMERIC field (models/context/FM.py:38-41,47-48):
    tables[f] is then the Linear(1, d) weight [d, 1], tables1[f] the Linear(1, 1) weight [1, 1], ids[f] the feature's values;
    such a field owns no row of the concatenated table and its occurrences carry `numeric_key` in cid
    fm / plan (d in 16 / 32 / 64 / 128, tables1 given): the same launch also forms the FM pairwise term fm_term [B, C] + the field
    sums fm_sum [B, C, d], and / or groups the composite keys for the backward pass's row sums (small batches) into a fresh
    workspace plan_ws; bump: an int64 [1] device counter the same launch increments (the caller promises nothing in the launch
    reads it; recorded for step_increment: bumped_early)"""
    F = len(tables)
    kinds = [FIELD_IDS] * F if kinds is None else [int(k) for k in kinds]
    d = next((t.shape[1] for t, k in zip(tables, kinds) if k == FIELD_IDS), tables[0].shape[0])
    B = ids[0].shape[0]
    dev, f32, i64 = tables[0].device, torch.float32, torch.int64
    out = torch.empty((B, n_cand, F, d), dtype=f32, device=dev)
    cid = torch.empty((B, n_cand, F), dtype=i64, device=dev) if want_cid else None
    offs, run = [], 0
    for t, k in zip(tables, kinds):
        if tuple(t.shape[-2:]) != ((t.shape[0], d) if k == FIELD_IDS else (d, 1)):
            raise ValueError("gather_fields: all tables need the same width (a numeric field's weight is [d, 1])")
        offs.append(run)
        run += t.shape[0] if k == FIELD_IDS else 0
    for x, k in zip(ids, kinds):
        if k != FIELD_IDS and field_kind(x) != k:
            raise ValueError("gather_fields: kind {} does not match the value dtype {}".format(k, x.dtype))
    out1 = tab1_arr = None
    if tables1 is not None:
        if len(tables1) != F or any(t1.shape != ((t.shape[0], 1) if k == FIELD_IDS else (1, 1)) for t, t1, k in zip(tables, tables1, kinds)):
            raise ValueError("gather_fields: the second family must be [vocab_f, 1] tables of the same vocabularies")
        out1 = torch.empty((B, n_cand, F, 1), dtype=f32, device=dev)
        tab1_arr = (C.c_void_p * F)(*[_ptr(t, f32, "table1").value for t in tables1])
    flags = step_dev = None
    if mark is not None:
        flags, step_dev = mark
        if tables1 is None:
            raise ValueError("gather_fields: row flags come with the pair gather")
        if flags.numel() != run:
            raise ValueError("gather_fields: one row flag per row of the concatenated tables")
    fused = bool(fm or plan)
    if fused and (tables1 is None or d not in (16, 32, 64, 128)):
        raise ValueError("gather_fields: the FM term / the plan ride with the pair gather at d in 16 / 32 / 64 / 128")
    if bump is not None and not fused:
        raise ValueError("gather_fields: a counter rides in the fused launch only (fm / plan)")
    args = [(C.c_void_p * F)(*[_ptr(t, f32, "table").value for t in tables]), tab1_arr,
            (C.c_void_p * F)(*[_ptr(x, i64 if k == FIELD_IDS else x.dtype, "ids").value for x, k in zip(ids, kinds)]),
            (C.c_int * F)(*[1 if x.dim() == 1 else 0 for x in ids]), (C.c_int * F)(*kinds), int(numeric_key), (C.c_int64 * F)(*offs),
            F, B, int(n_cand), d, _ptr(out, f32, "out"), _ptr(out1, f32, "out1", True), _ptr(cid, i64, "cid", True),
            _ptr(flags, torch.int32, "row_flags", True), _ptr(step_dev, i64, "step_dev", True), 1]
    fm_term = fm_sum = plan_ws = None
    if fused:
        if fm:
            fm_term = torch.empty((B, n_cand), dtype=f32, device=dev)
            fm_sum = torch.empty((B, n_cand, d), dtype=f32, device=dev)
        if plan:    # not the name-keyed workspace cache: the plan lives from this forward to its backward
            plan_ws = torch.empty(_lib.load().rc_small_row_sums_workspace_bytes(B * n_cand * F), dtype=torch.uint8, device=dev)
        args += [_ptr(fm_term, f32, "fm_out", True), _ptr(fm_sum, f32, "fm_sum", True), C.c_void_p(plan_ws.data_ptr()) if plan else None,
                 plan_ws.numel() if plan else 0, _ptr(bump, i64, "bump", True)]
    _lib.call("rc_gather_fields_fused" if fused else "rc_gather_fields", *args, _stream())
    if bump is not None:
        _bumped_early.append(bump)
    return FieldGather(out, out1, cid, offs + [run], fm_term, fm_sum, plan_ws)


def numeric_field_grads(gV, gL, values, fields, n_fields, n_cand, d):
    """weight gradients of the numeric fields (rc_numeric_field_grads): gV [n, F, d] | None, gL [n, F] | None per-occurrence
    gradient blocks, values[j] / fields[j] the value tensor and field index of numeric field j
    -> (list of dW [d, 1] | None, list of dw1 [1, 1] | None)"""
    J = len(values)
    src = gV if gV is not None else gL
    dev, f32 = src.device, torch.float32
    B = values[0].shape[0]
    arrays, dW, dW_arr, dw1, dw1_arr = _numeric_arrays(values, fields, dev, d if gV is not None else None, want_dw1=gL is not None)
    nbytes = _lib.load().rc_numeric_field_grads_workspace_bytes(B * n_cand, J, d)
    ws = workspace(nbytes, dev, "numeric_fields")
    _lib.call("rc_numeric_field_grads", _ptr(gV, f32, "gV", True), _ptr(gL, f32, "gL", True), *arrays, J,
              int(n_fields), B, int(n_cand), int(d), dW_arr, dw1_arr, *_ws_args(ws))
    return (None if dW is None else [dW[j] for j in range(J)]), (None if dw1 is None else [dw1[j] for j in range(J)])


def bce_prob(p, y, need_grad=True):
    """nn.BCELoss()(p, y) on probabilities (models/BaseModel.py:259-267) -> (loss [1], dloss/dp | None)"""
    n = p.numel()
    f32 = torch.float32
    loss_vec = torch.empty(n, dtype=f32, device=p.device)
    gp = torch.empty_like(p) if need_grad else None
    _lib.call("rc_bce_prob_fwd_bwd", _ptr(p, f32, "p"), _ptr(y, f32, "y"), n, 1.0 / n, _ptr(loss_vec, f32, "loss_vec"),
              _ptr(gp, f32, "gp", True), _stream())
    return reduce_sum(loss_vec, 1.0 / n), gp


def ctr_head(bias, lin, term1, term2, label):
    """rc_ctr_head_fwd_bwd: p = sigmoid(bias + lin.sum(-1) (+ term1) (+ term2)), BCE loss [1] and d loss / d logit [n].
    lin [n, F] fp32; term1 / term2 [n] | None; label int64 [n]"""
    n, F = lin.shape
    f32 = torch.float32
    p = torch.empty(n, dtype=f32, device=lin.device)
    loss_vec = torch.empty(n, dtype=f32, device=lin.device)
    gz = torch.empty(n, dtype=f32, device=lin.device)
    _lib.call("rc_ctr_head_fwd_bwd", _ptr(bias, f32, "bias"), _ptr(lin, f32, "lin"), int(F), _ptr(term1, f32, "term1", True),
              _ptr(term2, f32, "term2", True), _ptr(label, torch.int64, "label"), n, _ptr(p, f32, "p"), _ptr(loss_vec, f32, "loss_vec"),
              _ptr(gz, f32, "gz"), _stream())
    return p, reduce_sum(loss_vec, 1.0 / n), gz


CTR_HEAD_ONE_WG_MAX = 65536   # rows the one-workgroup head (rc_ctr_head_fwd_bwd_sums) takes


def ctr_head_sums(bias, lin, term1, term2, label, full=False):
    """ctr_head in one workgroup that also forms the loss mean and sum gz: -> (p [n], sums [2] = (loss, sum gz), gz [n]).
    full=True (g_lin / g_bias / bump given): the same launch leaves the backward fan-out for a seed gradient of exactly one --
    -> (p, sums, gz, g_lin [n, F], g_bias [1]) -- and takes a pending deferred counter increment along (Adam's step count)"""
    n, F = lin.shape
    f32 = torch.float32
    p = torch.empty(n, dtype=f32, device=lin.device)
    loss_vec = torch.empty(n, dtype=f32, device=lin.device)
    gz = torch.empty(n, dtype=f32, device=lin.device)
    sums = torch.empty(2, dtype=f32, device=lin.device)
    g_lin = g_bias = bump = None
    if full:
        g_lin = torch.empty((n, F), dtype=f32, device=lin.device)
        g_bias = torch.empty(1, dtype=f32, device=lin.device)
        bump = pending_deferred()
        if bump is not None and bump.device != lin.device:
            bump = None
    _lib.call("rc_ctr_head_fwd_bwd_sums", _ptr(bias, f32, "bias"), _ptr(lin, f32, "lin"), int(F), _ptr(term1, f32, "term1", True),
              _ptr(term2, f32, "term2", True), _ptr(label, torch.int64, "label"), n, _ptr(p, f32, "p"), _ptr(loss_vec, f32, "loss_vec"),
              _ptr(gz, f32, "gz"), _ptr(sums, f32, "sums"), _ptr(g_lin, f32, "g_lin", True), _ptr(g_bias, f32, "g_bias", True),
              _ptr(bump, torch.int64, "bump", True), _stream())
    if bump is not None:
        fold_deferred(bump)
    return (p, sums, gz, g_lin, g_bias) if full else (p, sums, gz)


def ctr_head_bwd(gz, sums, g_loss, F):
    """backward fan-out of the head: -> (g [n] = gz * g_loss, g_lin [n, F] (contiguous), g_bias [1])"""
    n = gz.shape[0]
    f32 = torch.float32
    g = torch.empty(n, dtype=f32, device=gz.device)
    g_lin = torch.empty((n, F), dtype=f32, device=gz.device)
    g_bias = torch.empty(1, dtype=f32, device=gz.device)
    _lib.call("rc_ctr_head_bwd", _ptr(gz, f32, "gz"), _ptr(sums, f32, "sums"), _ptr(g_loss, f32, "g_loss"), n, int(F), _ptr(g, f32, "g"),
              _ptr(g_lin, f32, "g_lin"), _ptr(g_bias, f32, "g_bias"), _stream())
    return g, g_lin, g_bias


# ---- batch assembly on the device (csrc/sampler.hip) -------------------------------------------------------

def sample_negatives(users, K, n_items, clicked_ptr=None, clicked_items=None, seed=0, base_index=0, out=None):
    """neg [n, K] int64: uniform over [1, n_items) minus the user's clicked set (models/BaseModel.py:206-214)"""
    n = users.numel()
    i64 = torch.int64
    neg = out if out is not None else torch.empty((n, K), dtype=i64, device=users.device)
    _lib.call("rc_sample_negatives", _ptr(users, i64, "users"), n, int(K), int(n_items),
              _ptr(clicked_ptr, i64, "clicked_ptr", True), _ptr(clicked_items, i64, "clicked_items", True),
              C.c_uint64(int(seed) & (2**64 - 1)), C.c_uint64(int(base_index)), _ptr(neg, i64, "neg"), _stream())
    return neg


def assemble_candidates(idx, users, items, neg):
    """(user_id [B], item_id [B, 1+K]) for the rows idx of a training set (models/BaseModel.py:192-203)"""
    B = idx.numel()
    K = 0 if neg is None else neg.shape[1]
    i64 = torch.int64
    u = torch.empty(B, dtype=i64, device=idx.device)
    cand = torch.empty((B, 1 + K), dtype=i64, device=idx.device)
    _lib.call("rc_assemble_candidates", _ptr(idx, i64, "idx"), B, K, _ptr(users, i64, "users"), _ptr(items, i64, "items"),
              _ptr(neg, i64, "neg", True), _ptr(u, i64, "users_out"), _ptr(cand, i64, "cand_out"), _stream())
    return u, cand


def gather_history(idx, users, position, his_ptr, his_items, L, his_times=None):
    """-> (history_items [B, L] right-padded with 0, history_times | None, lengths [B])  (models/BaseModel.py:236-245)"""
    B = idx.numel() if idx is not None else users.numel()
    i64 = torch.int64
    dev = users.device
    hist = torch.empty((B, L), dtype=i64, device=dev)
    times = torch.empty((B, L), dtype=i64, device=dev) if his_times is not None else None
    lengths = torch.empty(B, dtype=i64, device=dev)
    _lib.call("rc_gather_history", _ptr(idx, i64, "idx", True), B, int(L), _ptr(users, i64, "users"),
              _ptr(position, i64, "position"), _ptr(his_ptr, i64, "his_ptr"), _ptr(his_items, i64, "his_items"),
              _ptr(his_times, i64, "his_times", True), _ptr(hist, i64, "hist"), _ptr(times, i64, "times", True),
              _ptr(lengths, i64, "lengths"), _stream())
    return hist, times, lengths


# ---- evaluation (csrc/eval_rank.hip) ---------------------------------------------------------------------------

def target_rank(pred):
    """rank of column 0 among the row's candidates, ties against it (helpers/BaseRunner.py:62-63) -> int32 [n]"""
    n, Cn = pred.shape
    rank = torch.empty(n, dtype=torch.int32, device=pred.device)
    _lib.call("rc_target_rank", _ptr(pred, torch.float32, "pred"), n, Cn, _ptr(rank, torch.int32, "rank"), _stream())
    return rank


def full_catalogue_rank_supported(d):
    return bool(_lib.load().rc_full_catalogue_rank_supported(int(d)))


def full_catalogue_rank(Uvec, I, users, targets, clicked_ptr=None, clicked_items=None):
    """--test_all rank of the target among ALL items, clicked items masked -> (rank int32 [N], target_score [N])"""
    N, d = Uvec.shape
    i64, f32 = torch.int64, torch.float32
    rank = torch.empty(N, dtype=torch.int32, device=Uvec.device)
    tscore = torch.empty(N, dtype=f32, device=Uvec.device)
    _lib.call("rc_full_catalogue_rank", _ptr(Uvec, f32, "Uvec"), _ptr(I, f32, "I"), _ptr(users, i64, "users", True),
              _ptr(targets, i64, "targets"), N, I.shape[0], d, _ptr(clicked_ptr, i64, "clicked_ptr", True),
              _ptr(clicked_items, i64, "clicked_items", True), _ptr(tscore, f32, "target_score"),
              _ptr(rank, torch.int32, "rank"), _stream())
    return rank, tscore


def rank_metrics(rank, topk, metrics):
    """HR@k / NDCG@k from gt ranks (helpers/BaseRunner.py:64-76); a few scalar reductions, one D2H copy"""
    rank = rank.to(torch.float64)
    keys, vals = [], []
    for k in topk:
        hit = (rank <= k).to(torch.float64)
        for metric in metrics:
            if metric == "HR":
                vals.append(hit.mean())
            elif metric == "NDCG":
                vals.append((hit / torch.log2(rank + 1)).mean())
            else:
                raise ValueError("Undefined evaluation metric: {}.".format(metric))
            keys.append("{}@{}".format(metric, k))
    out = torch.stack(vals).cpu().numpy() if vals else []
    return {k: float(v) for k, v in zip(keys, out)}


def list_metrics_supported(n, max_pos, n_k):
    return bool(_lib.load().rc_list_metrics_supported(int(n), int(max_pos), int(n_k)))


def list_metrics(pred, pos_num, neg_num, max_pos, topk, want_mean=True):
    """ImpressionRunner's HR / NDCG / MAP @k (helpers/ImpressionRunner.py:18-66,74-133) on the device:
    pred [N, n] fp32, pos_num [N] int64 | None, neg_num [N] int64 -> (per_row float64 [N, 3, K], mean float64 [3, K] | None),
    metric order NDCG, MAP, HR"""
    N, n = pred.shape
    K = len(topk)
    dev, f64, i64 = pred.device, torch.float64, torch.int64
    per_row = torch.empty((N, 3, K), dtype=f64, device=dev)
    mean = torch.empty((3, K), dtype=f64, device=dev) if want_mean else None
    ks = (C.c_int * K)(*[int(k) for k in topk])
    _lib.call("rc_list_metrics", _ptr(pred, torch.float32, "pred") if N else None, _ptr(pos_num, i64, "pos_num", True),
              _ptr(neg_num, i64, "neg_num") if N else None, N, int(n), int(max_pos), ks, K, _ptr(per_row, f64, "per_row") if N else None,
              _ptr(mean, f64, "mean", True), _stream())
    return per_row, mean


# ---- row-sharded step: local kernels (csrc/owner_step.hip) --------------------------------------------------

def route_by_owner(ids, world, tuple_base=None, div=1):
    """stable grouping of ids by id % world -> (order int32 [n], counts int64 [world] on the device, payload
    int64 [n]: local rows id // world, or (tuple_base + position // div) << 32 | local row)"""
    ids = ids.reshape(-1)
    n = ids.numel()
    dev, i64 = ids.device, torch.int64
    order = torch.empty(n, dtype=torch.int32, device=dev)
    payload = torch.empty(n, dtype=i64, device=dev)
    counts = torch.empty(world, dtype=i64, device=dev)
    lib = _lib.load()
    ws = workspace(lib.rc_route_workspace_bytes(n, world), dev, "route")
    packed = tuple_base is not None
    _lib.call("rc_route_by_owner", _ptr(ids, i64, "ids"), n, int(world), int(tuple_base or 0), int(div),
              _ptr(order, torch.int32, "order"), _ptr(payload if packed else None, i64, "packed", True),
              _ptr(None if packed else payload, i64, "local_row", True), _ptr(counts, i64, "counts"),
              *_ws_args(ws))
    return order, counts, payload


def owner_unpack(recv):
    """(tuple << 32 | row) messages -> (t_idx int64, rows int64, t32 int32-typed uint32)"""
    n = recv.numel()
    dev, i64 = recv.device, torch.int64
    t_idx, rows = torch.empty(n, dtype=i64, device=dev), torch.empty(n, dtype=i64, device=dev)
    t32 = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.call("rc_owner_unpack", _ptr(recv, i64, "packed"), n, _ptr(t_idx, i64, "t_idx"), _ptr(rows, i64, "rows"),
              _ptr(t32, torch.int32, "t32"), _stream())
    return t_idx, rows, t32


def owner_backward_supported(d):
    return int(d) in (16, 32, 64, 128, 256)


def owner_backward(I, mI, vI, Uall, t32, rows, g, single, n_tuples, hyper):
    """pug [n_tuples, d] = per-tuple sum of g * I[row]; rows flagged in `single` are updated in place"""
    n = rows.numel()
    d = I.shape[1]
    f32 = torch.float32
    pug = torch.empty((n_tuples, d), dtype=f32, device=I.device)
    ws = workspace(_lib.load().rc_owner_backward_workspace_bytes(n), I.device, "owner")
    _lib.call("rc_owner_backward", *_table_args(I, mI, vI, need_W=True), d,
              _ptr(Uall, f32, "Uall"), _ptr(t32, torch.int32, "t32"), _ptr(rows, torch.int64, "rows"),
              _ptr(g, f32, "g"), _ptr(single, torch.uint8, "single", True), n, int(n_tuples),
              _hyper_ref(hyper), _ptr(pug, f32, "pug"), *_ws_args(ws))
    return pug


# ---- LightGCN graph propagation (models/general/LightGCN.py:137-151) ---------------------------------------------------------

def lgcn_check_shape(d, n_layers, n_nodes=0, nnz=0):
    """rc_lgcn_check_shape (host logic): d % 4 == 0, 4 <= d <= 256, 0 <= n_layers <= 8, N < 2^31, nnz < 2^31; raises ValueError
    with the library's reason otherwise"""
    _check_shape("LightGCN", "rc_lgcn_check_shape", d, n_layers, n_nodes, nnz)


def _lgcn_check(graph, d, n_layers):
    lgcn_check_shape(d, n_layers, graph.N, graph.nnz)


def lgcn_propagate_fwd(graph, user_emb, item_emb, n_layers, out=None):
    """mean(E_0, A E_0, ..., A^L E_0) over the graph (rechorus_amd.lgcn.LgcnGraph), E_0 = (user_emb | item_emb) read in place
    -> out [N, d] (the graph's persistent output buffer when out is the string "persistent", a new tensor when None)"""
    d = user_emb.shape[1]
    _lgcn_check(graph, d, n_layers)
    if user_emb.shape != (graph.n_users, d) or item_emb.shape != (graph.n_items, d):
        raise ValueError(f"lgcn_propagate_fwd: tables {tuple(user_emb.shape)} / {tuple(item_emb.shape)} do not match the graph "
                         f"({graph.n_users} users, {graph.n_items} items)")
    buf_a, buf_b, parts, persistent = graph.buffers(d)
    if isinstance(out, str) and out == "persistent":
        out = persistent
    elif out is None:
        out = torch.empty((graph.N, d), dtype=torch.float32, device=user_emb.device)
    _lib.call("rc_lgcn_propagate_fwd", C.byref(graph.struct), _ptr(user_emb, torch.float32, "user_emb"),
              _ptr(item_emb, torch.float32, "item_emb"), d, int(n_layers), _ptr(buf_a, torch.float32, "buf_a"),
              _ptr(buf_b, torch.float32, "buf_b"), _ptr(parts, torch.float32, "partials"), _ptr(out, torch.float32, "out"), _stream())
    return out


def lgcn_propagate_bwd(graph, grad_user, grad_item, n_layers):
    """gradient of lgcn_propagate_fwd: sum_l A^l G / (L+1), split into the two tables -> (grad_user_emb, grad_item_emb)"""
    d = grad_user.shape[1]
    _lgcn_check(graph, d, n_layers)
    if grad_user.shape != (graph.n_users, d) or grad_item.shape != (graph.n_items, d):
        raise ValueError("lgcn_propagate_bwd: gradient shapes do not match the graph")
    buf_a, buf_b, parts, _ = graph.buffers(d)
    gu = torch.empty((graph.n_users, d), dtype=torch.float32, device=grad_user.device)
    gi = torch.empty((graph.n_items, d), dtype=torch.float32, device=grad_user.device)
    _lib.call("rc_lgcn_propagate_bwd", C.byref(graph.struct), _ptr(grad_user, torch.float32, "grad_user"),
              _ptr(grad_item, torch.float32, "grad_item"), d, int(n_layers), _ptr(buf_a, torch.float32, "buf_a"),
              _ptr(buf_b, torch.float32, "buf_b"), _ptr(parts, torch.float32, "partials"), _ptr(gu, torch.float32, "grad_user_emb"),
              _ptr(gi, torch.float32, "grad_item_emb"), _stream())
    return gu, gi


# ---- DirectAU alignment + uniformity loss (models/general/DirectAU.py:54-88) -----------------------------------------------------

def directau_check_shape(d, batch=1):
    """rc_directau_check_shape (host logic): d % 4 == 0, 4 <= d <= 256, 1 <= batch <= 2^20; raises ValueError with the library's
    reason otherwise"""
    _check_shape("DirectAU", "rc_directau_check_shape", d, batch)


class DirectAUWorkspace(_ShapeWorkspace):
    """the scratch of rc_directau_fwd / _bwd, one buffer per (batch, d) that is never freed or moved while the owner lives: a
    captured training step replays on the same memory.  `generation` counts forwards, so that a backward can tell whether another
    forward has overwritten what it reads."""
    _query, _shape, _order = "rc_directau_workspace_bytes", ("batch", "d"), ("d", "batch")


def _dau_rows(name, t, batch, d):
    if t.dim() != 2 or t.shape[1] != d or (batch is not None and t.shape[0] != batch):
        raise ValueError(f"directau: {name} must be [batch, {d}], got {tuple(t.shape)}")


def directau_fwd(user_e, item_e, gamma=1.0, sets=3, workspace=None, user_ids=None, item_ids=None, prediction=False):
    """rc_directau_fwd on rows user_e[user_ids] / item_e[item_ids] (ids None: the [B, d] rows themselves) -> (out [4] = loss, align,
    unif_user, unif_item; prediction [B, 1] or None; the workspace buffer; its generation).  workspace: a DirectAUWorkspace that
    persists (a model's, so that a captured step replays on the same memory); None: a fresh one for this call alone"""
    d = user_e.shape[-1]
    B = user_ids.numel() if user_ids is not None else user_e.shape[0]
    directau_check_shape(d, B)
    _dau_rows("user rows", user_e, None if user_ids is not None else B, d)
    _dau_rows("item rows", item_e, None if item_ids is not None else B, d)
    for name, ids in (("user_ids", user_ids), ("item_ids", item_ids)):
        if ids is not None and ids.numel() != B:
            raise ValueError(f"directau: {name} must hold {B} ids")
    ws = workspace if workspace is not None else DirectAUWorkspace()   # None: a private one, alive as long as the caller keeps it
    buf, gen = ws.get(B, d, user_e.device), ws.stamp()
    out = torch.empty(4, dtype=torch.float32, device=user_e.device)
    pred = torch.empty((B, 1), dtype=torch.float32, device=user_e.device) if prediction else None
    uid = user_ids.reshape(-1).contiguous() if user_ids is not None else None
    iid = item_ids.reshape(-1).contiguous() if item_ids is not None else None
    _lib.call("rc_directau_fwd", _ptr(user_e, torch.float32, "user_e"), _ptr(uid, torch.int64, "user_ids", allow_none=True),
              _ptr(item_e, torch.float32, "item_e"), _ptr(iid, torch.int64, "item_ids", allow_none=True), B, d, float(gamma),
              int(sets), C.c_void_p(buf.data_ptr()), buf.numel(), _ptr(pred, torch.float32, "prediction", allow_none=True),
              _ptr(out, torch.float32, "out"), _stream())
    return out, pred, buf, gen


def directau_bwd(grad_out, batch, d, coef, buf, want_user=True, want_item=True):
    """rc_directau_bwd: grad_out [] / [1] on the device, coef = (align, unif_user, unif_item) -> (grad_user [B, d] | None,
    grad_item [B, d] | None), the per-occurrence row gradients"""
    directau_check_shape(d, batch)
    dev = buf.device
    g = grad_out.reshape(1).to(torch.float32).contiguous()
    gu = torch.empty((batch, d), dtype=torch.float32, device=dev) if want_user else None
    gi = torch.empty((batch, d), dtype=torch.float32, device=dev) if want_item else None
    _lib.call("rc_directau_bwd", _ptr(g, torch.float32, "grad_out"), int(batch), int(d), float(coef[0]), float(coef[1]),
              float(coef[2]), C.c_void_p(buf.data_ptr()), buf.numel(), _ptr(gu, torch.float32, "grad_user", allow_none=True),
              _ptr(gi, torch.float32, "grad_item", allow_none=True), _stream())
    return gu, gi


# ---- ComiRec multi-interest extraction (models/sequential/ComiRec.py:57-93) --------------------------------------------------------

def comirec_check_shape(d, attn_size, K, L):
    """rc_comirec_check_shape (host logic): d % 4 == 0, 4 <= d <= 256, 1 <= attn_size <= 64, 1 <= K <= 16, 1 <= L <= 256; raises
    ValueError with the library's reason otherwise"""
    _check_shape("ComiRec", "rc_comirec_check_shape", d, attn_size, K, L)


class ComiRecWorkspace(_ShapeWorkspace):
    """the scratch of rc_comirec_bwd (the per-workgroup partials of the weight gradients), one buffer per shape that is never
    freed or moved while the owner lives"""
    _query, _shape, _floor = "rc_comirec_workspace_bytes", ("d", "attn_size", "K", "L", "batch"), 256


def _comirec_shapes(item_emb, pos_emb, W1, b1, W2, b2, hist, lengths):
    d = item_emb.shape[1]
    A, K = W1.shape[0], W2.shape[0]
    if hist.dim() != 2 or hist.shape[0] < 1:
        raise ValueError(f"comirec: history must be [batch >= 1, L], got {tuple(hist.shape)}")
    B, L = hist.shape
    comirec_check_shape(d, A, K, L)
    if W1.shape != (A, d) or b1.shape != (A,) or W2.shape != (K, A) or (b2 is not None and b2.shape != (K,)):
        raise ValueError("comirec: W1 [attn_size, d], b1 [attn_size], W2 [K, attn_size], b2 [K] expected")
    if pos_emb is not None and pos_emb.shape[1] != d:
        raise ValueError("comirec: the position table must have the item table's width")
    if lengths.shape != (B,):
        raise ValueError(f"comirec: lengths must be [{B}], got {tuple(lengths.shape)}")
    return B, L, d, A, K


def comirec_fwd(item_emb, pos_emb, W1, b1, W2, b2, hist, lengths, targets=None, want_attn=True):
    """rc_comirec_fwd: ComiRec.py:64-87 in one launch -> (interests [B, K, d], attn [B, K, L] | None, sel int32 [B] | None,
    user [B, d] | None); pos_emb None: --add_pos 0; targets [B] item ids: the hard selection of the training path"""
    B, L, d, A, K = _comirec_shapes(item_emb, pos_emb, W1, b1, W2, b2, hist, lengths)
    dev, f32 = item_emb.device, torch.float32
    if targets is not None and targets.shape != (B,):
        raise ValueError(f"comirec: targets must be [{B}], got {tuple(targets.shape)}")
    interests = torch.empty((B, K, d), dtype=f32, device=dev)
    attn = torch.empty((B, K, L), dtype=f32, device=dev) if want_attn else None
    sel = torch.empty(B, dtype=torch.int32, device=dev) if targets is not None else None
    user = torch.empty((B, d), dtype=f32, device=dev) if targets is not None else None
    _lib.call("rc_comirec_fwd", _ptr(item_emb, f32, "item_emb"), item_emb.shape[0], _ptr(pos_emb, f32, "pos_emb", allow_none=True),
              pos_emb.shape[0] if pos_emb is not None else 0, _ptr(W1, f32, "W1"), _ptr(b1, f32, "b1"), _ptr(W2, f32, "W2"),
              _ptr(b2, f32, "b2"), _ptr(hist, torch.int64, "history"), _ptr(lengths, torch.int64, "lengths"),
              _ptr(targets, torch.int64, "targets", allow_none=True), B, L, d, A, K, _ptr(interests, f32, "interests"),
              _ptr(attn, f32, "attn", allow_none=True), _ptr(sel, torch.int32, "sel", allow_none=True),
              _ptr(user, f32, "user", allow_none=True), _stream())
    return interests, attn, sel, user


def comirec_bwd(item_emb, pos_emb, W1, b1, W2, hist, lengths, attn, sel, user, d_user, workspace=None):
    """rc_comirec_bwd -> (g_hist [B, L, d], g_x [B, L, d] | None, dW1, db1, dW2, db2): per-occurrence row gradients (zeros at
    invalid positions) and the weight gradients, no gradient through the selection"""
    B, L, d, A, K = _comirec_shapes(item_emb, pos_emb, W1, b1, W2, None, hist, lengths)
    dev, f32 = item_emb.device, torch.float32
    if attn.shape != (B, K, L) or sel.shape != (B,) or user.shape != (B, d) or d_user.shape != (B, d):
        raise ValueError("comirec_bwd: attn [B, K, L], sel [B], user [B, d], d_user [B, d] expected")
    ws = (workspace if workspace is not None else ComiRecWorkspace()).get(d, A, K, L, B, dev)
    g_hist = torch.empty((B, L, d), dtype=f32, device=dev)
    g_x = torch.empty((B, L, d), dtype=f32, device=dev) if pos_emb is not None else None
    dW1, db1 = torch.empty((A, d), dtype=f32, device=dev), torch.empty(A, dtype=f32, device=dev)
    dW2, db2 = torch.empty((K, A), dtype=f32, device=dev), torch.empty(K, dtype=f32, device=dev)
    _lib.call("rc_comirec_bwd", _ptr(item_emb, f32, "item_emb"), item_emb.shape[0], _ptr(pos_emb, f32, "pos_emb", allow_none=True),
              pos_emb.shape[0] if pos_emb is not None else 0, _ptr(W1, f32, "W1"), _ptr(b1, f32, "b1"), _ptr(W2, f32, "W2"),
              _ptr(hist, torch.int64, "history"), _ptr(lengths, torch.int64, "lengths"), _ptr(attn, f32, "attn"),
              _ptr(sel, torch.int32, "sel"), _ptr(user, f32, "user"), _ptr(d_user, f32, "d_user"), B, L, d, A, K,
              _ptr(g_hist, f32, "g_hist"), _ptr(g_x, f32, "g_x", allow_none=True), _ptr(dW1, f32, "dW1"), _ptr(db1, f32, "db1"),
              _ptr(dW2, f32, "dW2"), _ptr(db2, f32, "db2"), *_ws_args(ws))
    return g_hist, g_x, dW1, db1, dW2, db2


def comirec_score_max(interests, item_emb, iid):
    """rc_comirec_score_max: pred [B, C] = max_k <interests[b, k], item_emb[iid[b, c]]> (ComiRec.py:90-91)"""
    if interests.dim() != 3 or iid.dim() != 2 or iid.shape[0] != interests.shape[0] or iid.shape[1] < 1:
        raise ValueError(f"comirec_score_max: interests [B, K, d] and candidates [B, C >= 1] expected, got {tuple(interests.shape)} / "
                         f"{tuple(iid.shape)}")
    B, K, d = interests.shape
    comirec_check_shape(d, 1, K, 1)
    if item_emb.shape[1] != d:
        raise ValueError("comirec_score_max: interests and item table need the same emb_size")
    pred = torch.empty(iid.shape, dtype=torch.float32, device=interests.device)
    _lib.call("rc_comirec_score_max", _ptr(interests, torch.float32, "interests"), _ptr(item_emb, torch.float32, "item_emb"),
              item_emb.shape[0], _ptr(iid, torch.int64, "candidates"), B, iid.shape[1], d, K, _ptr(pred, torch.float32, "pred"), _stream())
    return pred


# ---- ContraRec: contrastive loss, forward-indexed position embedding (models/sequential/ContraRec.py:142-193, :259-267) -----------

def contra_check_shape(d, batch=1):
    """rc_contra_check_shape (host logic): d % 4 == 0, 4 <= d <= 256, 1 <= batch <= 2^19; raises ValueError with the library's
    reason otherwise"""
    _check_shape("ContraRec", "rc_contra_check_shape", d, batch)


def contra_layout(d, batch):
    """(column chunks, 32-row column blocks per chunk, workspace bytes) of the two sweeps at this shape: the host-side statement of
    con_layout in csrc/contrarec.hip (tests pin the byte count to rc_contra_workspace_bytes).  The sweep over the N = 2 batch stacked
    rows is split so that about 512 workgroups run: at most 16 chunks, at most one per column block."""
    N = 2 * int(batch)
    ncb = (N + 31) // 32
    nwg = (N + 127) // 128
    want = max(1, min((512 + nwg - 1) // nwg, 16, ncb))
    per = (ncb + want - 1) // want
    chunks = (ncb + per - 1) // per
    up = lambda n: (4 * n + 255) // 256 * 256
    nbytes = up(N * d) + up(N) + 4 * up(chunks * N) + 4 * up(N) + up(chunks * N * d)
    return chunks, per, nbytes


def contra_first_split_batch():
    """the smallest batch at which the layout splits the sweep into more than one column chunk"""
    B = 1
    while contra_layout(4, B)[0] < 2:
        B += 1
    return B


class ContraWorkspace(_ShapeWorkspace):
    """the scratch of rc_contra_loss_fwd / _bwd, one buffer per (batch, d) that is never freed or moved while the owner lives.
    `generation` counts forwards, so that a backward can tell whether another forward has overwritten what it reads."""
    _query, _shape, _order = "rc_contra_workspace_bytes", ("batch", "d"), ("d", "batch")


def _contra_args(va, vb, labels):
    if va.dim() != 2 or va.shape != vb.shape:
        raise ValueError(f"contra_loss: the two views must be [batch, d] alike, got {tuple(va.shape)} / {tuple(vb.shape)}")
    B, d = va.shape
    contra_check_shape(d, B)
    if labels is not None and labels.shape != (B,):
        raise ValueError(f"contra_loss: labels must be [{B}], got {tuple(labels.shape)}")
    return B, d


def contra_loss_fwd(va, vb, labels, temperature, workspace=None):
    """rc_contra_loss_fwd on the two views' un-normalised rows [B, d] -> (loss [1], the workspace buffer, its generation);
    labels int64 [B] or None (InfoNCE)"""
    B, d = _contra_args(va, vb, labels)
    ws = workspace if workspace is not None else ContraWorkspace()
    buf, gen = ws.get(B, d, va.device), ws.stamp()
    loss = torch.empty(1, dtype=torch.float32, device=va.device)
    _lib.call("rc_contra_loss_fwd", _ptr(va, torch.float32, "va"), _ptr(vb, torch.float32, "vb"),
              _ptr(labels, torch.int64, "labels", allow_none=True), B, d, float(temperature), C.c_void_p(buf.data_ptr()), buf.numel(),
              _ptr(loss, torch.float32, "loss"), _stream())
    return loss, buf, gen


def contra_loss_bwd(grad_out, labels, batch, d, temperature, buf):
    """rc_contra_loss_bwd: grad_out [] / [1] on the device -> (grad_va, grad_vb) [B, d], from what the forward left in buf"""
    contra_check_shape(d, batch)
    g = grad_out.reshape(1).to(torch.float32).contiguous()
    ga = torch.empty((batch, d), dtype=torch.float32, device=buf.device)
    gb = torch.empty((batch, d), dtype=torch.float32, device=buf.device)
    _lib.call("rc_contra_loss_bwd", _ptr(g, torch.float32, "grad_out"), _ptr(labels, torch.int64, "labels", allow_none=True),
              int(batch), int(d), float(temperature), C.c_void_p(buf.data_ptr()), buf.numel(), _ptr(ga, torch.float32, "grad_va"),
              _ptr(gb, torch.float32, "grad_vb"), _stream())
    return ga, gb


def seq_embed_fwdpos(item_emb, pos_emb, hist, lengths):
    """X [B * L, d] = item rows + position rows (position id = index) on valid rows, 0 on the padding (ContraRec.py:259-267)"""
    B, L = hist.shape
    d = item_emb.shape[1]
    if pos_emb.shape[0] < L or pos_emb.shape[1] != d:
        raise ValueError(f"seq_embed_fwdpos: the position table must be [>= {L}, {d}], got {tuple(pos_emb.shape)}")
    f32, i64 = torch.float32, torch.int64
    X = torch.empty((B * L, d), dtype=f32, device=hist.device)
    _lib.call("rc_seq_embed_fwdpos_fwd", _ptr(item_emb, f32, "item_emb"), _ptr(pos_emb, f32, "pos_emb"), _ptr(hist, i64, "hist"),
              _ptr(lengths, i64, "lengths"), B, L, d, _ptr(X, f32, "X"), _stream())
    return X


def seq_pos_grad_fwdpos(dX, lengths, B, L, n_pos):
    """dense gradient [n_pos, d] of the position table from the rows' gradients dX [B * L, d] (position id = index)"""
    d = dX.shape[1]
    if n_pos < L:
        raise ValueError(f"seq_pos_grad_fwdpos: the position table needs at least {L} rows, got {n_pos}")
    out = torch.empty((n_pos, d), dtype=torch.float32, device=dX.device)
    _lib.call("rc_seq_pos_grad_fwdpos", _ptr(dX, torch.float32, "dX"), _ptr(lengths, torch.int64, "lengths"), B, int(L), d, int(n_pos),
              _ptr(out, torch.float32, "grad_pos"), _stream())
    return out


# ---- BUIR bootstrap loss, evaluation head, target update (models/general/BUIR.py:66-110) -----------------------------------------

def buir_check_shape(d, batch=1):
    """rc_buir_check_shape (host logic): d % 16 == 0, 16 <= d <= 128, 1 <= batch <= 2^20; raises ValueError with the library's
    reason otherwise"""
    _check_shape("BUIR", "rc_buir_check_shape", d, batch)


class BuirWorkspace(_ShapeWorkspace):
    """the scratch of rc_buir_fwd / _bwd (the per-workgroup partials of loss, dW and db), one buffer per (batch, d) that is never
    freed or moved while the owner lives: a captured training step replays on the same memory.  Nothing in it outlives the call
    that wrote it (the backward pass recomputes the forward values from the tables), so two pending losses may share one
    workspace."""
    _query, _shape, _order = "rc_buir_workspace_bytes", ("batch", "d"), ("d", "batch")


def _buir_shapes(user_online, user_target, item_online, item_target, W, b, uid, iid):
    d = W.shape[-1]
    B = uid.numel()
    buir_check_shape(d, B)
    if W.shape != (d, d) or b.shape != (d,):
        raise ValueError(f"buir: predictor weight [d, d] and bias [d] expected, got {tuple(W.shape)} / {tuple(b.shape)}")
    for name, t in (("user_online", user_online), ("user_target", user_target), ("item_online", item_online),
                    ("item_target", item_target)):
        if t is not None and (t.dim() != 2 or t.shape[1] != d):
            raise ValueError(f"buir: {name} must be [rows, {d}], got {tuple(t.shape)}")
    if user_target is not None and (user_target.shape != user_online.shape or item_target.shape != item_online.shape):
        raise ValueError("buir: a target table has its online table's shape")
    if iid is not None and iid.numel() != B:
        raise ValueError(f"buir: one positive item per row expected, got {tuple(iid.shape)} for {B} users")
    return B, d


def _buir_common(tables, W, b, uid, iid):
    f32, i64 = torch.float32, torch.int64
    names = ("user_online", "user_target", "item_online", "item_target")
    return ([_ptr(t, f32, n) for t, n in zip(tables, names)] + [_ptr(W, f32, "W"), _ptr(b, f32, "b"), _ptr(uid, i64, "user ids"),
                                                                 _ptr(iid, i64, "item ids")])


def buir_fwd(user_online, user_target, item_online, item_target, W, b, uid, iid, workspace=None, prediction=True):
    """rc_buir_fwd -> (loss [], prediction [B, 1] | None): BUIR.py:73-110 for B (user, positive item) rows"""
    B, d = _buir_shapes(user_online, user_target, item_online, item_target, W, b, uid, iid)
    uid, iid = uid.reshape(-1).contiguous(), iid.reshape(-1).contiguous()
    dev = W.device
    buf = (workspace if workspace is not None else BuirWorkspace()).get(B, d, dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    pred = torch.empty((B, 1), dtype=torch.float32, device=dev) if prediction else None
    _lib.call("rc_buir_fwd", *_buir_common((user_online, user_target, item_online, item_target), W, b, uid, iid), B, d,
              C.c_void_p(buf.data_ptr()), buf.numel(), _ptr(pred, torch.float32, "prediction", allow_none=True),
              _ptr(loss, torch.float32, "loss"), _stream())
    return loss[0], pred


def buir_bwd(grad_out, user_online, user_target, item_online, item_target, W, b, uid, iid, workspace=None):
    """rc_buir_bwd: grad_out [] / [1] on the device -> (grad_user [B, d], grad_item [B, d], dW [d, d], db [d]); the first two are
    per-occurrence row gradients of the online tables"""
    B, d = _buir_shapes(user_online, user_target, item_online, item_target, W, b, uid, iid)
    uid, iid = uid.reshape(-1).contiguous(), iid.reshape(-1).contiguous()
    dev, f32 = W.device, torch.float32
    buf = (workspace if workspace is not None else BuirWorkspace()).get(B, d, dev)
    g = grad_out.reshape(1).to(f32).contiguous()
    gu, gi = torch.empty((B, d), dtype=f32, device=dev), torch.empty((B, d), dtype=f32, device=dev)
    dW, db = torch.empty((d, d), dtype=f32, device=dev), torch.empty(d, dtype=f32, device=dev)
    _lib.call("rc_buir_bwd", *_buir_common((user_online, user_target, item_online, item_target), W, b, uid, iid),
              _ptr(g, f32, "grad_out"), B, d, C.c_void_p(buf.data_ptr()), buf.numel(), _ptr(gu, f32, "grad_user"),
              _ptr(gi, f32, "grad_item"), _ptr(dW, f32, "dW"), _ptr(db, f32, "db"), _stream())
    return gu, gi, dW, db


def buir_query(user_online, W, b, uid):
    """rc_buir_query -> (q [B, d], c [B]): q_b = (W + W^T) u_b + b, c_b = <b, u_b> for u_b = user_online[uid[b]]"""
    B, d = _buir_shapes(user_online, None, None, None, W, b, uid, None)
    uid = uid.reshape(-1).contiguous()
    f32 = torch.float32
    q, c = torch.empty((B, d), dtype=f32, device=W.device), torch.empty(B, dtype=f32, device=W.device)
    _lib.call("rc_buir_query", _ptr(user_online, f32, "user_online"), _ptr(W, f32, "W"), _ptr(b, f32, "b"),
              _ptr(uid, torch.int64, "user ids"), B, d, _ptr(q, f32, "q"), _ptr(c, f32, "c"), _stream())
    return q, c


def buir_scores(q, c, item_online, iid):
    """rc_buir_scores -> [B, C]: <q_b, item_online[iid[b, c]]> + c_b"""
    if q.dim() != 2 or iid.dim() != 2 or iid.shape[0] != q.shape[0] or iid.shape[1] < 1 or c.shape != (q.shape[0],):
        raise ValueError(f"buir_scores: q [B, d], c [B] and candidates [B, C >= 1] expected, got {tuple(q.shape)} / {tuple(c.shape)} / "
                         f"{tuple(iid.shape)}")
    B, d = q.shape
    buir_check_shape(d, B)
    if item_online.dim() != 2 or item_online.shape[1] != d:
        raise ValueError("buir_scores: q and the item table need the same emb_size")
    out = torch.empty(iid.shape, dtype=torch.float32, device=q.device)
    _lib.call("rc_buir_scores", _ptr(q, torch.float32, "q"), _ptr(c, torch.float32, "c"), _ptr(item_online, torch.float32, "item_online"),
              _ptr(iid.contiguous(), torch.int64, "candidates"), B, iid.shape[1], d, _ptr(out, torch.float32, "scores"), _stream())
    return out


def ema_update(target_a, online_a, target_b, online_b, momentum):
    """rc_buir_ema: target = target * m + online * (1 - m) on both pairs in place, one launch, rounded as torch rounds the
    expression (BUIR.py:66-71)"""
    for t, o in ((target_a, online_a), (target_b, online_b)):
        if t.shape != o.shape:
            raise ValueError(f"ema_update: target {tuple(t.shape)} and online {tuple(o.shape)} differ in shape")
    f32 = torch.float32
    _lib.call("rc_buir_ema", _ptr(target_a, f32, "target_a"), _ptr(online_a, f32, "online_a"), target_a.numel(),
              _ptr(target_b, f32, "target_b"), _ptr(online_b, f32, "online_b"), target_b.numel(), float(momentum), _stream())


# ---- AutoInt field self-attention layer (models/context/AutoInt.py:49-80, utils/layers.py:9-63) ----------------------------------

def autoint_check_shape(n_fields, d_in, attention_size, num_heads):
    """rc_autoint_check_shape (host logic): 2 <= fields <= 32, d_in % 4 == 0, 4 <= d_in <= 128, 4 <= attention_size <= 64, num_heads a
    divisor of attention_size; raises ValueError with the library's reason otherwise"""
    _check_shape("AutoInt", "rc_autoint_check_shape", n_fields, d_in, attention_size, num_heads)


class AutoIntWorkspace(_ShapeWorkspace):
    """the scratch of rc_autoint_layer_bwd (the per-workgroup partials of the weight gradients), one buffer per shape that is never
    freed or moved while the owner lives: a captured training step replays on the same memory.  Nothing in it outlives the call
    that wrote it, so the layers of a stack share one workspace."""
    _query, _shape, _floor = "rc_autoint_workspace_bytes", ("n", "n_fields", "d_in", "attention_size", "num_heads"), 256


def _autoint_shapes(X, Wq, Wk, Wv, Wr, br, heads):
    if X.dim() < 3 or X.numel() == 0:
        raise ValueError(f"autoint_layer: X must be [..., fields, width] with at least one instance, got {tuple(X.shape)}")
    F, d = X.shape[-2:]
    N = X.numel() // (F * d)
    A = Wq.shape[0]
    autoint_check_shape(F, d, A, heads)
    for name, W in (("Wq", Wq), ("Wk", Wk), ("Wv", Wv), ("Wr", Wr)):
        if W.shape != (A, d):
            raise ValueError(f"autoint_layer: {name} must be [{A}, {d}], got {tuple(W.shape)}")
    if br is not None and br.shape != (A,):
        raise ValueError(f"autoint_layer: the residual bias must be [{A}], got {tuple(br.shape)}")
    return N, F, d, A


def autoint_layer_fwd(X, Wq, Wk, Wv, Wr, br, heads):
    """rc_autoint_layer_fwd: Y [..., F, A] = relu(attention over the fields of one instance + X Wr^T + br), one launch"""
    N, F, d, A = _autoint_shapes(X, Wq, Wk, Wv, Wr, br, heads)
    f32 = torch.float32
    Y = torch.empty(X.shape[:-1] + (A,), dtype=f32, device=X.device)
    _lib.call("rc_autoint_layer_fwd", _ptr(X, f32, "X"), _ptr(Wq, f32, "Wq"), _ptr(Wk, f32, "Wk"), _ptr(Wv, f32, "Wv"),
              _ptr(Wr, f32, "Wr"), _ptr(br, f32, "br"), N, F, d, A, int(heads), _ptr(Y, f32, "Y"), _stream())
    return Y


def autoint_layer_bwd(X, Wq, Wk, Wv, Wr, Y, dY, heads, workspace=None):
    """rc_autoint_layer_bwd -> (dX, dWq, dWk, dWv, dWr, dbr): Q, K, V and the softmax are recomputed from X; two launches"""
    N, F, d, A = _autoint_shapes(X, Wq, Wk, Wv, Wr, None, heads)
    if Y.shape != X.shape[:-1] + (A,) or dY.shape != Y.shape:
        raise ValueError(f"autoint_layer_bwd: Y and dY must be {tuple(X.shape[:-1]) + (A,)}, got {tuple(Y.shape)} / {tuple(dY.shape)}")
    dev, f32 = X.device, torch.float32
    ws = (workspace if workspace is not None else AutoIntWorkspace()).get(N, F, d, A, heads, dev)
    dX = torch.empty_like(X)
    dWq, dWk, dWv, dWr = (torch.empty((A, d), dtype=f32, device=dev) for _ in range(4))
    dbr = torch.empty(A, dtype=f32, device=dev)
    _lib.call("rc_autoint_layer_bwd", _ptr(X, f32, "X"), _ptr(Wq, f32, "Wq"), _ptr(Wk, f32, "Wk"), _ptr(Wv, f32, "Wv"),
              _ptr(Wr, f32, "Wr"), _ptr(Y, f32, "Y"), _ptr(dY, f32, "dY"), N, F, d, A, int(heads), C.c_void_p(ws.data_ptr()), ws.numel(),
              _ptr(dX, f32, "dX"), _ptr(dWq, f32, "dWq"), _ptr(dWk, f32, "dWk"), _ptr(dWv, f32, "dWv"), _ptr(dWr, f32, "dWr"),
              _ptr(dbr, f32, "dbr"), _stream())
    return dX, dWq, dWk, dWv, dWr, dbr


# ---- DCNv2 mixed cross layer (models/context/DCNv2.py:96-144) -----------------------------------------------------------------------

def dcnv2_check_shape(width, low_rank, expert_num):
    """rc_dcnv2_check_shape (host logic): width = fields * emb_size a multiple of 4 in [8, 1024], low_rank a multiple of 4 in
    [4, 128], expert_num in [1, 4]; raises ValueError with the library's reason otherwise"""
    _check_shape("DCNv2", "rc_dcnv2_check_shape", width, low_rank, expert_num)


class DCNv2Workspace(_ShapeWorkspace):
    """the scratch of rc_dcnv2_mix_layer_bwd (the per-workgroup partials of the weight gradients), one buffer per shape that is never
    freed or moved while the owner lives: a captured training step replays on the same memory.  Nothing in it outlives the call
    that wrote it, so the layers of a stack share one workspace."""
    _query, _shape, _floor = "rc_dcnv2_mix_layer_bwd_workspace_bytes", ("n", "width", "low_rank", "expert_num"), 256


def _dcnv2_shapes(X0, Xl, U, V, Cw, bias, Wg, bg):
    if Xl.dim() < 2 or Xl.numel() == 0 or X0.shape != Xl.shape:
        raise ValueError(f"dcnv2_mix_layer: X0 and Xl must be [..., width] of one shape with at least one row, got "
                         f"{tuple(X0.shape)} / {tuple(Xl.shape)}")
    D = Xl.shape[-1]
    N = Xl.numel() // D
    if U.dim() != 3 or U.shape[1] != D:
        raise ValueError(f"dcnv2_mix_layer: U must be [experts, {D}, low_rank], got {tuple(U.shape)}")
    E, _, r = U.shape
    dcnv2_check_shape(D, r, E)
    for name, W, shape in (("V", V, (E, D, r)), ("C", Cw, (E, r, r)), ("Wg", Wg, (E, D)), ("bg", bg, (E,))):
        if tuple(W.shape) != shape:
            raise ValueError(f"dcnv2_mix_layer: {name} must be {list(shape)}, got {tuple(W.shape)}")
    if bias.numel() != D:
        raise ValueError(f"dcnv2_mix_layer: bias must hold {D} values, got {tuple(bias.shape)}")
    return N, D, r, E


def dcnv2_mix_layer_fwd(X0, Xl, U, V, Cw, bias, Wg, bg):
    """rc_dcnv2_mix_layer_fwd: x_next [..., D] = x_l + x_0 * sum_e softmax_e(gate)_e (U_e tanh(C_e tanh(V_e^T x_l)) + bias), one launch"""
    N, D, r, E = _dcnv2_shapes(X0, Xl, U, V, Cw, bias, Wg, bg)
    f32 = torch.float32
    Xnext = torch.empty(Xl.shape, dtype=f32, device=Xl.device)
    _lib.call("rc_dcnv2_mix_layer_fwd", _ptr(X0, f32, "X0"), _ptr(Xl, f32, "Xl"), _ptr(U, f32, "U"), _ptr(V, f32, "V"), _ptr(Cw, f32, "C"),
              _ptr(bias, f32, "bias"), _ptr(Wg, f32, "Wg"), _ptr(bg, f32, "bg"), N, D, r, E, _ptr(Xnext, f32, "Xnext"), _stream())
    return Xnext


def dcnv2_mix_layer_bwd(dXnext, X0, Xl, U, V, Cw, bias, Wg, bg, workspace=None):
    """rc_dcnv2_mix_layer_bwd -> (dXl, dX0_part, dU, dV, dC, dbias, dWg, dbg): t, s and the gate are recomputed; two launches"""
    N, D, r, E = _dcnv2_shapes(X0, Xl, U, V, Cw, bias, Wg, bg)
    if dXnext.shape != Xl.shape:
        raise ValueError(f"dcnv2_mix_layer_bwd: dXnext must be {tuple(Xl.shape)}, got {tuple(dXnext.shape)}")
    dev, f32 = Xl.device, torch.float32
    ws = (workspace if workspace is not None else DCNv2Workspace()).get(N, D, r, E, dev)
    dXl = torch.empty(Xl.shape, dtype=f32, device=dev)
    dX0 = torch.empty(Xl.shape, dtype=f32, device=dev)
    dU = torch.empty((E, D, r), dtype=f32, device=dev)
    dV = torch.empty((E, D, r), dtype=f32, device=dev)
    dC = torch.empty((E, r, r), dtype=f32, device=dev)
    dbias = torch.empty(tuple(bias.shape), dtype=f32, device=dev)
    dWg = torch.empty((E, D), dtype=f32, device=dev)
    dbg = torch.empty((E,), dtype=f32, device=dev)
    _lib.call("rc_dcnv2_mix_layer_bwd", _ptr(dXnext, f32, "dXnext"), _ptr(X0, f32, "X0"), _ptr(Xl, f32, "Xl"), _ptr(U, f32, "U"),
              _ptr(V, f32, "V"), _ptr(Cw, f32, "C"), _ptr(bias, f32, "bias"), _ptr(Wg, f32, "Wg"), _ptr(bg, f32, "bg"), N, D, r, E,
              C.c_void_p(ws.data_ptr()), ws.numel(), _ptr(dXl, f32, "dXl"), _ptr(dX0, f32, "dX0_part"), _ptr(dU, f32, "dU"), _ptr(dV, f32, "dV"),
              _ptr(dC, f32, "dC"), _ptr(dbias, f32, "dbias"), _ptr(dWg, f32, "dWg"), _ptr(dbg, f32, "dbg"), _stream())
    return dXl, dX0, dU, dV, dC, dbias, dWg, dbg


# ---- list encoder block (models/reranker/PRM.py:64,90-92: nn.TransformerEncoderLayer under a key-padding mask) -------------------------

LISTENC_WEIGHTS = ("Win", "bin", "Wo", "bo", "g1", "be1", "W1", "b1", "W2", "b2", "g2", "be2")


def listenc_check_shape(n, d, heads, d_ff):
    """rc_listenc_check_shape (host logic): 1 <= n <= 64, d a multiple of 16 in [16, 128], heads a divisor of d with d / heads a
    multiple of 4, d_ff a multiple of 16 in [16, 256], and a list with the backward's intermediates within the LDS; raises ValueError
    with the library's reason otherwise"""
    _check_shape("list encoder", "rc_listenc_check_shape", n, d, heads, d_ff)


class ListEncWorkspace(_ShapeWorkspace):
    """the scratch of rc_listenc_block_bwd (the per-workgroup partials of the weight gradients), one buffer per shape that is never
    freed or moved while the owner lives: a captured training step replays on the same memory.  Nothing in it outlives the call
    that wrote it, so the blocks of a stack share one workspace."""
    _query, _shape, _floor = "rc_listenc_block_bwd_workspace_bytes", ("B", "n", "d", "heads", "d_ff"), 256


def _listenc_shapes(X, pad, weights, heads):
    if X.dim() != 3 or X.numel() == 0:
        raise ValueError(f"list_encoder_block: X must be [lists, slots, width] with at least one list, got {tuple(X.shape)}")
    B, n, d = X.shape
    if tuple(pad.shape) != (B, n):
        raise ValueError(f"list_encoder_block: pad must be [{B}, {n}], got {tuple(pad.shape)}")
    if len(weights) != len(LISTENC_WEIGHTS):
        raise ValueError(f"list_encoder_block: twelve weights are needed ({', '.join(LISTENC_WEIGHTS)})")
    W1 = weights[6]
    if W1.dim() != 2 or W1.shape[1] != d:
        raise ValueError(f"list_encoder_block: W1 must be [d_ff, {d}], got {tuple(W1.shape)}")
    dff = W1.shape[0]
    listenc_check_shape(n, d, heads, dff)
    shapes = ((3 * d, d), (3 * d,), (d, d), (d,), (d,), (d,), (dff, d), (dff,), (d, dff), (d,), (d,), (d,))
    for name, W, shape in zip(LISTENC_WEIGHTS, weights, shapes):
        if tuple(W.shape) != shape:
            raise ValueError(f"list_encoder_block: {name} must be {list(shape)}, got {tuple(W.shape)}")
    return B, n, d, dff


def listenc_block_fwd(X, pad, weights, heads):
    """rc_listenc_block_fwd: Y [B, n, d] = LN2(X1 + relu(X1 W1^T + b1) W2^T + b2), X1 = LN1(X + MHA(X; pad)), one launch.
    pad uint8 [B, n], 1 = padded slot (masked as a key); weights in LISTENC_WEIGHTS order"""
    B, n, d, dff = _listenc_shapes(X, pad, weights, heads)
    f32 = torch.float32
    Y = torch.empty(X.shape, dtype=f32, device=X.device)
    _lib.call("rc_listenc_block_fwd", _ptr(X, f32, "X"), _ptr(pad, torch.uint8, "pad"),
              *[_ptr(W, f32, k) for k, W in zip(LISTENC_WEIGHTS, weights)], B, n, d, int(heads), dff, _ptr(Y, f32, "Y"), _stream())
    return Y


def listenc_block_bwd(dY, X, pad, weights, heads, workspace=None):
    """rc_listenc_block_bwd -> (dX, [the twelve gradients in LISTENC_WEIGHTS order]): the block is recomputed from X; two launches"""
    B, n, d, dff = _listenc_shapes(X, pad, weights, heads)
    if dY.shape != X.shape:
        raise ValueError(f"listenc_block_bwd: dY must be {tuple(X.shape)}, got {tuple(dY.shape)}")
    dev, f32 = X.device, torch.float32
    ws = (workspace if workspace is not None else ListEncWorkspace()).get(B, n, d, heads, dff, dev)
    dX = torch.empty(X.shape, dtype=f32, device=dev)
    grads = [torch.empty(tuple(W.shape), dtype=f32, device=dev) for W in weights]
    _lib.call("rc_listenc_block_bwd", _ptr(dY, f32, "dY"), _ptr(X, f32, "X"), _ptr(pad, torch.uint8, "pad"),
              *[_ptr(W, f32, k) for k, W in zip(LISTENC_WEIGHTS, weights)], B, n, d, int(heads), dff, C.c_void_p(ws.data_ptr()), ws.numel(),
              _ptr(dX, f32, "dX"), *[_ptr(G, f32, "d" + k) for k, G in zip(LISTENC_WEIGHTS, grads)], _stream())
    return dX, grads


# ---- set attention block (models/reranker/SetRank.py:29-56 `MAB`: query rows that are not the key rows) -----------------------------

def setmab_check_shape(nq, nk, d, heads, d_ff):
    """rc_setmab_check_shape (host logic): 1 <= nq, nk <= 64, d, heads and d_ff as listenc_check_shape has them, and both row sets
    with the backward's intermediates within the LDS; raises ValueError with the library's reason otherwise"""
    _check_shape("set attention block", "rc_setmab_check_shape", nq, nk, d, heads, d_ff)


class SetMabWorkspace(_ShapeWorkspace):
    """the scratch of rc_setmab_bwd (the per-workgroup partials of the weight gradients and of a shared query source's gradient), one
    buffer per shape that is never freed or moved while the owner lives: a captured training step replays on the same memory.
    Nothing in it outlives the call that wrote it, so both blocks of every induced block of a stack share one workspace."""
    _query, _shape, _floor = "rc_setmab_bwd_workspace_bytes", ("B", "nq", "nk", "d", "heads", "d_ff"), 256


def _setmab_shapes(Qs, Ks, pad, weights, heads, shared_q):
    if Ks.dim() != 3 or Ks.numel() == 0:
        raise ValueError(f"set_attention_block: Ks must be [lists, key rows, width] with at least one list, got {tuple(Ks.shape)}")
    B, nk, d = Ks.shape
    if Qs.dim() != (2 if shared_q else 3) or Qs.numel() == 0 or Qs.shape[-1] != d or (not shared_q and Qs.shape[0] != B):
        raise ValueError(f"set_attention_block: Qs must be {'[query rows, ' if shared_q else f'[{B}, query rows, '}{d}], "
                         f"got {tuple(Qs.shape)} (shared_q={bool(shared_q)})")
    nq = Qs.shape[-2]
    if pad is not None and tuple(pad.shape) != (B, nk):
        raise ValueError(f"set_attention_block: pad must be [{B}, {nk}] or None, got {tuple(pad.shape)}")
    if len(weights) != len(LISTENC_WEIGHTS):
        raise ValueError(f"set_attention_block: twelve weights are needed ({', '.join(LISTENC_WEIGHTS)})")
    W1 = weights[6]
    if W1.dim() != 2 or W1.shape[1] != d:
        raise ValueError(f"set_attention_block: W1 must be [d_ff, {d}], got {tuple(W1.shape)}")
    dff = W1.shape[0]
    setmab_check_shape(nq, nk, d, heads, dff)
    shapes = ((3 * d, d), (3 * d,), (d, d), (d,), (d,), (d,), (dff, d), (dff,), (d, dff), (d,), (d,), (d,))
    for name, W, shape in zip(LISTENC_WEIGHTS, weights, shapes):
        if tuple(W.shape) != shape:
            raise ValueError(f"set_attention_block: {name} must be {list(shape)}, got {tuple(W.shape)}")
    return B, nq, nk, d, dff


def setmab_fwd(Qs, Ks, pad, weights, heads, shared_q=False):
    """rc_setmab_fwd: Y [B, nq, d] = LN2(X1 + relu(X1 W1^T + b1) W2^T + b2), X1 = LN1(Qs + MHA(Qs, Ks, Ks; pad)), one launch.
    Qs [B, nq, d], or [nq, d] with shared_q (one query source for every list); pad uint8 [B, nk], 1 = padded key, or None;
    weights in LISTENC_WEIGHTS order"""
    B, nq, nk, d, dff = _setmab_shapes(Qs, Ks, pad, weights, heads, shared_q)
    f32 = torch.float32
    Y = torch.empty((B, nq, d), dtype=f32, device=Ks.device)
    _lib.call("rc_setmab_fwd", _ptr(Qs, f32, "Qs"), _ptr(Ks, f32, "Ks"), _ptr(pad, torch.uint8, "pad", allow_none=True),
              *[_ptr(W, f32, k) for k, W in zip(LISTENC_WEIGHTS, weights)], B, nq, nk, d, int(heads), dff, int(bool(shared_q)),
              _ptr(Y, f32, "Y"), _stream())
    return Y


def setmab_bwd(dY, Qs, Ks, pad, weights, heads, shared_q=False, workspace=None):
    """rc_setmab_bwd -> (dQs, dKs, [the twelve gradients in LISTENC_WEIGHTS order]): the block is recomputed from Qs and Ks; dQs has
    Qs's shape (with shared_q: the sum over all lists); two launches, three with shared_q"""
    B, nq, nk, d, dff = _setmab_shapes(Qs, Ks, pad, weights, heads, shared_q)
    if tuple(dY.shape) != (B, nq, d):
        raise ValueError(f"setmab_bwd: dY must be {(B, nq, d)}, got {tuple(dY.shape)}")
    dev, f32 = Ks.device, torch.float32
    ws = (workspace if workspace is not None else SetMabWorkspace()).get(B, nq, nk, d, heads, dff, dev)
    dQs = torch.empty(Qs.shape, dtype=f32, device=dev)
    dKs = torch.empty(Ks.shape, dtype=f32, device=dev)
    grads = [torch.empty(tuple(W.shape), dtype=f32, device=dev) for W in weights]
    _lib.call("rc_setmab_bwd", _ptr(dY, f32, "dY"), _ptr(Qs, f32, "Qs"), _ptr(Ks, f32, "Ks"), _ptr(pad, torch.uint8, "pad", allow_none=True),
              *[_ptr(W, f32, k) for k, W in zip(LISTENC_WEIGHTS, weights)], B, nq, nk, d, int(heads), dff, int(bool(shared_q)),
              C.c_void_p(ws.data_ptr()), ws.numel(), _ptr(dQs, f32, "dQs"), _ptr(dKs, f32, "dKs"),
              *[_ptr(G, f32, "d" + k) for k, G in zip(LISTENC_WEIGHTS, grads)], _stream())
    return dQs, dKs, grads


# ---- FinalMLP: feature gates + first stream layers, bilinear fusion (models/context/FinalMLP.py:141-249) -------------------------------

def finalmlp_check_shape(n_fields, emb_size, gate_in_1, first_1, gate_in_2, first_2, x_dim, y_dim, num_heads, drop_p_1=0.0, drop_p_2=0.0):
    """rc_finalmlp_check_shape (host logic): 3 <= fields <= 32, emb_size % 4 == 0 in [4, 128], gate inputs / first-layer widths / stream
    outputs multiples of 4 in [4, 256], num_heads a divisor of both stream outputs, dropout in [0, 1), a 32-row tile within the LDS;
    raises ValueError with the library's reason otherwise"""
    _check_shape("FinalMLP", "rc_finalmlp_check_shape", n_fields, emb_size, gate_in_1, first_1, gate_in_2, first_2, x_dim, y_dim, num_heads,
                 extra=(float(drop_p_1), float(drop_p_2)))


def finalmlp_fusion_check_shape(x_dim, y_dim, num_heads):
    """the fusion kernels' own envelope (what a model without the feature gates needs): stream outputs multiples of 4 in [4, 256],
    num_heads a divisor of both; raises ValueError with the library's reason otherwise"""
    lib = _lib.load()
    if lib.rc_finalmlp_fusion_workspace_bytes(1, int(x_dim), int(y_dim), int(num_heads)) == 0:
        raise ValueError("FinalMLP on the HIP engine: " + lib.rc_last_error_string().decode())


class FinalMLPWorkspace(_ShapeWorkspace):
    """the scratch of rc_finalmlp_gate_bwd and rc_finalmlp_fusion_bwd (per-workgroup partials, the per-slab shares of dZin), one buffer
    per call kind and shape that is never freed or moved while the owner lives: a captured training step replays on the same memory"""
    _query, _floor = {"gate": "rc_finalmlp_gate_workspace_bytes", "fusion": "rc_finalmlp_fusion_workspace_bytes"}, 256

    def get(self, kind, key, device):
        """key: the arguments of the kind's size query"""
        key = tuple(int(k) for k in key)
        return self._buffer(self._query[kind], (kind,) + key, key, device)


def _finalmlp_stream(X, n_cand, stream, which, need_seed=True):
    """(struct rc_finalmlp_stream, shapes) of stream = (Zin, Wg, bg, W, b, drop_p, seed, site); every shape and dtype checked here"""
    Zin, Wg, bg, W, b, drop_p, seed, site = stream
    N, D = X.shape
    f32 = torch.float32
    if Zin.dim() != 2 or Zin.shape[0] not in (1, N // n_cand, N):
        raise ValueError(f"finalmlp_gate: the gate input of stream {which} must be [1 | {N // n_cand} | {N}, G], got {tuple(Zin.shape)}")
    G, H = Zin.shape[1], W.shape[0]
    if Wg.shape != (D, G) or bg.shape != (D,):
        raise ValueError(f"finalmlp_gate: the gate's last Linear of stream {which} must be [{D}, {G}] + [{D}], got {tuple(Wg.shape)} + {tuple(bg.shape)}")
    if W.shape != (H, D) or b.shape != (H,):
        raise ValueError(f"finalmlp_gate: the first layer of stream {which} must be [H, {D}] + [H], got {tuple(W.shape)} + {tuple(b.shape)}")
    drop_p = float(drop_p)
    if not 0.0 <= drop_p < 1.0 or (need_seed and drop_p > 0.0 and seed is None):
        raise ValueError(f"finalmlp_gate: dropout p={drop_p} of stream {which} needs p in [0, 1) and a device seed")
    st = _lib.FinalMlpStream(_ptr(Zin, f32, "Zin").value, _ptr(Wg, f32, "Wg").value, _ptr(bg, f32, "bg").value, _ptr(W, f32, "W").value,
                             _ptr(b, f32, "b").value, _ptr(seed, torch.int64, "seed").value if (drop_p > 0.0 and need_seed) else None,
                             Zin.shape[0], G, H, drop_p, int(site))
    return st, G, H


def _finalmlp_x(X, n_cand):
    if X.dim() != 2 or X.shape[0] < 1 or n_cand < 1 or X.shape[0] % n_cand != 0:
        raise ValueError(f"finalmlp_gate: X must be [instances, fields * emb_size] with whole candidate lists of {n_cand}, got {tuple(X.shape)}")
    return X.shape


def finalmlp_gate_fwd(X, n_cand, stream1, stream2):
    """rc_finalmlp_gate_fwd -> (A1 [N, H1], A2 [N, H2]): A_s = drop(relu((X * 2 sigmoid(Zin_s Wg_s^T + bg_s)) W_s^T + b_s)), one launch.
    stream = (Zin [1 | N / n_cand | N, G], Wg [D, G], bg [D], W [H, D], b [H], drop_p, seed | None, site)"""
    N, D = _finalmlp_x(X, n_cand)
    s1, _, H1 = _finalmlp_stream(X, n_cand, stream1, 1)
    s2, _, H2 = _finalmlp_stream(X, n_cand, stream2, 2)
    f32 = torch.float32
    A1 = torch.empty((N, H1), dtype=f32, device=X.device)
    A2 = torch.empty((N, H2), dtype=f32, device=X.device)
    _lib.call("rc_finalmlp_gate_fwd", _ptr(X, f32, "X"), N, int(n_cand), D, C.byref(s1), C.byref(s2), _ptr(A1, f32, "A1"),
              _ptr(A2, f32, "A2"), _stream())
    return A1, A2


def finalmlp_gate_bwd(X, n_cand, stream1, stream2, A1, dA1, A2, dA2, workspace=None):
    """rc_finalmlp_gate_bwd -> (dX, (dZin, dWg, dbg, dW, db) of stream 1, the same of stream 2); the gates are recomputed"""
    N, D = _finalmlp_x(X, n_cand)
    s1, G1, H1 = _finalmlp_stream(X, n_cand, stream1, 1, need_seed=False)      # (the saved A is the mask: nothing is drawn)
    s2, G2, H2 = _finalmlp_stream(X, n_cand, stream2, 2, need_seed=False)
    for name, t, H in (("A1", A1, H1), ("dA1", dA1, H1), ("A2", A2, H2), ("dA2", dA2, H2)):
        if t.shape != (N, H):
            raise ValueError(f"finalmlp_gate_bwd: {name} must be [{N}, {H}], got {tuple(t.shape)}")
    dev, f32 = X.device, torch.float32
    ws = (workspace if workspace is not None else FinalMLPWorkspace()).get(
        "gate", (N, n_cand, D, G1, H1, stream1[0].shape[0], G2, H2, stream2[0].shape[0]), dev)
    dX = torch.empty_like(X)
    grads, structs = [], []
    for stream in (stream1, stream2):
        g = tuple(torch.empty_like(t) for t in stream[:5])
        grads.append(g)
        structs.append(_lib.FinalMlpGrads(*[_ptr(t, f32, "grad").value for t in g]))
    _lib.call("rc_finalmlp_gate_bwd", _ptr(X, f32, "X"), N, int(n_cand), D, C.byref(s1), C.byref(s2), _ptr(A1, f32, "A1"),
              _ptr(dA1, f32, "dA1"), _ptr(A2, f32, "A2"), _ptr(dA2, f32, "dA2"), C.c_void_p(ws.data_ptr()), ws.numel(),
              _ptr(dX, f32, "dX"), C.byref(structs[0]), C.byref(structs[1]), _stream())
    return dX, grads[0], grads[1]


def _finalmlp_fusion_shapes(x, y, w_xy, w_x, w_y, heads):
    if x.dim() != 2 or y.dim() != 2 or x.shape[0] != y.shape[0] or x.shape[0] < 1:
        raise ValueError(f"finalmlp_fusion: x and y must be [instances, width] with the same instances, got {tuple(x.shape)} / {tuple(y.shape)}")
    N, H1 = x.shape
    H2 = y.shape[1]
    lib = _lib.load()
    if lib.rc_finalmlp_fusion_workspace_bytes(N, H1, H2, int(heads)) == 0:
        raise ValueError("FinalMLP on the HIP engine: " + lib.rc_last_error_string().decode())
    if w_xy.numel() != H1 * H2 // heads or w_x.numel() != H1 or w_y.numel() != H2:
        raise ValueError(f"finalmlp_fusion: w_xy / w_x / w_y must hold {H1 * H2 // heads} / {H1} / {H2} elements, got {w_xy.numel()} / "
                         f"{w_x.numel()} / {w_y.numel()}")
    return N, H1, H2


def finalmlp_fusion_fwd(x, y, w_xy, w_x, b_x, w_y, b_y, heads):
    """rc_finalmlp_fusion_fwd -> out [N] = w_x x + b_x + w_y y + b_y + sum_h x_h^T W_h y_h, one launch, nothing saved"""
    N, H1, H2 = _finalmlp_fusion_shapes(x, y, w_xy, w_x, w_y, heads)
    if b_x.numel() != 1 or b_y.numel() != 1:
        raise ValueError("finalmlp_fusion: b_x and b_y hold one element each")
    f32 = torch.float32
    out = torch.empty(N, dtype=f32, device=x.device)
    _lib.call("rc_finalmlp_fusion_fwd", _ptr(x, f32, "x"), _ptr(y, f32, "y"), _ptr(w_xy, f32, "w_xy"), _ptr(w_x, f32, "w_x"),
              _ptr(b_x, f32, "b_x"), _ptr(w_y, f32, "w_y"), _ptr(b_y, f32, "b_y"), N, H1, H2, int(heads), _ptr(out, f32, "out"), _stream())
    return out


def finalmlp_fusion_bwd(x, y, w_xy, w_x, w_y, dout, heads, workspace=None):
    """rc_finalmlp_fusion_bwd -> (dx, dy, dw_xy, dw_x, db_x, dw_y, db_y), shaped like their parameters (biases [1])"""
    N, H1, H2 = _finalmlp_fusion_shapes(x, y, w_xy, w_x, w_y, heads)
    if dout.shape != (N,):
        raise ValueError(f"finalmlp_fusion_bwd: dout must be [{N}], got {tuple(dout.shape)}")
    dev, f32 = x.device, torch.float32
    ws = (workspace if workspace is not None else FinalMLPWorkspace()).get("fusion", (N, H1, H2, heads), dev)
    dx, dy = torch.empty_like(x), torch.empty_like(y)
    dw_xy, dw_x, dw_y = torch.empty_like(w_xy), torch.empty_like(w_x), torch.empty_like(w_y)
    db_x, db_y = torch.empty(1, dtype=f32, device=dev), torch.empty(1, dtype=f32, device=dev)
    _lib.call("rc_finalmlp_fusion_bwd", _ptr(x, f32, "x"), _ptr(y, f32, "y"), _ptr(w_xy, f32, "w_xy"), _ptr(w_x, f32, "w_x"),
              _ptr(w_y, f32, "w_y"), _ptr(dout, f32, "dout"), N, H1, H2, int(heads), C.c_void_p(ws.data_ptr()), ws.numel(),
              _ptr(dx, f32, "dx"), _ptr(dy, f32, "dy"), _ptr(dw_xy, f32, "dw_xy"), _ptr(dw_x, f32, "dw_x"), _ptr(db_x, f32, "db_x"),
              _ptr(dw_y, f32, "dw_y"), _ptr(db_y, f32, "db_y"), _stream())
    return dx, dy, dw_xy, dw_x, db_x, dw_y, db_y


# ---- FPMC: pair-table scores, fused BPR step, item-side pair update (models/sequential/FPMC.py:44-56) -----------------------------

def fpmc_check_shape(d, n_cand=1):
    """rc_fpmc_check_shape (host logic): emb_size in {16, 32, 64, 128}, at least one candidate; raises ValueError with the library's
    reason otherwise"""
    _check_shape("FPMC", "rc_fpmc_check_shape", d, n_cand)


def fpmc_fwd_bwd_layout(d, n_cand):
    """the path rc_fpmc_fwd_bwd takes for (d, C): (lane-groups per tuple, candidate pair rows per lane-group) on the register path,
    None on the streaming path (rc_fpmc_fwd_bwd_layout, host logic)"""
    code = int(_lib.load().rc_fpmc_fwd_bwd_layout(int(d), int(n_cand)))
    return (code // 256, code % 256) if code else None


def _fpmc_shapes(UI, LI, IU, IL, uid, lid, iid):
    d = UI.shape[1]
    if not (LI.shape[1] == IU.shape[1] == IL.shape[1] == d):
        raise ValueError("FPMC: the four tables need the same emb_size")
    if not (LI.shape[0] == IU.shape[0] == IL.shape[0]):
        raise ValueError("FPMC: li, iu and il embeddings are indexed by item ids and need the same number of rows")
    if iid.dim() != 2 or uid.shape != (iid.shape[0],) or lid.shape != (iid.shape[0],):
        raise ValueError(f"FPMC: ids must be uid [B], lid [B], iid [B, C]; got {tuple(uid.shape)}, {tuple(lid.shape)}, {tuple(iid.shape)}")
    return iid.shape[0], iid.shape[1], d


def _fpmc_front_args(UI, LI, IU, IL, uid, lid, iid):
    f32, i64 = torch.float32, torch.int64
    return (_ptr(UI, f32, "UI"), _ptr(LI, f32, "LI"), _ptr(IU, f32, "IU"), _ptr(IL, f32, "IL"), _ptr(uid, i64, "uid"),
            _ptr(lid, i64, "lid"), _ptr(iid, i64, "iid"))


def fpmc_scores(UI, LI, IU, IL, uid, lid, iid):
    """pred[b, c] = <UI[uid[b]], IU[iid[b, c]]> + <LI[lid[b]], IL[iid[b, c]]>, any C >= 1 (rc_fpmc_scores)"""
    B, Cn, d = _fpmc_shapes(UI, LI, IU, IL, uid, lid, iid)
    pred = torch.empty((B, Cn), dtype=torch.float32, device=UI.device)
    _lib.call("rc_fpmc_scores", *_fpmc_front_args(UI, LI, IU, IL, uid, lid, iid), B, Cn, d, _ptr(pred, torch.float32, "pred"), _stream())
    return pred


def fpmc_fwd_bwd(UI, LI, IU, IL, uid, lid, iid, inv_b=None, want_pred=True):
    """rc_fpmc_fwd_bwd: scores + GeneralModel.loss + backward to the query rows in one launch.
    Returns (pred|None, loss_vec [B], gpred [B, C], ugrad [B, d], lgrad [B, d])."""
    B, Cn, d = _fpmc_shapes(UI, LI, IU, IL, uid, lid, iid)
    if inv_b is None:
        inv_b = 1.0 / B
    dev, f32 = UI.device, torch.float32
    pred, loss_vec, gpred = _step_outputs(B, Cn, dev, want_pred)
    ugrad = torch.empty((B, d), dtype=f32, device=dev)
    lgrad = torch.empty((B, d), dtype=f32, device=dev)
    _lib.call("rc_fpmc_fwd_bwd", *_fpmc_front_args(UI, LI, IU, IL, uid, lid, iid), B, Cn, d, float(inv_b),
              _ptr(pred, f32, "pred", True), _ptr(loss_vec, f32, "loss_vec"), _ptr(gpred, f32, "gpred"), _ptr(ugrad, f32, "ugrad"),
              _ptr(lgrad, f32, "lgrad"), _stream())
    return pred, loss_vec, gpred, ugrad, lgrad


def fpmc_item_update(keys, perm, heads, n_heads, gpred, UI, LI, uid, lid, hyper=None, IU=None, IL=None, m=(None, None), v=(None, None),
                     dense_grad=(None, None)):
    """rc_fpmc_item_update: one pass over the sorted candidate ids (keys / perm of sort_ids(iid), heads / n_heads of segment_heads)
    that sums gpred[o] * UI[uid[o / C]] and gpred[o] * LI[lid[o / C]] per distinct candidate row and either applies `hyper` to rows
    of IU / IL (m, v: (state of IU, state of IL)) in place or writes dense_grad = (dense .grad of IU, of IL); gpred [B, C]"""
    n_occ = keys.numel()
    d = UI.shape[1]
    Cn = gpred.shape[-1]
    f32, i32 = torch.float32, torch.int32
    ws = workspace(_lib.load().rc_fpmc_item_update_workspace_bytes(n_occ, d), keys.device, "fpmc_item")
    _lib.call("rc_fpmc_item_update", _ptr(IU, f32, "IU", True), _ptr(m[0], f32, "mIU", True), _ptr(v[0], f32, "vIU", True),
              _ptr(IL, f32, "IL", True), _ptr(m[1], f32, "mIL", True), _ptr(v[1], f32, "vIL", True), d, _ptr(keys, i32, "keys"),
              _ptr(perm, i32, "perm"), n_occ, _ptr(gpred, f32, "gpred"), _ptr(UI, f32, "UI"), _ptr(LI, f32, "LI"),
              _ptr(uid, torch.int64, "uid"), _ptr(lid, torch.int64, "lid"), Cn, _hyper_ref(hyper),
              _ptr(dense_grad[0], f32, "dense_grad_iu", True), _ptr(dense_grad[1], f32, "dense_grad_il", True),
              _ptr(heads, i32, "heads"), _ptr(n_heads, i32, "n_heads"), *_ws_args(ws))


class _RowwiseTrainer:
    """What the row-wise trainers share: the optimizers their step covers, the hyper record `hyper` (step() counts its step), the
    parameter tensors by name in `P` and the optimizer state of each in `state[name]` (new_opt_state)."""

    def __init__(self, opt, lr, l2, beta1, beta2, eps):
        if opt not in ("SGD", "Adam", "Adagrad"):
            raise ValueError(f"{type(self).__name__}: the row-wise step covers SGD, Adam and Adagrad, not {opt!r}")
        self.opt = opt
        self.hyper = make_hyper(opt, lr, l2, beta1, beta2, eps, step=0)

    def _new_state(self):
        """fresh optimizer state for every tensor of P (after the subclass has checked the shapes: a refused one allocates nothing)"""
        self.state = {name: new_opt_state(t, self.opt) for name, t in self.P.items()}

    def _mv(self, name):
        return self.state[name].get("m"), self.state[name].get("v")

    def _tables(self, names):
        """(W list, m list | None, v list | None) of the named tables, as the entry points with pointer arrays take them: an
        optimizer without that state passes NULL for the whole array"""
        mv = [self._mv(k) for k in names]
        m, v = ([x[j] for x in mv] if mv[0][j] is not None else None for j in (0, 1))
        return [self.P[k] for k in names], m, v


class FpmcTrainer(_RowwiseTrainer):
    """Row-wise-optimizer FPMC training on the device tables UI [n_users, d], LI / IU / IL [n_items, d] (ui_embeddings, li_embeddings,
    iu_embeddings, il_embeddings of models/sequential/FPMC.py:36-39).

    One `step(uid, lid, iid)` = one iteration of BaseRunner.fit's batch loop (helpers/BaseRunner.py:193-206): two sorts + the head
    list -> rc_fpmc_fwd_bwd -> rc_fpmc_item_update (reads the pre-step UI / LI) -> the two query-side rc_segmented_update.  Only rows
    of the batch move (and only their optimizer state): the row-wise semantics of BprmfTrainer."""

    def __init__(self, UI, LI, IU, IL, opt="SGD", lr=1e-3, l2=0.0, beta1=0.9, beta2=0.999, eps=None):
        super().__init__(opt, lr, l2, beta1, beta2, eps)
        self.UI, self.LI, self.IU, self.IL = UI, LI, IU, IL
        self.P = {"UI": UI, "LI": LI, "IU": IU, "IL": IL}
        self.d = UI.shape[1]
        fpmc_check_shape(self.d)
        self._new_state()

    def step(self, uid, lid, iid, inv_b=None):
        """one training step; returns the device loss tensor (shape [1], no sync)"""
        B, Cn, d = _fpmc_shapes(self.UI, self.LI, self.IU, self.IL, uid, lid, iid)
        if inv_b is None:
            inv_b = 1.0 / B
        n_users, n_items = self.UI.shape[0], self.IU.shape[0]
        self.hyper.step += 1
        # candidates on their own; users + last items jointly (last items keyed behind the users)
        ikeys, iperm = sort_ids(iid, n_items)
        _, heads, n_heads = segment_heads(ikeys, iperm, want_single=False)
        qkeys, qperm = sort_ids(uid, n_users + n_items, lid, n_users)
        _, loss_vec, gpred, ugrad, lgrad = fpmc_fwd_bwd(self.UI, self.LI, self.IU, self.IL, uid, lid, iid, inv_b, want_pred=False)
        loss = reduce_sum(loss_vec, inv_b)
        mIU, vIU = self._mv("IU")
        mIL, vIL = self._mv("IL")
        fpmc_item_update(ikeys, iperm, heads, n_heads, gpred, self.UI, self.LI, uid, lid, hyper=self.hyper, IU=self.IU, IL=self.IL,
                         m=(mIU, mIL), v=(vIU, vIL))
        # the query side last: the item-side update above read the pre-step UI and LI.  Plain gradient rows, one per occurrence;
        # each table takes its half of the joint sort, LI's keyed behind the users and numbered behind their occurrences
        m, v = self._mv("UI")
        segmented_update(qkeys[:B], qperm[:B], ugrad, hyper=self.hyper, W=self.UI, m=m, v=v)
        m, v = self._mv("LI")
        segmented_update(qkeys[B:], qperm[B:], lgrad, hyper=self.hyper, W=self.LI, m=m, v=v, key_base=n_users, occ_base=B)
        return loss


# ---- SLRC+: biased MF + Hawkes excitation, fused BPR step, seven-table item update (models/sequential/SLRCPlus.py:62-89) ----------

SLRC_PARAMS = ("U", "I", "user_bias", "item_bias", "global_alpha", "alphas", "pis", "betas", "sigmas", "mus")   # the argument order
SLRC_ITEM_TABLES = ("I", "item_bias", "alphas", "pis", "betas", "sigmas", "mus")   # the [7] arrays of rc_slrc_item_update


def slrc_check_shape(d, n_cand=1, n_rel=1):
    """rc_slrc_check_shape (host logic): emb_size in {16, 32, 64, 128}, at least one candidate, 1..8 relations; raises ValueError
    with the library's reason otherwise"""
    _check_shape("SLRCPlus", "rc_slrc_check_shape", d, n_cand, n_rel)


def slrc_fwd_bwd_layout(d, n_cand, n_rel=1):
    """the path rc_slrc_fwd_bwd takes for (d, C, R): the candidate rows per lane-group on the register path, None on the
    streaming path (rc_slrc_fwd_bwd_layout, host logic)"""
    return int(_lib.load().rc_slrc_fwd_bwd_layout(int(d), int(n_cand), int(n_rel))) or None


def _slrc_shapes(P, uid, iid, intervals):
    U, I, ub, ib, ga, *H = P
    d, n_users, n_items = U.shape[1], U.shape[0], I.shape[0]
    R = H[0].shape[1]
    if I.shape[1] != d:
        raise ValueError("SLRCPlus: u_embeddings and i_embeddings need the same emb_size")
    if ub.numel() != n_users or ib.numel() != n_items or ga.numel() != 1:
        raise ValueError("SLRCPlus: user_bias [n_users, 1], item_bias [n_items, 1] and a scalar global_alpha are needed")
    if any(tuple(h.shape) != (n_items, R) for h in H):
        raise ValueError("SLRCPlus: alphas, pis, betas, sigmas and mus must all be [n_items, relation_num]")
    if iid.dim() != 2 or uid.shape != (iid.shape[0],) or tuple(intervals.shape) != (iid.shape[0], iid.shape[1], R):
        raise ValueError(f"SLRCPlus: need uid [B], iid [B, C], relational_interval [B, C, {R}]; got {tuple(uid.shape)}, "
                         f"{tuple(iid.shape)}, {tuple(intervals.shape)}")
    return iid.shape[0], iid.shape[1], d, R


def _slrc_front_args(P, uid, iid, intervals):
    f32, i64 = torch.float32, torch.int64
    return tuple(_ptr(t, f32, name) for t, name in zip(P, SLRC_PARAMS)) + (
        _ptr(uid, i64, "uid"), _ptr(iid, i64, "iid"), _ptr(intervals, f32, "relational_interval"))


def slrc_scores(P, uid, iid, intervals):
    """SLRC+'s prediction [B, C] for any C >= 1 (rc_slrc_scores); P: the ten parameter tensors in SLRC_PARAMS order"""
    B, Cn, d, R = _slrc_shapes(P, uid, iid, intervals)
    pred = torch.empty((B, Cn), dtype=torch.float32, device=iid.device)
    _lib.call("rc_slrc_scores", *_slrc_front_args(P, uid, iid, intervals), B, Cn, d, R, _ptr(pred, torch.float32, "pred"), _stream())
    return pred


def slrc_fwd_bwd(P, uid, iid, intervals, inv_b=None, want_pred=True):
    """rc_slrc_fwd_bwd: scores + GeneralModel.loss + backward in one launch.
    Returns (pred|None, loss_vec [B], gpred [B, C], ugrad [B, d], ubgrad [B], hgrad [B * C, 5 R], gagrad [B])."""
    B, Cn, d, R = _slrc_shapes(P, uid, iid, intervals)
    if inv_b is None:
        inv_b = 1.0 / B
    dev, f32 = iid.device, torch.float32
    pred, loss_vec, gpred = _step_outputs(B, Cn, dev, want_pred)
    ugrad = torch.empty((B, d), dtype=f32, device=dev)
    ubgrad = torch.empty(B, dtype=f32, device=dev)
    hgrad = torch.empty((B * Cn, 5 * R), dtype=f32, device=dev)
    gagrad = torch.empty(B, dtype=f32, device=dev)
    _lib.call("rc_slrc_fwd_bwd", *_slrc_front_args(P, uid, iid, intervals), B, Cn, d, R, float(inv_b), _ptr(pred, f32, "pred", True),
              _ptr(loss_vec, f32, "loss_vec"), _ptr(gpred, f32, "gpred"), _ptr(ugrad, f32, "ugrad"), _ptr(ubgrad, f32, "ubgrad"),
              _ptr(hgrad, f32, "hgrad"), _ptr(gagrad, f32, "gagrad"), _stream())
    return pred, loss_vec, gpred, ugrad, ubgrad, hgrad, gagrad


def slrc_excitation_grads(P, uid, iid, intervals, gpred):
    """rc_slrc_excitation_bwd: for a given gpred [B, C] -> (hgrad [B * C, 5 R], ubgrad [B], gagrad [B]) as slrc_fwd_bwd returns them"""
    B, Cn, d, R = _slrc_shapes(P, uid, iid, intervals)
    dev, f32 = iid.device, torch.float32
    hgrad = torch.empty((B * Cn, 5 * R), dtype=f32, device=dev)
    ubgrad = torch.empty(B, dtype=f32, device=dev)
    gagrad = torch.empty(B, dtype=f32, device=dev)
    _lib.call("rc_slrc_excitation_bwd", *(_ptr(t, f32, name) for t, name in zip(P[4:], SLRC_PARAMS[4:])), _ptr(iid, torch.int64, "iid"),
              _ptr(intervals, f32, "relational_interval"), _ptr(gpred, f32, "gpred"), B, Cn, R, _ptr(hgrad, f32, "hgrad"),
              _ptr(ubgrad, f32, "ubgrad"), _ptr(gagrad, f32, "gagrad"), _stream())
    return hgrad, ubgrad, gagrad


_NUMBER_WORDS = {3: "three", 7: "seven"}      # the lengths of CHORUS_CAT_TABLES and SLRC_ITEM_TABLES


def _ptr_array(tensors, names, what, allow_none=False):
    """a host array of the device pointers of one float tensor per name (in the order of `names`), or NULL when `tensors` is None"""
    if tensors is None:
        return None
    n = len(names)
    if len(tensors) != n:
        raise ValueError(f"{what}: {_NUMBER_WORDS[n]} tensors are needed ({', '.join(names)})")
    return (C.c_void_p * n)(*(_ptr(t, torch.float32, f"{what}[{k}]", allow_none) for t, k in zip(tensors, names)))


def slrc_item_update(keys, perm, heads, n_heads, gpred, hgrad, U, uid, hyper=None, W=None, m=None, v=None, dense_grad=None):
    """rc_slrc_item_update: one pass over the sorted candidate ids (keys / perm of sort_ids(iid), heads / n_heads of segment_heads)
    that sums gpred[o] * U[uid[o / C]], gpred[o] and hgrad[o] per distinct candidate row and either applies `hyper` to that row of
    the seven item tables W (m, v: their states; SLRC_ITEM_TABLES order; item_bias with l2 = 0) in place or writes the seven
    dense gradients; gpred [B, C], hgrad [B * C, 5 R]"""
    n_occ = keys.numel()
    d = U.shape[1]
    Cn = gpred.shape[-1]
    R = hgrad.shape[-1] // 5
    f32, i32 = torch.float32, torch.int32
    ws = workspace(_lib.load().rc_slrc_item_update_workspace_bytes(n_occ, d), keys.device, "slrc_item")
    T = SLRC_ITEM_TABLES
    _lib.call("rc_slrc_item_update", _ptr_array(W, T, "W"), _ptr_array(m, T, "m", True), _ptr_array(v, T, "v", True), d, R,
              _ptr(keys, i32, "keys"), _ptr(perm, i32, "perm"), n_occ, _ptr(gpred, f32, "gpred"), _ptr(hgrad, f32, "hgrad"),
              _ptr(U, f32, "U"), _ptr(uid, torch.int64, "uid"), Cn, _hyper_ref(hyper), _ptr_array(dense_grad, T, "dense_grad"),
              _ptr(heads, i32, "heads"), _ptr(n_heads, i32, "n_heads"), *_ws_args(ws))


def slrc_user_bias_update(keys, perm, ubgrad, hyper=None, user_bias=None, m=None, v=None, dense_grad=None):
    """rc_slrc_user_bias_update: per distinct user of the sorted uid list the sum of ubgrad over its tuples, then `hyper` on
    user_bias (one float per row, l2 forced to 0) in place, or the dense gradient"""
    f32, i32 = torch.float32, torch.int32
    _lib.call("rc_slrc_user_bias_update", _ptr(user_bias, f32, "user_bias", True), _ptr(m, f32, "m", True), _ptr(v, f32, "v", True),
              _ptr(keys, i32, "keys"), _ptr(perm, i32, "perm"), keys.numel(), _ptr(ubgrad, f32, "ubgrad"), _hyper_ref(hyper),
              _ptr(dense_grad, f32, "dense_grad", True), _stream())


class SlrcTrainer(_RowwiseTrainer):
    """Row-wise-optimizer SLRC+ training on the ten device parameters (SLRC_PARAMS order; models/sequential/SLRCPlus.py:49-60).

    One `step(uid, iid, intervals)` = one iteration of BaseRunner.fit's batch loop (helpers/BaseRunner.py:193-206): two sorts + the
    head list -> rc_slrc_fwd_bwd -> rc_slrc_item_update (reads the pre-step U) -> rc_segmented_update on U, rc_slrc_user_bias_update,
    rc_dense_update on global_alpha.  Only rows of the batch move (and only their optimizer state): the row-wise semantics of
    BprmfTrainer; the two bias tables take no weight decay, global_alpha (dense, one float) does."""

    def __init__(self, *params, opt="SGD", lr=1e-3, l2=0.0, beta1=0.9, beta2=0.999, eps=None):
        super().__init__(opt, lr, l2, beta1, beta2, eps)
        if len(params) != len(SLRC_PARAMS):
            raise ValueError("SlrcTrainer: ten parameter tensors are needed: " + ", ".join(SLRC_PARAMS))
        self.P = dict(zip(SLRC_PARAMS, params))
        self.d, self.R = self.P["U"].shape[1], self.P["alphas"].shape[1]
        slrc_check_shape(self.d, 1, self.R)
        self._new_state()

    def step(self, uid, iid, intervals, inv_b=None):
        """one training step; returns the device loss tensor (shape [1], no sync)"""
        P = [self.P[k] for k in SLRC_PARAMS]
        B, Cn, d, R = _slrc_shapes(P, uid, iid, intervals)
        if inv_b is None:
            inv_b = 1.0 / B
        U = self.P["U"]
        self.hyper.step += 1
        ikeys, iperm = sort_ids(iid, self.P["I"].shape[0])
        _, heads, n_heads = segment_heads(ikeys, iperm, want_single=False)
        ukeys, uperm = sort_ids(uid, U.shape[0])
        _, loss_vec, gpred, ugrad, ubgrad, hgrad, gagrad = slrc_fwd_bwd(P, uid, iid, intervals, inv_b, want_pred=False)
        loss = reduce_sum(loss_vec, inv_b)
        W, m, v = self._tables(SLRC_ITEM_TABLES)
        slrc_item_update(ikeys, iperm, heads, n_heads, gpred, hgrad, U, uid, hyper=self.hyper, W=W, m=m, v=v)
        # the user side last: the item-side update above read the pre-step U
        m, v = self._mv("U")
        segmented_update(ukeys, uperm, ugrad, hyper=self.hyper, W=U, m=m, v=v)
        m, v = self._mv("user_bias")
        slrc_user_bias_update(ukeys, uperm, ubgrad, hyper=self.hyper, user_bias=self.P["user_bias"], m=m, v=v)
        m, v = self._mv("global_alpha")
        dense_update(self.P["global_alpha"], reduce_sum(gagrad), self.hyper, m=m, v=v)
        return loss


# ---- CFKG: translation distance on one entity table, fused margin-hinge step (models/general/CFKG.py:57-76) -----------------------

def cfkg_check_shape(d, n_cand=1, n_rel=1):
    """rc_cfkg_check_shape (host logic): emb_size in {16, 32, 64, 128}, at least one candidate, 1..8 relations; raises ValueError
    with the library's reason otherwise"""
    _check_shape("CFKG", "rc_cfkg_check_shape", d, n_cand, n_rel)


def cfkg_fwd_bwd_rows_per_block(d):
    """the rows one workgroup of rc_cfkg_fwd_bwd takes at emb_size d (host logic); the launch geometry changes at its multiples"""
    return int(_lib.load().rc_cfkg_fwd_bwd_rows_per_block(int(d)))


def _cfkg_shapes(E, R, head, tail, rel):
    d = E.shape[1]
    if R.dim() != 2 or R.shape[1] != d:
        raise ValueError("CFKG: e_embeddings and r_embeddings need the same emb_size")
    if head.dim() != 2 or tail.shape != head.shape or rel.shape != head.shape:
        raise ValueError(f"CFKG: head_id, tail_id and relation_id must share one [B, C] shape; got {tuple(head.shape)}, "
                         f"{tuple(tail.shape)}, {tuple(rel.shape)}")
    return head.shape[0], head.shape[1], d


def _cfkg_front_args(E, R, head, tail, rel):
    f32, i64 = torch.float32, torch.int64
    return (_ptr(E, f32, "E"), _ptr(R, f32, "R"), _ptr(head, i64, "head_id"), _ptr(tail, i64, "tail_id"), _ptr(rel, i64, "relation_id"))


def cfkg_scores(E, R, head, tail, rel):
    """pred[b, c] = -|E[head[b, c]] + R[rel[b, c]] - E[tail[b, c]]|^2 for any [B, C] id triple (rc_cfkg_scores)"""
    B, Cn, d = _cfkg_shapes(E, R, head, tail, rel)
    pred = torch.empty((B, Cn), dtype=torch.float32, device=E.device)
    _lib.call("rc_cfkg_scores", *_cfkg_front_args(E, R, head, tail, rel), B, Cn, d, E.shape[0], R.shape[0],
              _ptr(pred, torch.float32, "pred"), _stream())
    return pred


def cfkg_scores_grads(E, R, head, tail, rel, gpred):
    """rc_cfkg_scores_bwd: for a given gpred [B, C] the head rows' gradient G [B * C, d] = -2 gpred (E[head] + R[rel] - E[tail]);
    the tail rows' is -G, the relation rows' is G"""
    B, Cn, d = _cfkg_shapes(E, R, head, tail, rel)
    G = torch.empty((B * Cn, d), dtype=torch.float32, device=E.device)
    _lib.call("rc_cfkg_scores_bwd", *_cfkg_front_args(E, R, head, tail, rel), _ptr(gpred, torch.float32, "gpred"), B, Cn, d, E.shape[0],
              R.shape[0], _ptr(G, torch.float32, "G"), _stream())
    return G


def cfkg_fwd_bwd(E, R, h, t, hn, tn, r, margin=0.0, inv_b=None, want_pred=True):
    """rc_cfkg_fwd_bwd: the quadruple feed's scores, MarginRankingLoss(margin) and backward in one launch + the relation reduce.
    h, t, hn, tn: int64 [B] row indices of E; r: int64 [B].
    Returns (pred [B, 4] | None, loss_vec [B], grows [B, 4, d] (rows of h, t, hn, tn), GR [n_rel, d])."""
    B, d, n_rel = h.shape[0], E.shape[1], R.shape[0]
    if R.shape[1] != d:
        raise ValueError("CFKG: e_embeddings and r_embeddings need the same emb_size")
    if any(x.shape != (B,) for x in (t, hn, tn, r)):
        raise ValueError("CFKG: h, t, hn, tn and r must all be [B]")
    cfkg_check_shape(d, 4, n_rel)
    if inv_b is None:
        inv_b = 1.0 / B
    dev, f32, i64 = E.device, torch.float32, torch.int64
    pred = torch.empty((B, 4), dtype=f32, device=dev) if want_pred else None
    loss_vec = torch.empty(B, dtype=f32, device=dev)
    grows = torch.empty((B, 4, d), dtype=f32, device=dev)
    GR = torch.empty((n_rel, d), dtype=f32, device=dev)
    ws = workspace(_lib.load().rc_cfkg_fwd_bwd_workspace_bytes(B, d, n_rel), dev, "cfkg_front")
    _lib.call("rc_cfkg_fwd_bwd", _ptr(E, f32, "E"), _ptr(R, f32, "R"), _ptr(h, i64, "h"), _ptr(t, i64, "t"), _ptr(hn, i64, "hn"),
              _ptr(tn, i64, "tn"), _ptr(r, i64, "r"), B, d, E.shape[0], n_rel, float(margin), float(inv_b),
              _ptr(loss_vec, f32, "loss_vec"), _ptr(pred, f32, "pred", True), _ptr(grows, f32, "grows"), _ptr(GR, f32, "GR"),
              *_ws_args(ws))
    return pred, loss_vec, grows, GR


class CfkgTrainer(_RowwiseTrainer):
    """CFKG training on the device tables E [n_users + n_entities, d] and R [n_relations, d] (e_embeddings, r_embeddings of
    models/general/CFKG.py:50-55).

    One `step(head, tail, rel)` = one iteration of BaseRunner.fit's batch loop (helpers/BaseRunner.py:193-206) on the [B, 4] training
    feed: rc_cfkg_fwd_bwd -> one rc_sort_ids over the 4 B keys (h, t, h', t') -> one rc_segmented_update of E from the gradient rows
    -> rc_dense_update of R.  The two tables follow different semantics, on purpose: E is updated ROW-WISE (only rows of the batch
    move, and only their optimizer state; weight decay reaches only them -- the semantics of BprmfTrainer), and the joint sort is
    what makes an entity that is a head in one row and a tail in another (or in the same row) see ONE summed gradient.  R has at
    most 8 rows and essentially every batch touches all of them, so it is updated DENSELY from GR and follows torch.optim exactly
    (weight decay and Adam's moment decay on every row, every step)."""

    def __init__(self, E, R, margin=0.0, opt="SGD", lr=1e-3, l2=0.0, beta1=0.9, beta2=0.999, eps=None):
        super().__init__(opt, lr, l2, beta1, beta2, eps)
        self.E, self.R, self.margin = E, R, float(margin)
        self.P = {"E": E, "R": R}
        self.d = E.shape[1]
        cfkg_check_shape(self.d, 4, R.shape[0])
        self._new_state()

    def step(self, head, tail, rel, inv_b=None):
        """one training step on head_id / tail_id / relation_id [B, 4]; returns the device loss tensor (shape [1], no sync)"""
        if head.dim() != 2 or head.shape[1] != 4 or tail.shape != head.shape or rel.shape != head.shape:
            raise ValueError(f"CfkgTrainer: the training feed is head_id, tail_id, relation_id [B, 4]; got {tuple(head.shape)}, "
                             f"{tuple(tail.shape)}, {tuple(rel.shape)}")
        B = head.shape[0]
        if inv_b is None:
            inv_b = 1.0 / B
        # (h, t, h', t') per row, in the order of the gradient rows: the sort's occurrence o = 4 b + j is row o of grows
        dev, i64 = self.E.device, torch.int64
        ids = torch.empty((B, 4), dtype=i64, device=dev)
        torch.stack((head[:, 0], tail[:, 0], head[:, 3], tail[:, 2]), dim=1, out=ids)
        cols = torch.empty((4, B), dtype=i64, device=dev)
        cols.copy_(ids.t())
        r = torch.empty(B, dtype=i64, device=dev)
        r.copy_(rel[:, 0])
        self.hyper.step += 1
        _, loss_vec, grows, GR = cfkg_fwd_bwd(self.E, self.R, cols[0], cols[1], cols[2], cols[3], r, self.margin, inv_b, want_pred=False)
        loss = reduce_sum(loss_vec, inv_b)
        keys, perm = sort_ids(ids, self.E.shape[0])
        m, v = self._mv("E")
        segmented_update(keys, perm, grows.view(4 * B, self.d), hyper=self.hyper, W=self.E, m=m, v=v)
        m, v = self._mv("R")
        dense_update(self.R, GR, self.hyper, m=m, v=v)
        return loss


# ---- DIN: target attention over the history (models/context_seq/DIN.py:63-95; csrc/din.hip) --------------------------------------

def _din_widths(widths):
    widths = [int(w) for w in widths]
    return len(widths), (C.c_int * max(len(widths), 1))(*widths)


def din_check_shape(H, L, widths, drop_p=0.0):
    """rc_din_check_shape (host logic), the one statement of the envelope: H a multiple of 4 in [4, 512], 1 <= L <= 64, 1 to 3 hidden
    widths, each a multiple of 16 in [16, 256] and at most 256 in all, 0 <= drop_p < 1; raises ValueError with the library's reason"""
    n, arr = _din_widths(widths)
    _check_shape("DIN attention", "rc_din_check_shape", H, L, n, extra=(arr, C.c_float(float(drop_p))))


def din_param_count(H, widths):
    """floats of the attention MLP's parameters in definition order [W_1 | b_1 | W_2 | b_2 | W_3 | b_3 | w_out | b_out]"""
    n, arr = _din_widths(widths)
    return int(_lib.load().rc_din_param_count(int(H), n, arr))


def _din_shapes(q, keys, lengths, params, n_cand, widths):
    if keys.dim() != 3 or q.dim() != 2 or q.shape[1] != keys.shape[2] or q.shape[0] != keys.shape[0] * n_cand:
        raise ValueError(f"DIN attention: q [B * C, H] and keys [B, L, H] do not fit: {tuple(q.shape)}, {tuple(keys.shape)}, C={n_cand}")
    B, L, H = keys.shape
    if lengths.shape != (B,):
        raise ValueError(f"DIN attention: lengths must be [B], got {tuple(lengths.shape)}")
    din_check_shape(H, L, widths)
    if params.dim() != 1 or params.numel() != din_param_count(H, widths):
        raise ValueError(f"DIN attention: params must hold {din_param_count(H, widths)} floats, got {tuple(params.shape)}")
    return B, L, H


def din_attention_fwd(q, keys, lengths, params, n_cand, widths, drop_p=0.0, seed=None, site0=0, out=None, want_att=False):
    """rc_din_attention_fwd: out[n] = sum_l w[n, l] keys[b, l] with the masked, scaled attention weights w of DIN.attention.
    q [B * C, H], keys [B, L, H], lengths int64 [B], params: the attention MLP flat in definition order.
    out: None (a fresh [N, H]) or a 2-D view with unit column stride whose row stride is a multiple of 4 (a slice of a wider buffer).
    Returns (out, att [N, L] | None)."""
    B, L, H = _din_shapes(q, keys, lengths, params, n_cand, widths)
    f32, N = torch.float32, q.shape[0]
    if out is None:
        out = torch.empty((N, H), dtype=f32, device=q.device)
    if out.dtype != f32 or not out.is_cuda or out.shape != (N, H) or out.stride(1) != 1:
        raise ValueError("DIN attention: out must be a float32 [N, H] GPU view with unit column stride")
    att = torch.empty((N, L), dtype=f32, device=q.device) if want_att else None
    n, arr = _din_widths(widths)
    _lib.call("rc_din_attention_fwd", _ptr(q, f32, "q"), _ptr(keys, f32, "keys"), _ptr(lengths, torch.int64, "lengths"),
              _ptr(params, f32, "params"), B, int(n_cand), L, H, n, arr, *_drop_args(drop_p, seed), C.c_uint32(int(site0)),
              C.c_void_p(out.data_ptr()), out.stride(0), _ptr(att, f32, "att", True), _stream())
    return out, att


def din_attention_bwd(q, keys, lengths, params, d_out, n_cand, widths, drop_p=0.0, seed=None, site0=0):
    """rc_din_attention_bwd: (dq [N, H], dkeys [B, L, H], dparams) for a given d_out [N, H]; everything recomputed from the inputs
    with the forward's seed and site0.  No float atomics: two runs are bit-equal."""
    B, L, H = _din_shapes(q, keys, lengths, params, n_cand, widths)
    f32, dev = torch.float32, q.device
    dq, dkeys, dparams = torch.empty_like(q), torch.empty_like(keys), torch.empty_like(params)
    n, arr = _din_widths(widths)
    ws = workspace(_lib.load().rc_din_attention_bwd_workspace_bytes(B, H, n, arr), dev, "din_bwd")
    _lib.call("rc_din_attention_bwd", _ptr(q, f32, "q"), _ptr(keys, f32, "keys"), _ptr(lengths, torch.int64, "lengths"),
              _ptr(params, f32, "params"), _ptr(d_out, f32, "d_out"), B, int(n_cand), L, H, n, arr, *_drop_args(drop_p, seed),
              C.c_uint32(int(site0)), _ptr(dq, f32, "dq"), _ptr(dkeys, f32, "dkeys"), _ptr(dparams, f32, "dparams"), *_ws_args(ws))
    return dq, dkeys, dparams


# ---- KDA: relational dynamic aggregation (models/sequential/KDA.py:265-303; csrc/kda.hip) ---------------------------------------------

def kda_check_shape(V, L, R, F):
    """rc_kda_check_shape (host logic), the one statement of the envelope: V in {16, 32, 64, 128}, 1 <= L <= 64, 1 <= R <= 8,
    2 <= F <= 129; raises ValueError with the library's reason"""
    _check_shape("KDA aggregation", "rc_kda_check_shape", V, L, R, F)


def _kda_shapes(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val):
    if seq.dim() != 3 or target.dim() != 3 or target.shape[0] != seq.shape[0] or target.shape[2] != seq.shape[2]:
        raise ValueError(f"KDA aggregation: seq [B, L, V] and target [B, C, V] do not fit: {tuple(seq.shape)}, {tuple(target.shape)}")
    (B, L, V), Cn = seq.shape, target.shape[1]
    if rel.dim() != 2 or rel.shape[1] != V:
        raise ValueError(f"KDA aggregation: rel must be [R, {V}], got {tuple(rel.shape)}")
    R = rel.shape[0]
    if freq_real.dim() != 2 or freq_real.shape[0] != R or freq_imag.shape != freq_real.shape:
        raise ValueError(f"KDA aggregation: freq_real and freq_imag must both be [{R}, F], got {tuple(freq_real.shape)}, "
                         f"{tuple(freq_imag.shape)}")
    F = freq_real.shape[1]
    if hist.shape != (B, L) or delta_t.shape != (B, L):
        raise ValueError(f"KDA aggregation: hist and delta_t must be [{B}, {L}], got {tuple(hist.shape)}, {tuple(delta_t.shape)}")
    if include_val and (value is None or value.shape != (B, Cn, R, V)):
        raise ValueError(f"KDA aggregation: value must be [{B}, {Cn}, {R}, {V}], got {None if value is None else tuple(value.shape)}")
    if Cn < 1:
        raise ValueError("KDA aggregation: need at least one candidate")
    kda_check_shape(V, L, R, F)
    return B, Cn, L, R, V, F


def _kda_inputs(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val):
    f32 = torch.float32
    return (_ptr(seq, f32, "seq"), _ptr(hist, torch.int64, "hist"), _ptr(delta_t, f32, "delta_t"), _ptr(target, f32, "target"),
            _ptr(value if include_val else None, f32, "value", True), _ptr(rel, f32, "rel"), _ptr(freq_real, f32, "freq_real"),
            _ptr(freq_imag, f32, "freq_imag"))


def kda_aggregate_fwd(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val=True):
    """rc_kda_aggregate_fwd: context [B, C, R, V] = sum_l softmax_l(<seq[b, l], ri>)[l] decay[b, l, r] seq[b, l] over the valid l
    (hist > 0), ri = (rel[r] + value[b, c, r]) * target[b, c] (include_val) or rel[r] * target[b, c]; one launch.  A row without a
    valid position gives zeros."""
    B, Cn, L, R, V, F = _kda_shapes(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val)
    ctx = torch.empty((B, Cn, R, V), dtype=torch.float32, device=seq.device)
    if B:
        _lib.call("rc_kda_aggregate_fwd", *_kda_inputs(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val),
                  B, Cn, L, R, V, F, int(bool(include_val)), _ptr(ctx, torch.float32, "context"), _stream())
    return ctx


def kda_aggregate_bwd(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, d_context, include_val=True):
    """rc_kda_aggregate_bwd: (dseq, dtarget, dvalue | None, drel, dfreq_real, dfreq_imag) for a given d_context [B, C, R, V];
    everything recomputed from the inputs.  No atomics: two runs are bit-equal."""
    B, Cn, L, R, V, F = _kda_shapes(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val)
    f32, dev = torch.float32, seq.device
    if d_context.shape != (B, Cn, R, V):
        raise ValueError(f"KDA aggregation: d_context must be [{B}, {Cn}, {R}, {V}], got {tuple(d_context.shape)}")
    dseq, dtarget = torch.empty_like(seq), torch.empty_like(target)
    dvalue = torch.empty((B, Cn, R, V), dtype=f32, device=dev) if include_val else None
    drel, dfr, dfi = torch.empty_like(rel), torch.empty_like(freq_real), torch.empty_like(freq_imag)
    if not B:
        return dseq, dtarget, dvalue, drel.zero_(), dfr.zero_(), dfi.zero_()
    ws = workspace(_lib.load().rc_kda_aggregate_bwd_workspace_bytes(B, R, V, F), dev, "kda_bwd")
    _lib.call("rc_kda_aggregate_bwd", *_kda_inputs(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val),
              _ptr(d_context, f32, "d_context"), B, Cn, L, R, V, F, int(bool(include_val)), _ptr(dseq, f32, "dseq"),
              _ptr(dtarget, f32, "dtarget"), _ptr(dvalue, f32, "dvalue", True), _ptr(drel, f32, "drel"), _ptr(dfr, f32, "dfreq_real"),
              _ptr(dfi, f32, "dfreq_imag"), *_ws_args(ws))
    return dseq, dtarget, dvalue, drel, dfr, dfi


# ---- Chorus: knowledge- and time-aware item vectors, two stages (models/sequential/Chorus.py:100-177; csrc/chorus.hip) -------------

CHORUS_PARAMS = ("U", "I", "Rel", "betas", "mus", "sigmas", "w", "user_bias", "item_bias")   # the reference's definition order
CHORUS_CAT_TABLES = ("betas", "sigmas", "mus")   # the [3] arrays of rc_chorus_category_update and kgrad's column blocks
CHORUS_KINDS = {"exponential": 0, "complement": 1, "substitute": 2}


def chorus_kinds(item_relations):
    """the temporal kernel of every relation (Chorus.py:106-118): relation 0 and a column naming neither word take the exponential
    one, 'complement' is tested before 'substitute'"""
    kinds = [0]
    for name in item_relations:
        kinds.append(1 if "complement" in name else (2 if "substitute" in name else 0))
    return kinds


def chorus_check_shape(d, n_cand=1, n_rel=1):
    """rc_chorus_check_shape (host logic): emb_size in {16, 32, 64, 128}, at least one candidate, 1..8 relations; raises ValueError
    with the library's reason otherwise"""
    _check_shape("Chorus", "rc_chorus_check_shape", d, n_cand, n_rel)


def chorus_front_tuples_per_block():
    """the tuples one workgroup of rc_chorus_fwd_bwd takes (host logic); the launch geometry changes at its multiples"""
    return int(_lib.load().rc_chorus_front_tuples_per_block())


def chorus_category_piece():
    """the sorted positions one workgroup of rc_chorus_category_update sums (host logic)"""
    return int(_lib.load().rc_chorus_category_piece())


def chorus_kg_feed(head_id, tail_id):
    """Stage 1's feed (Chorus.py:216-219: head_id = (t, t, t', t), tail_id = (h, h, h, h'), which corrupts the HEAD slot in pair 1)
    in the layout of rc_cfkg_fwd_bwd / CfkgTrainer (head = (a, a, a, a'), tail = (b, b, b', b), which corrupts the TAIL slot in
    pair 1): the two pairs exchanged.  The per-row loss is unchanged; `pred` columns 2 and 3 come out swapped."""
    a, b = head_id[:, 0], tail_id[:, 0]
    return torch.stack((a, a, a, head_id[:, 2]), dim=1), torch.stack((b, b, tail_id[:, 3], b), dim=1)


def _chorus_shapes(P, uid, iid, cid, intervals, kinds):
    U, I, Rel, betas, mus, sigmas, w, ub, ib = P
    d, n_users, n_items, R = U.shape[1], U.shape[0], I.shape[0], Rel.shape[0]
    if I.shape[1] != d or Rel.shape[1] != d or w.numel() != d:
        raise ValueError("Chorus: u_embeddings, i_embeddings, r_embeddings and prediction.weight need the same emb_size")
    if ub.numel() != n_users or ib.numel() != n_items:
        raise ValueError("Chorus: user_bias [n_users, 1] and item_bias [n_items, 1] are needed")
    if betas.dim() != 2 or betas.shape[1] != R or sigmas.shape != betas.shape or mus.shape != betas.shape:
        raise ValueError("Chorus: betas, mus and sigmas must all be [category_num, relation_num]")
    if iid.dim() != 2 or uid.shape != (iid.shape[0],) or cid.shape != iid.shape or tuple(intervals.shape) != (*iid.shape, R):
        raise ValueError(f"Chorus: need uid [B], iid [B, C], category_id [B, C], relational_interval [B, C, {R}]; got "
                         f"{tuple(uid.shape)}, {tuple(iid.shape)}, {tuple(cid.shape)}, {tuple(intervals.shape)}")
    if len(kinds) != R or any(k not in (0, 1, 2) for k in kinds):
        raise ValueError(f"Chorus: kinds must hold {R} values of 0 / 1 / 2, got {list(kinds)}")
    return iid.shape[0], iid.shape[1], d, R


def _chorus_tables(P, gmf, with_bias=True):
    """(U, I, Rel, betas, sigmas, mus, w | NULL [, user_bias, item_bias]) in the entry points' order"""
    U, I, Rel, betas, mus, sigmas, w, ub, ib = P
    f32 = torch.float32
    out = (_ptr(U, f32, "U"), _ptr(I, f32, "I"), _ptr(Rel, f32, "Rel"), _ptr(betas, f32, "betas"), _ptr(sigmas, f32, "sigmas"),
           _ptr(mus, f32, "mus"), _ptr(w if gmf else None, f32, "w", True))
    if with_bias:
        out += (_ptr(None if gmf else ub, f32, "user_bias", True), _ptr(None if gmf else ib, f32, "item_bias", True))
    return out


def _chorus_ids(uid, iid, cid, intervals, kinds):
    i64 = torch.int64
    return (_ptr(uid, i64, "uid"), _ptr(iid, i64, "iid"), _ptr(cid, i64, "category_id"),
            _ptr(intervals, torch.float32, "relational_interval"), (C.c_int * len(kinds))(*[int(k) for k in kinds]))


def chorus_scores(P, uid, iid, cid, intervals, kinds, gmf=False):
    """Chorus's stage-2 prediction [B, C] for any C >= 1 (rc_chorus_scores); P: the nine parameter tensors in CHORUS_PARAMS order"""
    B, Cn, d, R = _chorus_shapes(P, uid, iid, cid, intervals, kinds)
    pred = torch.empty((B, Cn), dtype=torch.float32, device=iid.device)
    _lib.call("rc_chorus_scores", *_chorus_tables(P, gmf), *_chorus_ids(uid, iid, cid, intervals, kinds), B, Cn, d, R,
              _ptr(pred, torch.float32, "pred"), _stream())
    return pred


def _chorus_front_outputs(B, Cn, d, R, gmf, dev):
    f32 = torch.float32
    out = {"coef": torch.empty((B, Cn), dtype=f32, device=dev), "ugrad": torch.empty((B, d), dtype=f32, device=dev),
           "ubgrad": torch.empty(B, dtype=f32, device=dev), "kgrad": torch.empty((B * Cn, 3 * R), dtype=f32, device=dev),
           "GRel": torch.empty((R, d), dtype=f32, device=dev),
           "gw": torch.empty(d, dtype=f32, device=dev) if gmf else None,
           "uprime": torch.empty((B, d), dtype=f32, device=dev) if gmf else None}
    args = tuple(_ptr(out[k], f32, k, k in ("gw", "uprime")) for k in ("coef", "ugrad", "ubgrad", "kgrad", "GRel", "gw", "uprime"))
    return out, args


def chorus_fwd_bwd(P, uid, iid, cid, intervals, kinds, gmf=False, inv_b=None, want_pred=True):
    """rc_chorus_fwd_bwd: scores + GeneralModel.loss + backward in one launch, plus the fixed-order reduce of GRel / gw.
    Returns a dict: pred | None, loss_vec [B], gpred [B, C], coef [B, C], ugrad [B, d], ubgrad [B], kgrad [B * C, 3 R] (betas | sigmas
    | mus), GRel [R, d], and for GMF gw [d], uprime [B, d] (None for BPR)."""
    B, Cn, d, R = _chorus_shapes(P, uid, iid, cid, intervals, kinds)
    if inv_b is None:
        inv_b = 1.0 / B
    dev, f32 = iid.device, torch.float32
    out, out_args = _chorus_front_outputs(B, Cn, d, R, gmf, dev)
    out["pred"], out["loss_vec"], out["gpred"] = _step_outputs(B, Cn, dev, want_pred)
    ws = workspace(_lib.load().rc_chorus_front_workspace_bytes(B, d, R), dev, "chorus_front")
    _lib.call("rc_chorus_fwd_bwd", *_chorus_tables(P, gmf), *_chorus_ids(uid, iid, cid, intervals, kinds), B, Cn, d, R, float(inv_b),
              _ptr(out["pred"], f32, "pred", True), _ptr(out["loss_vec"], f32, "loss_vec"), _ptr(out["gpred"], f32, "gpred"), *out_args,
              *_ws_args(ws))
    return out


def chorus_scores_grads(P, uid, iid, cid, intervals, kinds, gpred, gmf=False):
    """rc_chorus_scores_bwd: for a given gpred [B, C] the dict of chorus_fwd_bwd without pred, loss_vec and gpred"""
    B, Cn, d, R = _chorus_shapes(P, uid, iid, cid, intervals, kinds)
    if gpred.shape != (B, Cn):
        raise ValueError(f"Chorus: gpred must be [{B}, {Cn}], got {tuple(gpred.shape)}")
    dev = iid.device
    out, out_args = _chorus_front_outputs(B, Cn, d, R, gmf, dev)
    ws = workspace(_lib.load().rc_chorus_front_workspace_bytes(B, d, R), dev, "chorus_front")
    ids = _chorus_ids(uid, iid, cid, intervals, kinds)
    _lib.call("rc_chorus_scores_bwd", *_chorus_tables(P, gmf, with_bias=False), *ids, _ptr(gpred, torch.float32, "gpred"), B, Cn, d, R,
              *out_args, *_ws_args(ws))
    return out


def chorus_category_update(keys, perm, heads, n_heads, kgrad, n_cat, hyper=None, W=None, m=None, v=None, dense_grad=None,
                           workspace_buf=None):
    """rc_chorus_category_update: one pass over the sorted category ids (keys / perm of sort_ids(cid), heads / n_heads of
    segment_heads) that sums kgrad [n_occ, 3 R] per distinct category and either applies `hyper` to that row of the three tables W
    (m, v: their states; CHORUS_CAT_TABLES order) in place or writes the three dense gradients"""
    n_occ = keys.numel()
    if kgrad.dim() != 2 or kgrad.shape[0] != n_occ or kgrad.shape[1] % 3:
        raise ValueError(f"Chorus: kgrad must be [{n_occ}, 3 R], got {tuple(kgrad.shape)}")
    R = kgrad.shape[1] // 3
    for t in (W or []) + (dense_grad or []):
        if t is not None and tuple(t.shape) != (int(n_cat), R):
            raise ValueError(f"Chorus: every category table must be [{int(n_cat)}, {R}], got {tuple(t.shape)}")
    f32, i32 = torch.float32, torch.int32
    need = _lib.load().rc_chorus_category_update_workspace_bytes(n_occ, int(n_cat), R)
    ws = workspace_buf if workspace_buf is not None else workspace(need, keys.device, "chorus_cat")
    T = CHORUS_CAT_TABLES
    _lib.call("rc_chorus_category_update", _ptr_array(W, T, "W", True), _ptr_array(m, T, "m", True), _ptr_array(v, T, "v", True), int(n_cat), R,
              _ptr(keys, i32, "keys"), _ptr(perm, i32, "perm"), n_occ, _ptr(kgrad, f32, "kgrad"), _hyper_ref(hyper),
              _ptr_array(dense_grad, T, "dense_grad", True), _ptr(heads, i32, "heads"), _ptr(n_heads, i32, "n_heads"), *_ws_args(ws))


class ChorusTrainer(_RowwiseTrainer):
    """Row-wise-optimizer training of Chorus's stage 2 on the nine device parameters (CHORUS_PARAMS order; Chorus.py:79-88).

    One `step(uid, iid, cid, intervals)` = one iteration of BaseRunner.fit's batch loop (helpers/BaseRunner.py:193-206): three sorts
    (candidates, categories, users) + the categories' head list -> rc_chorus_fwd_bwd -> rc_segmented_update on I (coef, the pre-step U
    or uprime) -> rc_slrc_user_bias_update on item_bias (gpred is its per-occurrence gradient) -> rc_chorus_category_update ->
    rc_dense_update on Rel (and on prediction.weight for GMF) -> the user side last: rc_segmented_update on U, rc_slrc_user_bias_update
    on user_bias.  Three hyper records, as Chorus.customize_parameters groups the parameters (Chorus.py:179-194): (lr, l2) for U,
    betas, mus, sigmas and prediction.weight; (lr_scale * lr, l2) for I and Rel; (lr, 0) for the two bias tables.  Only rows of the
    batch move (and only their optimizer state); Rel and prediction.weight are dense and follow torch.optim exactly.  A parameter the
    head does not read (the biases under GMF, prediction.weight under BPR, sigmas and mus without a 'substitute' relation) has no
    gradient and is left alone, as torch.optim does."""

    def __init__(self, *params, kinds, gmf=False, opt="SGD", lr=1e-3, l2=0.0, lr_scale=0.1, beta1=0.9, beta2=0.999, eps=None):
        super().__init__(opt, lr, l2, beta1, beta2, eps)
        if len(params) != len(CHORUS_PARAMS):
            raise ValueError("ChorusTrainer: nine parameter tensors are needed: " + ", ".join(CHORUS_PARAMS))
        self.P = dict(zip(CHORUS_PARAMS, params))
        self.d, self.R, self.n_cat = self.P["U"].shape[1], self.P["Rel"].shape[0], self.P["betas"].shape[0]
        chorus_check_shape(self.d, 1, self.R)
        self.kinds, self.gmf = [int(k) for k in kinds], bool(gmf)
        self.hyper_kg = make_hyper(opt, lr_scale * lr, l2, beta1, beta2, eps, step=0)
        self.hyper_bias = make_hyper(opt, lr, 0.0, beta1, beta2, eps, step=0)
        self._new_state()

    def step(self, uid, iid, cid, intervals, inv_b=None):
        """one training step; returns the device loss tensor (shape [1], no sync)"""
        P = [self.P[k] for k in CHORUS_PARAMS]
        B, Cn, d, R = _chorus_shapes(P, uid, iid, cid, intervals, self.kinds)
        if inv_b is None:
            inv_b = 1.0 / B
        U, I = self.P["U"], self.P["I"]
        for h in (self.hyper, self.hyper_kg, self.hyper_bias):
            h.step += 1
        ikeys, iperm = sort_ids(iid, I.shape[0])
        ckeys, cperm = sort_ids(cid, self.n_cat)
        _, heads, n_heads = segment_heads(ckeys, cperm, want_single=False)
        ukeys, uperm = sort_ids(uid, U.shape[0])
        out = chorus_fwd_bwd(P, uid, iid, cid, intervals, self.kinds, self.gmf, inv_b, want_pred=False)
        loss = reduce_sum(out["loss_vec"], inv_b)
        m, v = self._mv("I")
        if self.gmf:
            segmented_update(ikeys, iperm, out["uprime"], hyper=self.hyper_kg, W=I, m=m, v=v, coef=out["coef"], div=Cn)
        else:
            segmented_update(ikeys, iperm, U, hyper=self.hyper_kg, W=I, m=m, v=v, coef=out["coef"], src_index=uid, div=Cn)
            m, v = self._mv("item_bias")
            slrc_user_bias_update(ikeys, iperm, out["gpred"], hyper=self.hyper_bias, user_bias=self.P["item_bias"], m=m, v=v)
        W, m, v = self._tables(CHORUS_CAT_TABLES)
        # sigmas and mus are read by the 'substitute' kernel alone: without one they have no gradient and stay as they are
        live = [True, 2 in self.kinds, 2 in self.kinds]
        chorus_category_update(ckeys, cperm, heads, n_heads, out["kgrad"], self.n_cat, hyper=self.hyper,
                               W=[t if on else None for t, on in zip(W, live)], m=m, v=v)
        m, v = self._mv("Rel")
        dense_update(self.P["Rel"], out["GRel"], self.hyper_kg, m=m, v=v)
        if self.gmf:
            m, v = self._mv("w")
            dense_update(self.P["w"], out["gw"].view_as(self.P["w"]), self.hyper, m=m, v=v)
        # the user side last: the item update above read the pre-step U
        m, v = self._mv("U")
        segmented_update(ukeys, uperm, out["ugrad"], hyper=self.hyper, W=U, m=m, v=v)
        if not self.gmf:
            m, v = self._mv("user_bias")
            slrc_user_bias_update(ukeys, uperm, out["ubgrad"], hyper=self.hyper_bias, user_bias=self.P["user_bias"], m=m, v=v)
        return loss
