"""Guard bands for the engine wrappers: an arena whose every view lies between two bands of a known pattern, and a stand-in for the
name `torch` inside rechorus_amd.engine that serves the wrappers' own allocations (outputs, workspaces) from that arena.

A kernel that stores past its output, uses more scratch than its *_workspace_bytes function declares, or keeps a value it read
past an input's end changes nothing a value comparison sees while torch's caching allocator pads and packs the blocks.  Here the
byte after a view's last byte is band: float tensors sit between bands of the 32-bit word 0x7FC0DEAD (a quiet NaN: a kept over-read
surfaces in the values), integer tensors (ids, offsets, lengths, permutations, keys) between zero bytes -- zero is a valid id, offset
and length everywhere in the ABI, so an over-read index never becomes a wild address.  uint8 buffers (workspaces, flag arrays) get a
third pattern, the 64-bit word 1: a workspace is where counters are zero-filled, and a zero fill that runs past the declared size would
vanish in a zero band; read as int32 or int64 the band is only ever 0 or 1, still a valid index.

Plain helper module: no conftest, no plugin.  tests/test_guarded_cpu.py holds it to what it claims on a CPU arena."""
import contextlib

import numpy as np
import torch

FLOAT_WORD = 0x7FC0DEAD
ALIGN = 256
_FLOAT_BYTES = [(FLOAT_WORD >> (8 * k)) & 0xFF for k in range(4)]     # little endian
_SCRATCH_BYTES = [1, 0, 0, 0, 0, 0, 0, 0]                               # the 64-bit word 1: int32 reads 1, 0, 1, 0, ..., int64 reads 1
_PERIOD = {"float": 4, "int": 1, "scratch": 8}


def band_of(dtype):
    """which band pattern lies beside a tensor of this dtype"""
    return "float" if dtype.is_floating_point else ("scratch" if dtype == torch.uint8 else "int")
_SERVED = ("empty", "empty_like", "zeros", "zeros_like", "full", "ones")
_REFUSED = ("full_like", "ones_like", "empty_strided", "rand", "randn", "randint", "rand_like", "randn_like")   # would escape the arena


class GuardError(AssertionError):
    pass


def _bytes(t):
    """the tensor's memory as a flat uint8 view (bit-for-bit comparisons: NaN payloads and signed zeros count)"""
    return t.reshape(-1).view(torch.uint8)


class _View:
    def __init__(self, name, kind, start, nbytes, lead, trail_end, band, tensor):
        self.name, self.kind, self.start, self.nbytes = name, kind, start, nbytes
        self.lead, self.trail_end, self.band, self.tensor = lead, trail_end, band, tensor
        self.snapshot = None

    @property
    def end(self):
        return self.start + self.nbytes


class Arena:
    """One buffer.  take() hands out contiguous views: first byte 256-byte aligned (what the header promises a workspace; tensors
    need 16), the LAST byte immediately followed by the trailing band -- no padding up to the next alignment -- and at least
    `guard` bytes of band on either side, in the pattern of the view's own dtype (band_of)."""

    def __init__(self, device, nbytes, guard=65536):
        self.device = torch.device(device)
        self.guard = int(guard)
        self.buf = torch.empty(int(nbytes) + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = self.buf.data_ptr()
        self.size = self.buf.numel()
        n_pat = self.guard + 2 * ALIGN
        self._pat = {"float": torch.tensor(_FLOAT_BYTES * (n_pat // 4 + 2), dtype=torch.uint8).to(self.device),
                     "scratch": torch.tensor(_SCRATCH_BYTES * (n_pat // 8 + 2), dtype=torch.uint8).to(self.device),
                     "int": torch.zeros(n_pat + 8, dtype=torch.uint8, device=self.device)}
        self.reset()

    def reset(self):
        self.views = []
        self._off = 0

    def _pattern(self, band, a, b):
        """the band pattern of arena bytes [a, b): the words are aligned to absolute addresses, so that a float32 view of a float
        band reads NaN and an int64 view of a scratch band reads 1"""
        phase = (self.base + a) % _PERIOD[band]
        return self._pat[band][phase:phase + (b - a)]

    def take(self, shape, dtype, name, kind="out"):
        """kind: "out" (written by the call), "in" (must come back bit-identical), "table" (updated in place: the caller declares
        the rows that may change in check(tables=...)), "inout" (any of it may change)"""
        if isinstance(shape, (int, np.integer)):
            shape = (int(shape),)
        shape = tuple(int(s) for s in shape)
        numel = int(np.prod(shape, dtype=np.int64)) if shape else 1
        item = torch.empty(0, dtype=dtype).element_size()
        nbytes = numel * item
        lead = self._off
        start = (self.base + lead + self.guard + ALIGN - 1) // ALIGN * ALIGN - self.base
        trail_end = start + nbytes + self.guard
        if trail_end > self.size:
            raise MemoryError(f"guarded arena exhausted: {name} needs {nbytes} bytes, {self.size - lead} left of {self.size}")
        band = band_of(dtype)
        self.buf[lead:start].copy_(self._pattern(band, lead, start))
        self.buf[start + nbytes:trail_end].copy_(self._pattern(band, start + nbytes, trail_end))
        t = self.buf[start:start + nbytes].view(dtype).view(shape)
        self.views.append(_View(name, kind, start, nbytes, lead, trail_end, band, t))
        self._off = trail_end
        return t

    def put(self, src, name, kind="in"):
        """a copy of `src` (tensor or array) in the arena, registered as an input: its bits before the call are kept for check()"""
        src = torch.as_tensor(src)
        t = self.take(src.shape, src.dtype, name, kind)
        t.copy_(src)
        self.views[-1].snapshot = t.clone()
        return t

    def contains(self, t):
        """does the tensor's memory lie inside the arena (inside one taken view, to be exact)?"""
        if t.numel() == 0:
            return True
        if not t.is_contiguous():      # a strided window (a column block of a wider result): its first and last element
            flat = t.reshape(-1) if t.dim() == 0 else t
            last = sum((s - 1) * st for s, st in zip(flat.shape, flat.stride()))
            a = t.data_ptr() - self.base
            b = a + (last + 1) * t.element_size()
        else:
            a = t.data_ptr() - self.base
            b = a + t.numel() * t.element_size()
        return any(v.start <= a and b <= v.end for v in self.views)

    def view_of(self, t):
        a = t.data_ptr() - self.base
        for v in self.views:
            if v.start <= a < max(v.end, v.start + 1):
                return v
        return None

    def _check_band(self, v, side, a, b):
        got, want = self.buf[a:b], self._pattern(v.band, a, b)
        if torch.equal(got, want):
            return
        dirty = torch.nonzero(got != want).reshape(-1)
        first, last = int(dirty[0]) + a, int(dirty[-1]) + a
        if side == "after":
            where = f"bytes +{first - v.end} .. +{last - v.end} past the tensor's end"
        else:
            where = f"bytes {first - v.start} .. {last - v.start} before the tensor's start ({first - v.end} .. {last - v.end} from its end)"
        raise GuardError(f"guard band {side} '{v.name}' ({v.kind}, {v.nbytes} bytes) is dirty: {int(dirty.numel())} bytes, {where}")

    def check(self, inputs=None, tables=None):
        """after a synchronize: (a) every band holds its pattern bit for bit; (b) every input (all views of kind "in", or the
        tensors listed in `inputs`) is bit-identical to its copy from before the call; (c) of every view of kind "table" only the
        rows in tables[name] (indices into its first dimension) may differ from the copy."""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        for v in self.views:
            self._check_band(v, "before", v.lead, v.start)
            self._check_band(v, "after", v.end, v.trail_end)
        tables = dict(tables or {})
        listed = None if inputs is None else {t.data_ptr() for t in inputs}
        for v in self.views:
            if v.snapshot is None:
                continue
            if v.kind == "in" and (listed is None or v.tensor.data_ptr() in listed):
                if not torch.equal(_bytes(v.tensor), _bytes(v.snapshot)):
                    bad = torch.nonzero(_bytes(v.tensor) != _bytes(v.snapshot)).reshape(-1)
                    raise GuardError(f"input '{v.name}' was altered in place: {int(bad.numel())} bytes, first at byte {int(bad[0])}, "
                                     f"last at byte {int(bad[-1])} of {v.nbytes}")
            elif v.kind == "table":
                if v.name not in tables:
                    raise GuardError(f"table '{v.name}' is updated in place: check(tables=...) must name the rows that may change")
                rows = torch.as_tensor(tables.pop(v.name), dtype=torch.int64).reshape(-1).to(self.device)
                n = v.tensor.shape[0]
                a, b = v.tensor.reshape(n, -1), v.snapshot.reshape(n, -1)
                changed = (a.view(torch.uint8).reshape(n, -1) != b.view(torch.uint8).reshape(n, -1)).any(dim=1)
                allowed = torch.zeros(n, dtype=torch.bool, device=self.device)
                allowed[rows] = True
                stray = torch.nonzero(changed & ~allowed).reshape(-1)
                if stray.numel():
                    raise GuardError(f"table '{v.name}': {int(stray.numel())} rows outside the declared row set changed, first row "
                                     f"{int(stray[0])}, last row {int(stray[-1])}")
        if tables:
            raise GuardError(f"check(tables=...) names tables the arena does not hold: {sorted(tables)}")


class _TorchProxy:
    """what rechorus_amd.engine sees as `torch` under guarded(): every attribute is the real module's, except the allocation
    functions, which are served from the arena when they name the arena's device (device-less and other-device allocations pass
    through) and raise when asked for something the arena cannot give (strides, pinned memory, a memory format)."""

    def __init__(self, arena):
        self.__dict__["_arena"] = arena
        self.__dict__["served"] = []          # (what, shape, dtype, bytes)

    def __getattr__(self, name):
        if name in _REFUSED:
            raise GuardError(f"torch.{name} inside the engine is not served from the guarded arena: teach tests/guarded.py about it")
        return getattr(torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the guarded torch proxy is read-only")

    def _mine(self, device):
        return device is not None and torch.device(device).type == self._arena.device.type

    def _serve(self, what, shape, dtype, kw):
        if kw:
            raise GuardError(f"torch.{what}(..., {', '.join(sorted(kw))}=...) cannot be served from the guarded arena")
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        t = self._arena.take(shape, dtype, f"engine#{len(self.served)}:{what}{tuple(shape)}:{str(dtype)[6:]}", "out")
        self.served.append((what, tuple(shape), dtype, t.numel() * t.element_size()))
        return t

    @staticmethod
    def _size(size):
        """both conventions: empty((a, b), ...) and empty(n, ...) / empty(a, b, ...)"""
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        if not all(isinstance(s, (int, np.integer)) for s in size):
            raise GuardError(f"allocation size {size!r} is not a tuple of ints")
        return tuple(int(s) for s in size)

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._serve("empty", self._size(size), dtype, kw)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._serve("zeros", self._size(size), dtype, kw).zero_()

    def ones(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.ones(*size, dtype=dtype, device=device, **kw)
        return self._serve("ones", self._size(size), dtype, kw).fill_(1)

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        if dtype is None:
            raise GuardError("torch.full without a dtype: the proxy does not infer one")
        return self._serve("full", self._size((size,)), dtype, kw).fill_(fill_value)

    def empty_like(self, t, dtype=None, device=None, **kw):
        device = t.device if device is None else device
        if not self._mine(device):
            return torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._serve("empty_like", tuple(t.shape), t.dtype if dtype is None else dtype, kw)

    def zeros_like(self, t, dtype=None, device=None, **kw):
        device = t.device if device is None else device
        if not self._mine(device):
            return torch.zeros_like(t, dtype=dtype, device=device, **kw)
        return self._serve("zeros_like", tuple(t.shape), t.dtype if dtype is None else dtype, kw).zero_()


class Served:
    """what one guarded() block served: `count` allocations, each (what, shape, dtype, bytes) in `allocations`; `workspaces` lists
    (tag, bytes asked, buffer) of every engine.workspace() call"""

    def __init__(self, proxy):
        self._proxy = proxy
        self.workspaces = []

    @property
    def allocations(self):
        return list(self._proxy.served)

    @property
    def count(self):
        return len(self._proxy.served)

    @property
    def scratch_bytes(self):
        """bytes of uint8 buffers served: engine.workspace() and the per-shape workspace objects of the newer models"""
        return sum(n for _, _, dt, n in self._proxy.served if dt == torch.uint8)

    @property
    def output_bytes(self):
        return sum(n for _, _, dt, n in self._proxy.served if dt != torch.uint8)


@contextlib.contextmanager
def guarded(engine, arena, monkeypatch):
    """Inside the block rechorus_amd.engine allocates from `arena`: the name `torch` of that module alone is a _TorchProxy, and
    engine._ws_cache is an empty dict whose entries are dropped when a request of another size comes, so engine.workspace() allocates
    afresh at exactly the requested size (never below the 256 bytes it has always rounded up to) -- an entry point receives the byte count its own *_workspace_bytes function returned and
    not one byte more.  The per-shape workspace objects of DirectAU, ComiRec, ContraRec, BUIR, AutoInt and FinalMLP are created per
    call when the caller passes none (what the guarded tests do), so their buffers come from the arena as well.  -> Served"""
    proxy = _TorchProxy(arena)
    served = Served(proxy)
    real_workspace = engine.workspace

    def workspace(nbytes, device, tag="default"):
        # a cached buffer of another size would hand the kernel more than this call declares (or grow geometrically): drop it, so
        # that the real engine.workspace() allocates afresh
        key = (str(device), tag)
        cached = engine._ws_cache.get(key)
        if cached is not None and cached.numel() != max(int(nbytes), 256):
            del engine._ws_cache[key]
        buf = real_workspace(nbytes, device, tag)
        served.workspaces.append((tag, int(nbytes), buf))
        return buf

    with monkeypatch.context() as m:
        m.setattr(engine, "torch", proxy)
        m.setattr(engine, "_ws_cache", {})
        m.setattr(engine, "_ws_retired", [])
        if hasattr(engine, "_rows_plan_zeroed"):
            # RowsPlan zero-fills a workspace once per address: an arena address comes back with other contents after a reset
            m.setattr(engine, "_rows_plan_zeroed", set())
        m.setattr(engine, "workspace", workspace)
        yield served
