"""LightGCN's graph on the HIP engine: the normalised user-item adjacency as CSR and the propagation plan built once per model
(reference: models/general/LightGCN.py:23-53 `build_adjmat`, :137-151 `LGCNEncoder.forward`).

The adjacency is D^-1/2 A D^-1/2 of the bipartite graph over N = n_users + n_items nodes, users first.  It is built here with
vectorised numpy in the reference's float32 arithmetic (row sums in float32 + 1e-10, np.power(., -0.5), (d_i * a_ij) * d_j), so
`indptr` / `indices` equal the reference's and `data` is bit-equal to it -- the reference's dok_matrix loop does not finish at
millions of edges.  The graph never changes during training, so the plan the kernels follow (rc_lgcn_propagate_fwd/bwd) is built
once: work items longest first, and rows longer than `chunk` edges split into fixed-order chunks whose partial sums a second pass
adds per row (a hub row on one wave would set the duration of the whole product).
"""
import ctypes as C
import itertools

import numpy as np
import torch

# waves in flight on the whole MI355X (256 CUs x 32 waves): a row longer than a quarter of one wave's share of the edges is split
WAVES_IN_FLIGHT = 256 * 32
MIN_CHUNK = 64


def _pairs(train_clicked_set):
    """(users, items) int64 arrays of the training interactions: a {user: set(items)} dict (the corpus' train_clicked_set) or a
    pair of arrays"""
    if isinstance(train_clicked_set, dict):
        users = list(train_clicked_set.keys())
        lens = np.fromiter((len(train_clicked_set[u]) for u in users), dtype=np.int64, count=len(users))
        u = np.repeat(np.asarray(users, dtype=np.int64), lens)
        i = np.fromiter(itertools.chain.from_iterable(train_clicked_set[x] for x in users), dtype=np.int64, count=int(lens.sum()))
        return u, i
    u, i = train_clicked_set
    return np.asarray(u, dtype=np.int64).reshape(-1), np.asarray(i, dtype=np.int64).reshape(-1)


def build_norm_adj(n_users, n_items, train_clicked_set, check_symmetric=True):
    """the reference's `build_adjmat(n_users, n_items, train_clicked_set, selfloop_flag=False)` as CSR:
    (indptr int64 [N+1], indices int32 [nnz], data float32 [nnz]); repeated interactions count once (dok_matrix R[u, i] = 1)"""
    n_users, n_items = int(n_users), int(n_items)
    N = n_users + n_items
    u, i = _pairs(train_clicked_set)
    if u.size and (u.min() < 0 or u.max() >= n_users or i.min() < 0 or i.max() >= n_items):
        raise ValueError("build_norm_adj: an interaction lies outside [0, n_users) x [0, n_items)")
    key = np.unique(u * n_items + i)                 # sorted by (user, item), duplicates gone
    uu, ii = key // n_items, key % n_items
    key_t = np.sort(ii * n_users + uu)               # the transpose, sorted by (item, user)
    ti, tu = key_t // n_users, key_t % n_users
    rows = np.concatenate([uu, n_users + ti])
    cols = np.concatenate([n_users + ii, tu])
    deg = np.bincount(rows, minlength=N)
    # np.array(adj.sum(1)) + 1e-10 in float32 (the counts are exact), then np.power(., -0.5) as the reference takes it
    rowsum = deg.astype(np.float32).reshape(-1, 1) + 1e-10
    d_inv_sqrt = np.power(rowsum, -0.5).flatten()
    d_inv_sqrt[np.isinf(d_inv_sqrt)] = 0.
    data = (d_inv_sqrt[rows] * np.float32(1.0)) * d_inv_sqrt[cols]   # (d_i * a_ij) * d_j, a_ij = 1
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = cols.astype(np.int32)
    data = data.astype(np.float32)
    if check_symmetric:
        assert_symmetric(indptr, indices, data)
    return indptr, indices, data


def assert_symmetric(indptr, indices, data):
    """A == A^T exactly, pattern and values: the backward pass multiplies by A where autograd would use A^T"""
    N = indptr.size - 1
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr))
    cols = indices.astype(np.int64)
    order = np.argsort(cols * N + rows, kind="stable")     # the transpose's entries in CSR order
    if not (np.array_equal(cols[order], rows) and np.array_equal(rows[order], cols) and np.array_equal(data[order], data)):
        raise AssertionError("normalised adjacency is not exactly symmetric")


def default_chunk(nnz):
    """a quarter of one wave's share of the edges, at least MIN_CHUNK, a multiple of 64"""
    c = max(MIN_CHUNK, int(nnz) // (4 * WAVES_IN_FLIGHT))
    return (c + 63) // 64 * 64


def build_plan(indptr, chunk):
    """the propagation plan of rc_lgcn_graph, as numpy arrays:
      work_row / work_beg / work_len / work_part : one item per row of at most `chunk` edges (part -1: the item writes the row)
                                                   and one per chunk of a longer row (part: its slot of partial sums);
                                                   all items ordered by decreasing length (stable: row order among equals)
      long_row / long_part_ptr                   : rows that were split, and the slots of each one's chunks in chunk order"""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("build_plan: chunk must be >= 1")
    N = indptr.size - 1
    deg = np.diff(indptr).astype(np.int64)
    is_long = deg > chunk
    short = np.nonzero(~is_long)[0]
    long_row = np.nonzero(is_long)[0]
    n_ch = (deg[long_row] + chunk - 1) // chunk
    long_part_ptr = np.zeros(long_row.size + 1, dtype=np.int64)
    np.cumsum(n_ch, out=long_part_ptr[1:])
    n_parts = int(long_part_ptr[-1])
    c_row = np.repeat(long_row, n_ch)
    c_idx = np.arange(n_parts, dtype=np.int64) - np.repeat(long_part_ptr[:-1], n_ch)     # chunk number within its row
    c_beg = indptr[c_row] + c_idx * chunk
    c_len = np.minimum(chunk, deg[c_row] - c_idx * chunk)
    row = np.concatenate([c_row, short])
    beg = np.concatenate([c_beg, indptr[short]])
    ln = np.concatenate([c_len, deg[short]])
    part = np.concatenate([np.arange(n_parts, dtype=np.int64), np.full(short.size, -1, dtype=np.int64)])
    order = np.argsort(-ln, kind="stable")
    assert N < 2 ** 31 and n_parts < 2 ** 31
    return dict(work_row=row[order].astype(np.int32), work_beg=beg[order].astype(np.int64),
                work_len=ln[order].astype(np.int32), work_part=part[order].astype(np.int32),
                long_row=long_row.astype(np.int32), long_part_ptr=long_part_ptr.astype(np.int32), n_parts=n_parts)


GRAPH_KEYS = ("indptr", "indices", "values", "work_row", "work_beg", "work_len", "work_part", "long_row", "long_part_ptr")


def graph_arrays(n_users, n_items, indptr, indices, data, chunk=None):
    """the CSR and its plan as the numpy arrays LgcnGraph wraps (GRAPH_KEYS), plus the chunk length and the partial-slot count"""
    N = int(n_users) + int(n_items)
    if indptr.size != N + 1 or int(indptr[-1]) != indices.size or data.size != indices.size:
        raise ValueError("graph_arrays: indptr does not match the node / edge counts")
    if indices.size and (int(indices.min()) < 0 or int(indices.max()) >= N):
        raise ValueError("graph_arrays: a column id lies outside [0, N)")
    chunk = int(chunk) if chunk else default_chunk(indices.size)
    plan = build_plan(indptr, chunk)
    arrays = dict(indptr=np.asarray(indptr, dtype=np.int64), indices=np.asarray(indices, dtype=np.int32),
                  values=np.asarray(data, dtype=np.float32), **{k: plan[k] for k in GRAPH_KEYS[3:]})
    return arrays, chunk, plan["n_parts"]


class LgcnGraph:
    """the CSR and its plan on one device (tensors named GRAPH_KEYS), the rc_lgcn_graph struct pointing at them, and the persistent
    [N, d] buffers of the products (two ping-pong layers, the partial sums, the forward output): allocated once, so a captured
    training step replays on the same memory"""

    def __init__(self, n_users, n_items, tensors, chunk, n_parts):
        from ._lib import LgcnGraph as _S
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.N = self.n_users + self.n_items
        self.chunk, self.n_parts = int(chunk), int(n_parts)
        self.tensors = {k: tensors[k] for k in GRAPH_KEYS}
        for k, v in self.tensors.items():
            if not v.is_contiguous():
                raise ValueError(f"LgcnGraph: {k} must be contiguous")
        self.nnz = int(self.tensors["indices"].numel())
        self.device = self.tensors["indptr"].device
        self._buffers = {}
        p = lambda x: C.c_void_p(x.data_ptr()) if x.numel() else C.c_void_p(0)
        t = self.tensors
        self.struct = _S(self.n_users, self.n_items, self.nnz, p(t["indptr"]), p(t["indices"]), p(t["values"]),
                         int(t["work_row"].numel()), p(t["work_row"]), p(t["work_beg"]), p(t["work_len"]), p(t["work_part"]),
                         int(t["long_row"].numel()), p(t["long_row"]), p(t["long_part_ptr"]), self.n_parts)

    @classmethod
    def build(cls, n_users, n_items, indptr, indices, data, device, chunk=None):
        arrays, chunk, n_parts = graph_arrays(n_users, n_items, indptr, indices, data, chunk)
        dev = torch.device(device)
        return cls(n_users, n_items, {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}, chunk, n_parts)

    @classmethod
    def from_interactions(cls, n_users, n_items, train_clicked_set, device, chunk=None):
        return cls.build(n_users, n_items, *build_norm_adj(n_users, n_items, train_clicked_set), device=device, chunk=chunk)

    def buffers(self, d):
        """(buf_a, buf_b, partials, out) for tables of width d, created on first use"""
        b = self._buffers.get(d)
        if b is None:
            e = lambda n: torch.empty((max(n, 1), d), dtype=torch.float32, device=self.device)
            b = self._buffers[d] = (e(self.N), e(self.N), e(self.n_parts), e(self.N))
        return b

    def with_chunk(self, chunk):
        """the same graph under another chunk length (tests force splitting on small graphs with it)"""
        t = self.tensors
        return LgcnGraph.build(self.n_users, self.n_items, t["indptr"].cpu().numpy(), t["indices"].cpu().numpy(),
                               t["values"].cpu().numpy(), self.device, chunk=chunk)
