"""CPU: LightGCN's host side against the reference's goldens (tests/golden/make_golden_lightgcn.py) -- the normalised adjacency bit
for bit, the propagation plan's chunk algebra, a float64 restatement of the propagation, the model file's class lookup, flags,
state_dict keys and shape envelope.  No kernel runs here."""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT, assert_close, golden_cases, load_golden

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

CASES = golden_cases("lightgcn_")


def _clicked(g):
    out = {}
    for u, i in zip(g["train_u"].tolist(), g["train_i"].tolist()):
        out.setdefault(u, set()).add(i)
    return out


def _dense_adj(indptr, indices, data):
    import scipy.sparse as sp
    N = indptr.size - 1
    return sp.csr_matrix((data.astype(np.float64), indices, indptr), shape=(N, N))


def propagate64(A, E0, L):
    """the reference's encoder in float64: mean of E_0, A E_0, ..., A^L E_0"""
    acc, e = E0.copy(), E0
    for _ in range(L):
        e = A @ e
        acc = acc + e
    return acc / (L + 1)


def test_golden_cases_exist():
    assert len(CASES) == 5, CASES


@pytest.mark.parametrize("case", CASES)
def test_norm_adj_equals_the_reference_bit_for_bit(case):
    from rechorus_amd import lgcn
    g = load_golden(case)
    n_users, n_items = (int(x) for x in g["meta"][:2])
    indptr, indices, data = lgcn.build_norm_adj(n_users, n_items, _clicked(g))
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
    assert np.array_equal(indptr, g["indptr"]) and np.array_equal(indices, g["indices"])
    assert np.array_equal(data.view(np.uint32), g["data"].view(np.uint32))
    # the same from (users, items) arrays, with repeated interactions counting once (dok_matrix R[u, i] = 1)
    u = np.concatenate([g["train_u"], g["train_u"][:50]])
    i = np.concatenate([g["train_i"], g["train_i"][:50]])
    again = lgcn.build_norm_adj(n_users, n_items, (u, i))
    assert all(np.array_equal(a, b) for a, b in zip(again, (indptr, indices, data)))
    deg = np.diff(indptr)
    assert deg[0] == 0 and deg[n_users] == 0          # row 0 of both tables is an isolated node
    assert deg.max() > lgcn.default_chunk(indices.size)   # an item hub the default plan splits
    lgcn.assert_symmetric(indptr, indices, data)


def test_one_case_has_a_hub_of_degree_1000():
    assert max(int(np.diff(load_golden(c)["indptr"]).max()) for c in CASES) >= 1000


def test_symmetry_check_catches_a_one_ulp_asymmetry():
    from rechorus_amd import lgcn
    g = load_golden(CASES[0])
    data = g["data"].copy()
    data[7] = np.nextafter(data[7], np.float32(1))
    with pytest.raises(AssertionError, match="symmetric"):
        lgcn.assert_symmetric(g["indptr"], g["indices"], data)


@pytest.mark.parametrize("chunk", [1, 3, 64, 500, None])
def test_plan_covers_every_edge_once_in_order(chunk):
    """the chunk algebra restated: direct items are whole rows, the chunks of a long row tile it in order and their partial
    slots are long_part_ptr's range in chunk order; items longest first"""
    from rechorus_amd import lgcn
    g = load_golden(CASES[0])
    indptr = g["indptr"]
    N = indptr.size - 1
    c = chunk or lgcn.default_chunk(indptr[-1])
    plan = lgcn.build_plan(indptr, c)
    row, beg, ln, part = plan["work_row"], plan["work_beg"], plan["work_len"], plan["work_part"]
    assert np.all(np.diff(ln) <= 0)
    deg = np.diff(indptr)
    direct = part < 0
    # every row is written exactly once: by its direct item or by the combine pass of its long row
    written = np.concatenate([row[direct], plan["long_row"]])
    assert np.array_equal(np.sort(written), np.arange(N))
    assert np.array_equal(beg[direct], indptr[row[direct]]) and np.array_equal(ln[direct], deg[row[direct]])
    assert np.all(deg[row[direct]] <= c) and np.all(deg[plan["long_row"]] > c)
    by_part = np.full(plan["n_parts"], -1, dtype=np.int64)
    by_part[part[~direct]] = np.nonzero(~direct)[0]
    assert np.all(by_part >= 0)                        # every slot has exactly one chunk
    lp = plan["long_part_ptr"]
    for j, r in enumerate(plan["long_row"]):
        items = by_part[lp[j]:lp[j + 1]]
        assert np.all(row[items] == r) and np.all(ln[items] <= c) and np.all(ln[items] >= 1)
        edges = np.concatenate([np.arange(beg[k], beg[k] + ln[k]) for k in items])
        assert np.array_equal(edges, np.arange(indptr[r], indptr[r + 1]))
    if chunk == 1:
        assert plan["n_parts"] == indptr[-1] - np.sum(deg[deg <= 1])


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference_forward(case):
    g = load_golden(case)
    L = int(g["meta"][3])
    n_users = int(g["meta"][0])
    A = _dense_adj(g["indptr"], g["indices"], g["data"])
    E0 = np.concatenate([g["U0"], g["I0"]]).astype(np.float64)
    out = propagate64(A, E0, L)
    assert_close(out[:n_users], g["fwd_U"], what=case + " fwd users")
    assert_close(out[n_users:], g["fwd_I"], what=case + " fwd items")
    # the scores of the first batch are dot products of the propagated rows
    U, I = out[:n_users], out[n_users:]
    pred = np.einsum("bd,bcd->bc", U[g["uid"]], I[g["iid"]])
    assert_close(pred, g["pred"], what=case + " pred")


@pytest.mark.parametrize("L", [0, 1, 3, 8])
def test_horner_backward_is_the_adjoint_of_the_forward(L):
    """sum_l A^l G / (L+1) in Horner form (what rc_lgcn_propagate_bwd computes) is the adjoint of the forward: <f(E), G> = <E, b(G)>"""
    g = load_golden(CASES[0])
    A = _dense_adj(g["indptr"], g["indices"], g["data"])
    rng = np.random.default_rng(L)
    E, G = rng.normal(size=(A.shape[0], 8)), rng.normal(size=(A.shape[0], 8))
    h = G / (L + 1)
    for _ in range(L):
        h = A @ h + G / (L + 1)
    lhs = np.sum(propagate64(A, E, L) * G)
    rhs = np.sum(E * h)
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def _args(**kw):
    a = dict(device="cpu", model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=64, n_layers=3)
    a.update(kw)
    return SimpleNamespace(**a)


def test_class_lookup_and_flags():
    import main
    cls = main.find_class("model", ("LightGCN", ""))
    imp = main.find_class("model", ("LightGCN", "Impression"))
    assert cls.__name__ == "LightGCN" and imp.__name__ == "LightGCNImpression"
    assert (cls.reader, cls.runner) == ("BaseReader", "BaseRunner")
    assert (imp.reader, imp.runner) == ("ImpressionReader", "ImpressionRunner")
    assert cls.extra_log_args == ["emb_size", "n_layers", "batch_size"] == imp.extra_log_args
    assert cls.candidate_permutation_equivariant and not hasattr(cls, "hip_train_step")
    a, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args(
        ["--emb_size", "64", "--n_layers", "3", "--num_neg", "1", "--test_all", "1"])
    assert (a.emb_size, a.n_layers, a.num_neg, a.test_all) == (64, 3, 1, 1)
    d, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
    assert (d.emb_size, d.n_layers) == (64, 3)
    a, _ = imp.parse_model_args(argparse.ArgumentParser()).parse_known_args(["--n_layers", "2", "--loss_n", "BPR"])
    assert a.n_layers == 2 and a.loss_n == "BPR"


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_and_init_match_the_reference(case):
    import torch
    from models.general.LightGCN import LightGCN
    g = load_golden(case)
    n_users, n_items, d, L, _, _, seed = (int(x) for x in g["meta"])
    torch.manual_seed(seed)
    m = LightGCN(_args(emb_size=d, n_layers=L), SimpleNamespace(n_users=n_users, n_items=n_items, train_clicked_set=_clicked(g)))
    assert sorted(m.state_dict().keys()) == sorted(g["state_keys"].tolist())
    # the same RNG stream as the reference's construction: xavier_uniform user table, then item table
    assert np.array_equal(m.encoder.embedding_dict["user_emb"].detach().numpy(), g["U0"])
    assert np.array_equal(m.encoder.embedding_dict["item_emb"].detach().numpy(), g["I0"])
    # the CSR and its plan are buffers that follow the module, not checkpoint entries
    assert "encoder.adj_indptr" in dict(m.named_buffers()) and "encoder.adj_indptr" not in m.state_dict()


@pytest.mark.parametrize("d,L", [(30, 3), (2, 1), (260, 3), (64, 9), (64, -1)])
def test_envelope_raises_in_init(d, L):
    from models.general.LightGCN import LightGCN
    corpus = SimpleNamespace(n_users=5, n_items=6, train_clicked_set={1: {2, 3}, 2: {3}})
    with pytest.raises(ValueError, match="envelope"):
        LightGCN(_args(emb_size=d, n_layers=L), corpus)


def test_check_shape_reports_the_envelope():
    """rc_lgcn_check_shape is host logic: RC_OK inside the envelope, RC_ERR_UNSUPPORTED with the reason outside it"""
    from rechorus_amd import _lib, engine
    lib = _lib.load()
    for d, L, n, nnz in ((4, 0, 0, 0), (256, 8, 2 ** 31 - 1, 2 ** 31 - 1), (48, 3, 10, 10), (64, 3, 10, 0)):
        assert lib.rc_lgcn_check_shape(d, L, n, nnz) == _lib.RC_OK, (d, L, n, nnz)
        engine.lgcn_check_shape(d, L, n, nnz)
    for d, L, n, nnz in ((0, 3, 10, 10), (2, 3, 10, 10), (30, 3, 10, 10), (260, 3, 10, 10), (64, 9, 10, 10), (64, -1, 10, 10),
                         (64, 3, 2 ** 31, 10), (64, 3, 10, 2 ** 31), (64, 3, -1, 10)):
        assert lib.rc_lgcn_check_shape(d, L, n, nnz) == -4, (d, L, n, nnz)      # RC_ERR_UNSUPPORTED
        assert b"outside the envelope" in lib.rc_last_error_string()
        with pytest.raises(ValueError, match="envelope"):
            engine.lgcn_check_shape(d, L, n, nnz)


def test_entry_points_refuse_a_shape_outside_the_envelope_without_a_gpu():
    """the propagation entry points check the envelope themselves, before any launch"""
    import ctypes as C
    from rechorus_amd import _lib
    lib = _lib.load()
    g = _lib.LgcnGraph(3, 4, 0, *([None] * 3), 0, *([None] * 4), 0, None, None, 0)
    p = C.c_void_p(256)
    assert lib.rc_lgcn_propagate_fwd(C.byref(g), p, p, 30, 3, p, p, p, p, None) == -4
    assert lib.rc_lgcn_propagate_bwd(C.byref(g), p, p, 64, 9, p, p, p, p, p, None) == -4
    assert lib.rc_lgcn_propagate_fwd(None, p, p, 64, 3, p, p, p, p, None) == -1
    assert b"null pointer" in lib.rc_last_error_string()


def test_envelope_edges_build():
    from models.general.LightGCN import LightGCN
    corpus = SimpleNamespace(n_users=5, n_items=6, train_clicked_set={1: {2, 3}, 2: {3}})
    for d, L in ((4, 0), (256, 8), (48, 2)):
        m = LightGCN(_args(emb_size=d, n_layers=L), corpus)
        assert m.encoder.embedding_dict["item_emb"].shape == (6, d)


def test_no_torch_sparse_in_the_package():
    hits = []
    for base, _, files in os.walk(os.path.join(ROOT, "rechorus_amd")):
        for f in files:
            if f.endswith(".py"):
                p = os.path.join(base, f)
                if "torch.sparse" in open(p).read():
                    hits.append(p)
    assert not hits, hits


def test_lgcn_kernels_use_no_float_atomics():
    import re
    src = open(os.path.join(ROOT, "rechorus_amd", "csrc", "lgcn.hip")).read()
    assert not re.search(r"atomic\w*\s*\(|__hip_atomic|__atomic", src)
