"""GPU: every kernel at the edges of the shape envelope it declares (the rc_*_supported predicates, tests/envelopes.py).  The
largest accepted value of a bounded dimension is found by scanning the predicate, so the tests follow the code: max + 1 must be
refused, max runs forward and backward against a float64 restatement of the same operation, and where the engine reroutes
max + 1 (BPRMF's generic fall-back) that shape runs too.  Batch sizes are ragged and update / row-sum inputs repeat ids."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close, assert_update_close
import envelopes as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(cuda):
    from rechorus_amd import engine
    return engine


@pytest.fixture(scope="module")
def lib(cuda):
    from rechorus_amd import _lib
    return _lib.load()


def scan_max(ok, lo, hi):
    """largest v in [lo, hi] the predicate accepts, scanning up from lo (which it must accept) until it refuses"""
    assert ok(lo), ("the predicate refuses its smallest shape", lo)
    v = lo
    while v < hi and ok(v + 1):
        v += 1
    assert v < hi, ("the scan reached its bound: widen it", hi)
    return v


def t(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bpr_rows64(pred):
    """models/BaseModel.py:182-185 in float64, per row (before the mean): global max of the negatives, softmax, clamp, log"""
    pos, neg = pred[:, 0], pred[:, 1:]
    w = (neg - neg.max()).softmax(dim=1)
    return -(((pos[:, None] - neg).sigmoid() * w).sum(dim=1)).clamp(min=1e-8, max=1 - 1e-8).log()


# ---- BPRMF fused forward + backward ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", E.BPRMF_FUSED_D)
def test_bprmf_fused_at_the_largest_candidate_count(d, cuda, eng, lib):
    """rc_bprmf_fwd_bwd at the largest C of the register path (its last (GS, CPL) tiling) and at max + 1 (the generic kernel):
    pred, loss rows, d pred and the user-row gradient against autograd in float64"""
    Cmax = scan_max(lambda C: lib.rc_bprmf_fused_supported(d, C), 2, 1 << 14)
    assert not lib.rc_bprmf_fused_supported(d, Cmax + 1)
    rng = np.random.default_rng(d)
    n_users, n_items = 23, 3 * Cmax
    U = rng.normal(0, 1.0 / d ** 0.5, (n_users, d)).astype(np.float32) * 2
    I = rng.normal(0, 1.0, (n_items, d)).astype(np.float32)
    for C in (Cmax, Cmax + 1):
        B = 37
        uid = rng.integers(0, n_users, B).astype(np.int64)
        uid[:5] = 4                                   # a repeated user
        iid = rng.integers(0, n_items, (B, C)).astype(np.int64)
        iid[:, 1] = 9                                 # a repeated item
        pred, loss_vec, gpred, ugrad = eng.bprmf_fwd_bwd(*(t(a, cuda) for a in (U, I, uid, iid)))
        u = torch.from_numpy(U[uid]).double().requires_grad_(True)
        p64 = (u[:, None, :] * torch.from_numpy(I[iid]).double()).sum(-1)
        p64.retain_grad()
        rows = _bpr_rows64(p64)
        rows.mean().backward()
        what = f"d={d} C={C}"
        assert_close(pred.cpu().numpy(), p64.detach().numpy(), what="pred " + what)
        assert_close(loss_vec.cpu().numpy(), rows.detach().numpy(), what="loss rows " + what, atol_scale=2e-5)
        assert_close(gpred.cpu().numpy(), p64.grad.numpy(), what="d pred " + what, atol_scale=2e-5)
        assert_close(ugrad.cpu().numpy(), u.grad.numpy(), what="user rows " + what, atol_scale=2e-5)


# ---- NeuMF fused training step at its LDS bound ---------------------------------------------------------------------------------

NEUMF_KEYS = ("mf_u_embeddings.weight", "mf_i_embeddings.weight", "mlp_u_embeddings.weight", "mlp_i_embeddings.weight", "mlp.0.weight",
              "mlp.0.bias", "prediction.weight")


def _neumf_problem(rng, n_users, n_items, d, l1):
    P = {"mf_u_embeddings.weight": rng.normal(0, 0.3, (n_users, d)), "mf_i_embeddings.weight": rng.normal(0, 0.3, (n_items, d)),
         "mlp_u_embeddings.weight": rng.normal(0, 0.3, (n_users, d)), "mlp_i_embeddings.weight": rng.normal(0, 0.3, (n_items, d)),
         "mlp.0.weight": rng.normal(0, 0.2, (l1, 2 * d)), "mlp.0.bias": rng.normal(0, 0.2, l1),
         "prediction.weight": rng.normal(0, 0.2, (1, d + l1))}
    return {k: v.astype(np.float32) for k, v in P.items()}


def _neumf64(P, uid, iid):
    """models/general/NeuMF.py:56-76 (one hidden layer, no dropout) + the BPR loss of models/BaseModel.py:182-185 in float64 autograd
    -> (pred [B, C], loss rows [B], dense gradient of every parameter of the mean loss)"""
    T = {k: torch.from_numpy(P[k]).double().requires_grad_(True) for k in NEUMF_KEYS}
    u, i = torch.from_numpy(uid), torch.from_numpy(iid)
    B, C = iid.shape
    mf = T["mf_u_embeddings.weight"][u][:, None, :] * T["mf_i_embeddings.weight"][i]
    mlp_u = T["mlp_u_embeddings.weight"][u][:, None, :].expand(B, C, -1)
    h = torch.relu(torch.cat([mlp_u, T["mlp_i_embeddings.weight"][i]], dim=-1) @ T["mlp.0.weight"].T + T["mlp.0.bias"])
    pred = (torch.cat([mf, h], dim=-1) @ T["prediction.weight"].T).view(B, C)
    rows = _bpr_rows64(pred)
    rows.mean().backward()
    return pred.detach().numpy(), rows.detach().numpy(), {k: T[k].grad.numpy() for k in NEUMF_KEYS}


def test_neumf_fused_step_at_the_lds_bound(cuda, eng, lib, monkeypatch):
    """rc_neumf_train_step at the largest C whose LDS image fits, for every (d, l1) the step has a kernel for: predictions, loss rows,
    dense gradients, user rows, the row-wise update of single-occurrence item rows and the gradient rows of hot ones, against a
    float64 autograd restatement (through the checks of the fused-step tests).  C = max + 1 goes to the three-kernel step through
    NeumfTrainer where that step has the tower: one SGD step against the float64 gradients."""
    from test_gpu_neumf import NAMES, _check_fused_against, _state_for, to_dev
    rng = np.random.default_rng(21)
    shapes = [(d, l1) for d in (32, 64, 128) for l1 in (16, 32, 64) if lib.rc_neumf_train_step_supported(2, d, l1)]
    assert len(shapes) == 8, shapes
    rerouted = 0
    for j, (d, l1) in enumerate(shapes):
        Cmax = scan_max(lambda C: lib.rc_neumf_train_step_supported(C, d, l1), 2, 4096)
        assert not lib.rc_neumf_train_step_supported(Cmax + 1, d, l1)
        opt = ("SGD", "Adam", "Adagrad")[j % 3]
        n_users, n_items, B = 29, 5000, 67
        P = _neumf_problem(rng, n_users, n_items, d, l1)
        uid = rng.integers(0, n_users, size=B).astype(np.int64)
        iid = rng.integers(0, n_items, size=(B, Cmax)).astype(np.int64)
        iid[:, 0] = iid[:, 0] % 5      # hot positives
        Pd = to_dev(P, cuda)
        pred, rows, G = _neumf64(P, uid, iid)
        state = _state_for(eng, Pd, opt, rng, cuda)
        _check_fused_against(eng, P, Pd, state, uid, iid, opt, 0.03, 1e-4, 2, pred, rows, G, 2e-5, cuda, f"d={d} l1={l1} B={B} C={Cmax} {opt}")
        if not eng.neumf_supported(d, l1):
            continue                   # (hidden 16: a tower of the one-kernel step only; NeumfTrainer refuses C = max + 1 there)
        rerouted += 1
        C = Cmax + 1
        iid = rng.integers(0, n_items, size=(B, C)).astype(np.int64)
        iid[:, 0] = iid[:, 0] % 5
        _, rows, G = _neumf64(P, uid, iid)
        Pd = to_dev(P, cuda)
        lr = 0.05
        tr = eng.NeumfTrainer(Pd, opt="SGD", lr=lr, l2=0.0, rowwise=True)
        tr.timing = {}
        loss = float(tr.step(torch.from_numpy(uid).to(cuda), torch.from_numpy(iid).to(cuda)).item())
        what = f"three-kernel step d={d} l1={l1} B={B} C={C}"
        assert "fused_step" not in tr.timing, what
        assert_close(loss, rows.mean(), what=what + " loss")
        for k, name in NAMES.items():      # SGD without weight decay: the row-wise step of the touched rows is the dense step
            W0 = P[name].reshape(Pd[k].shape)
            assert_update_close(Pd[k].cpu().numpy(), W0, W0 - lr * G[name].reshape(W0.shape), what=what + " " + k)
    assert rerouted >= 6, rerouted


# ---- NeuMF z-head (sharded step's home rank) --------------------------------------------------------------------------------------

def test_neumf_zhead_at_its_envelope(cuda, eng, lib):
    """engine.neumf_zhead at the largest C, the widest d = l1, the narrowest d = l1 = 1 and odd widths: loss rows, predictions, both
    gradient blocks and the dense gradients against autograd in float64"""
    Cmax = scan_max(lambda C: lib.rc_neumf_zhead_supported(C, 8, 8), 2, 1 << 14)
    dmax = scan_max(lambda w: lib.rc_neumf_zhead_supported(2, w, 8), 1, 1 << 14)
    lmax = scan_max(lambda w: lib.rc_neumf_zhead_supported(2, 8, w), 1, 1 << 14)
    assert not lib.rc_neumf_zhead_supported(Cmax + 1, 8, 8) and not lib.rc_neumf_zhead_supported(2, dmax + 1, 8)
    assert not lib.rc_neumf_zhead_supported(2, 8, lmax + 1) and lib.rc_neumf_zhead_supported(Cmax, dmax, lmax)
    rng = np.random.default_rng(31)
    for B, C, d, l1 in E.ZHEAD_SHAPES:
        C, d, l1 = C or Cmax, d or dmax, l1 or lmax
        assert lib.rc_neumf_zhead_supported(C, d, l1)
        mk = lambda *s, sd=0.4: rng.normal(0, sd, s).astype(np.float32)
        urows, irows = mk(B, 2 * d), mk(B * C, d + l1)
        W1, b1, w_out = mk(l1, 2 * d, sd=0.4 / d ** 0.5), mk(l1), mk(d + l1, sd=1.0 / (d + l1) ** 0.5)
        got = eng.neumf_zhead(t(urows, cuda), t(irows, cuda), t(W1, cuda), t(b1, cuda), t(w_out, cuda), B, C, 1.0 / B, want_pred=True)
        u64, i64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (urows, irows))
        W1u = torch.from_numpy(W1[:, :d]).double().requires_grad_(True)
        b64, w64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (b1, w_out))
        mf_u, mlp_u = u64[:, :d], u64[:, d:]
        mf_i, zi = i64[:, :d].reshape(B, C, d), i64[:, d:].reshape(B, C, l1)
        h = torch.relu((mlp_u @ W1u.T + b64)[:, None, :] + zi)
        p64 = (mf_u[:, None, :] * mf_i * w64[:d]).sum(-1) + (h * w64[d:]).sum(-1)
        rows = _bpr_rows64(p64)
        rows.mean().backward()
        what = f"B={B} C={C} d={d} l1={l1}"
        n = (B * C) ** 0.5
        assert_close(got[0].cpu().numpy(), rows.detach().numpy(), what="loss rows " + what, atol_scale=2e-5)
        assert_close(got[4].cpu().numpy(), p64.detach().numpy(), what="pred " + what)
        assert_close(got[1].cpu().numpy(), u64.grad.numpy(), what="gu " + what, atol_scale=2e-5)
        assert_close(got[2].cpu().numpy(), i64.grad.numpy(), what="gi " + what, atol_scale=2e-5)
        for k, ref in (("W1u", W1u.grad), ("b1", b64.grad), ("w_out", w64.grad)):
            assert_close(got[3][k].cpu().numpy(), ref.numpy(), what="d" + k + " " + what, rtol=2e-5, atol_scale=2e-5, abs_floor=3e-7 * n)


# ---- sequence attention at the longest history ------------------------------------------------------------------------------------

def _attention64(q, k, v, H, full):
    B, L, D = q.shape
    dk = D // H
    split = lambda x: x.view(B, L, H, dk).transpose(1, 2)
    s = split(q) @ split(k).transpose(-2, -1) / dk ** 0.5
    s = s.masked_fill(~full, float("-inf"))
    p = (s - s.max()).softmax(dim=-1)
    p = p.masked_fill(torch.isnan(p), 0)
    return (p @ split(v)).transpose(1, 2).reshape(B, L, D)


@pytest.mark.parametrize("H,dk", E.SEQ_ATTENTION_HEADS)
def test_seq_attention_at_the_longest_history(H, dk, cuda, eng, lib):
    """rc_seq_attention_fwd / _bwd, causal, at the largest L with sequence lengths {1, L - 1, L, > L}: ctx, dQ, dK, dV against
    autograd in float64"""
    Lmax = scan_max(lambda L: lib.rc_seq_attention_supported(L, 1), 1, 1 << 14)
    dkmax = scan_max(lambda w: lib.rc_seq_attention_supported(1, w), 1, 1 << 14)
    assert not lib.rc_seq_attention_supported(Lmax + 1, 1) and not lib.rc_seq_attention_supported(1, dkmax + 1)
    dk = dk or dkmax
    L, B, D = Lmax, 4, H * dk
    assert eng.seq_attention_supported(L, dk)
    rng = np.random.default_rng(L + dk)
    mk = lambda: torch.from_numpy(rng.normal(0, 1.0, (B, L, D)).astype(np.float32)).to(cuda)
    q, k, v, w = mk(), mk(), mk(), mk()
    lengths = torch.tensor([1, L - 1, L, L + 37], dtype=torch.int64, device=cuda)
    off = eng.seq_offsets(lengths, L)
    eff = lengths.clamp(max=L)
    assert off.cpu().tolist() == [0] + np.cumsum(eff.cpu().numpy()).tolist()
    valid = torch.arange(L, device=cuda)[None, :] < eff[:, None]
    full = torch.tril(torch.ones((L, L), dtype=torch.bool, device=cuda))[None, None] & valid[:, None, None, :]
    q64, k64, v64 = (x.double().requires_grad_(True) for x in (q, k, v))
    want = _attention64(q64, k64, v64, H, full) * valid[:, :, None]
    (want * w.double()).sum().backward()
    qf, kf, vf = (x.reshape(B * L, D).contiguous() for x in (q, k, v))
    ctx, lse = eng.seq_attention_fwd(qf, kf, vf, off, B, L, H, causal=True)
    got = ctx.view(B, L, D)[valid]
    assert_close(got.cpu().numpy(), want[valid].detach().cpu().numpy(), what=f"ctx L={L} dk={dk}")
    dctx = (w * valid[:, :, None]).reshape(B * L, D).contiguous()
    dQ, dK, dV = eng.seq_attention_bwd(qf, kf, vf, off, B, L, H, lse, dctx, causal=True)
    for name, g, ref in (("dQ", dQ, q64.grad), ("dK", dK, k64.grad), ("dV", dV, v64.grad)):
        assert_close(g.view(B, L, D)[valid].cpu().numpy(), ref[valid].cpu().numpy(), what=f"{name} L={L} dk={dk}", rtol=2e-5, atol_scale=2e-5)


# ---- impression list metrics at the widest list -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mp_rule", E.LIST_METRICS_MAX_POS)
def test_list_metrics_at_the_widest_list(mp_rule, cuda, eng, lib):
    """rc_list_metrics at the largest n with max_pos = n (the fullest LDS carve) and n / 2, with the most values of k, against the
    mirror's numpy evaluate_method at 1e-12"""
    plugin = os.path.join(ROOT, "rechorus_amd", "rechorus")
    if plugin not in sys.path:
        sys.path.insert(0, plugin)
    from helpers.ImpressionRunner import ImpressionRunner
    from test_gpu_impression import _device_metrics
    nmax = scan_max(lambda n: lib.rc_list_metrics_supported(n, n, 1), 1, 1 << 14)
    kmax = scan_max(lambda k: lib.rc_list_metrics_supported(8, 4, k), 1, 1024)
    assert not lib.rc_list_metrics_supported(nmax + 1, 0, 1) and not lib.rc_list_metrics_supported(8, 4, kmax + 1)
    assert not lib.rc_list_metrics_supported(nmax, nmax + 1, 1)
    n = nmax
    mp = n if mp_rule == "n" else n // 2
    assert lib.rc_list_metrics_supported(n, mp, kmax)
    rng = np.random.default_rng(mp)
    N = 67
    pred = rng.choice(np.linspace(-2, 2, 41).astype(np.float32), size=(N, n))          # ties inside and across the groups
    pos = rng.integers(0, mp + 3, size=N)
    pos[:4] = (mp, mp - 1, 1, 0)
    neg = rng.integers(0, n - mp + 3, size=N)
    topk = sorted({1, 2, 3, 5, 10, 20, 50, 100, 500, 1000, 1023, 1024, 1025, 2047, n, n + 5})[:kmax]
    assert len(topk) == kmax
    col = np.arange(n)[None, :]
    keep = (col < np.minimum(pos, mp)[:, None]) | ((col >= mp) & (col < mp + np.minimum(neg, n - mp)[:, None]))
    want = ImpressionRunner.evaluate_method(np.where(keep, pred, -np.inf), topk, [], False, neg, mp, pos, ret_all=1)
    dirty = np.where(keep, pred, np.float32(1e30))
    per_row, mean = _device_metrics(dirty, pos, neg, mp, topk, cuda)
    for m, name in enumerate(("NDCG", "MAP", "HR")):
        for j, k in enumerate(topk):
            wv = want["%s@%d" % (name, k)]
            assert np.allclose(per_row[:, m, j], wv, atol=1e-12, rtol=0), (mp, name, k, np.abs(per_row[:, m, j] - wv).max())
            assert abs(mean[m, j] - wv.mean()) < 1e-12


# ---- MLP tower tail: every accepted (K, N2) ---------------------------------------------------------------------------------------

def _tail_pairs():
    from rechorus_amd import _lib
    lib = _lib.load()
    return [(K, N2) for K in range(1, 1025) for N2 in range(1, 129) if lib.rc_tower_tail_supported(1, K, N2)]


def test_tower_tail_every_accepted_pair(cuda, eng, lib):
    """rc_tower_tail_fwd / _bwd at every (K, N2) the predicate accepts (found by scanning K <= 1024, N2 <= 128), a ragged M, bias and a
    dropout-free ReLU input: H2, z, dX, dW2, db2, dW3, db3 against oracle/mlp_oracle.py (float64)"""
    from oracle import mlp_oracle as MO
    pairs = _tail_pairs()
    Ks, Ns = sorted({K for K, _ in pairs}), sorted({N for _, N in pairs})
    assert len(pairs) == len(Ks) * len(Ns) == 12, pairs
    assert not lib.rc_tower_tail_supported(1, max(Ks) + 1, max(Ns)) and not lib.rc_tower_tail_supported(1, max(Ks), max(Ns) + 1)
    M = 333
    rng = np.random.default_rng(41)
    for K, N2 in pairs:
        X = np.where(rng.random((M, K)) < 0.45, 0.0, np.abs(rng.normal(0, 0.5, (M, K)))).astype(np.float32)
        W2 = rng.normal(0, 1.0 / K ** 0.5, (N2, K)).astype(np.float32)
        b2 = rng.normal(0, 0.1, N2).astype(np.float32)
        W3 = rng.normal(0, 0.3, (1, N2)).astype(np.float32)
        b3 = rng.normal(0, 0.1, 1).astype(np.float32)
        dz = rng.normal(0, 1.0, (M, 1)).astype(np.float32)
        H2o, _ = MO.linear_fwd(X, W2, b2, True, None)
        zo, _ = MO.linear_fwd(H2o, W3, b3, False)
        dZ2o, dW3o, db3o = MO.linear_bwd_chain(H2o, W3, dz, x_mask=H2o > 0, x_scale=1.0)
        dXo, dW2o, db2o = MO.linear_bwd_chain(X, W2, dZ2o, x_mask=X > 0, x_scale=1.0)
        assert eng.tower_tail_supported(M, K, N2)
        H2, z = eng.tower_tail_fwd(t(X, cuda), t(W2, cuda), t(b2, cuda), t(W3, cuda), t(b3, cuda))
        what = f" K={K} N2={N2}"
        assert_close(H2.cpu().numpy(), H2o, what="H2" + what, rtol=2e-5, atol_scale=2e-5)
        assert_close(z.cpu().numpy(), zo, what="z" + what, rtol=2e-5, atol_scale=2e-5)
        dX, dW2, db2, dW3, db3 = eng.tower_tail_bwd(t(X, cuda), t(W2, cuda), t(W3, cuda), t(H2o.astype(np.float32), cuda), t(dz, cuda), 0.0,
                                                    need_dx=True, x_act=True, x_drop_p=0.0, need_db2=True, need_db3=True)
        for name, g, ref in (("dX", dX, dXo), ("dW2", dW2, dW2o), ("db2", db2, db2o), ("dW3", dW3, dW3o), ("db3", db3, db3o)):
            assert_close(g.cpu().numpy(), ref, what=name + what, rtol=2e-5, atol_scale=2e-5)


# ---- small-list row sums at the longest list --------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", E.SMALL_ROW_SUMS_D)
def test_small_row_sums_at_the_longest_list_with_a_hot_row(d, cuda, eng, lib, monkeypatch):
    """embedding_dense_backward on the small-list route (rc_small_row_sums) at the largest n, one id holding most of the positions:
    against a float64 index_add; n + 1 is refused"""
    n_rows = 70_001
    nmax = scan_max(lambda n: lib.rc_small_row_sums_supported(n, n_rows, d), 1, 1 << 17)
    assert not lib.rc_small_row_sums_supported(nmax + 1, n_rows, d)
    rng = np.random.default_rng(nmax + d)
    ids = rng.integers(0, n_rows, size=nmax).astype(np.int64)
    ids[rng.permutation(nmax)[:nmax * 3 // 4]] = n_rows // 3          # the hot row
    ids[-3:] = n_rows - 1                                              # a short run at the end, the last row
    src = rng.normal(size=(nmax, d)).astype(np.float32)
    want = np.zeros((n_rows, d), np.float64)
    np.add.at(want, ids, src.astype(np.float64))
    monkeypatch.setattr(eng, "_EDB_SMALL", True)
    monkeypatch.setattr(eng, "_EDB_SMALL_MAX", nmax)
    assert eng.small_route_ok(nmax, n_rows, d)
    G = eng.embedding_dense_backward(t(src, cuda), t(ids, cuda), n_rows, route="small").cpu().numpy()
    cnt = np.bincount(ids, minlength=n_rows)
    hot = cnt > 32
    # the hot row against its own scale, every other touched row against theirs (one scale for both would hide the short rows)
    assert_close(G[hot], want[hot], what=f"hot row d={d}", rtol=2e-5, atol_scale=2e-5)
    assert_close(G[~hot & (cnt > 0)], want[~hot & (cnt > 0)], what=f"other rows d={d}", rtol=2e-5, atol_scale=2e-5)
    assert np.all(G[cnt == 0] == 0)


# ---- SASRec encoders: narrow heads at the most layers, and the block-by-block route at the longest history -----------------------

SAS_LAYER_KEYS = {"Wq": "masked_attn_head.q_linear.weight", "bq": "masked_attn_head.q_linear.bias",
                  "Wk": "masked_attn_head.k_linear.weight", "bk": "masked_attn_head.k_linear.bias",
                  "Wv": "masked_attn_head.v_linear.weight", "bv": "masked_attn_head.v_linear.bias",
                  "ln1w": "layer_norm1.weight", "ln1b": "layer_norm1.bias", "W1": "linear1.weight", "b1": "linear1.bias",
                  "W2": "linear2.weight", "b2": "linear2.bias", "ln2w": "layer_norm2.weight", "ln2b": "layer_norm2.bias"}


def _sasrec64(P, hist, lengths, n_layers, n_heads, dhv):
    """models/sequential/SASRec.py:58-76 with utils/layers.py's attention (global-max shift, NaN -> 0) and transformer layer, no
    dropout, in float64 autograd; backward of sum(hv * dhv) -> (hv [B, d], {parameter name: gradient})"""
    T = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in P.items()}
    hist_t, len_t = torch.from_numpy(hist), torch.from_numpy(lengths)
    B, L = hist.shape
    d = T["i_embeddings.weight"].shape[1]
    dk = d // n_heads
    valid = (hist_t > 0).long()
    position = (len_t[:, None] - torch.arange(L)[None, :]) * valid
    x = T["i_embeddings.weight"][hist_t] + T["p_embeddings.weight"][position]
    causal = torch.tril(torch.ones((L, L), dtype=torch.bool))
    split = lambda y: y.view(B, L, n_heads, dk).transpose(1, 2)
    for l in range(n_layers):
        p = lambda name: T["transformer_block.%d.%s" % (l, name)]
        lin = lambda y, name: y @ p(name + ".weight").T + p(name + ".bias")
        q, k, v = (split(lin(x, "masked_attn_head.%s_linear" % c)) for c in "qkv")
        s = (q @ k.transpose(-2, -1) / dk ** 0.5).masked_fill(~causal, float("-inf"))
        a = (s - s.max()).softmax(dim=-1)
        ctx = (a.masked_fill(torch.isnan(a), 0) @ v).transpose(1, 2).reshape(B, L, d)
        y1 = torch.nn.functional.layer_norm(ctx + x, (d,), p("layer_norm1.weight"), p("layer_norm1.bias"))
        f = lin(torch.relu(lin(y1, "linear1")), "linear2")
        x = torch.nn.functional.layer_norm(f + y1, (d,), p("layer_norm2.weight"), p("layer_norm2.bias"))
    x = x * valid[:, :, None]
    hv = x[torch.arange(B), len_t - 1]
    (hv * torch.from_numpy(dhv).double()).sum().backward()
    return hv.detach().numpy(), {k: t.grad.numpy() for k, t in T.items()}


@pytest.mark.parametrize("impl", ["sequence", "batch"])
@pytest.mark.parametrize("d,n_heads", E.SASREC_CORE_HEADS)
def test_sasrec_core_encoders_at_the_most_heads_and_layers(d, n_heads, impl, cuda, eng, lib):
    """rc_sasrec_fwd / _bwd (per-sequence and batch encoders) with d_k = d / n_heads down to 1, the most layers and the largest L
    the core path takes (found by scanning rc_sasrec_supported), lengths {1, L - 1, L} and ragged B: the output rows, every
    layer's parameter gradients and the position- and item-table gradients against a float64 autograd restatement"""
    from test_gpu_sasrec import _random_sasrec, to_dev
    n_layers = scan_max(lambda n: lib.rc_sasrec_supported(d, n, n_heads, 8), 1, 64)
    L = scan_max(lambda L: lib.rc_sasrec_supported(d, n_layers, n_heads, L), 1, 4096)
    assert not lib.rc_sasrec_supported(d, n_layers + 1, n_heads, 8) and not lib.rc_sasrec_supported(d, n_layers, n_heads, L + 1)
    assert lib.rc_sasrec_supported(d, n_layers, n_heads, L) and (n_heads == d or not lib.rc_sasrec_supported(d, 1, d + 1, 8))
    rng = np.random.default_rng(d * 100 + n_heads)
    B, n_items = 37, 300
    P = _random_sasrec(rng, n_items, d, n_layers, L)
    lengths = rng.integers(1, L + 1, size=B).astype(np.int64)
    lengths[:4] = (1, L - 1, L, L)
    hist = rng.integers(1, n_items, size=(B, L)).astype(np.int64) * (np.arange(L)[None, :] < lengths[:, None])
    hist[2, :] = 7                                             # a repeated item
    dhv = rng.normal(size=(B, d)).astype(np.float32)
    Pd = to_dev(P, n_layers, cuda)
    h_d, l_d = (torch.from_numpy(x).to(cuda) for x in (hist, lengths))
    hv, xsave = eng.sasrec_fwd(Pd["item_emb"], Pd["pos_emb"], Pd["layers"], n_heads, h_d, l_d, save=True, impl=impl)
    hv64, G = _sasrec64(P, hist, lengths, n_layers, n_heads, dhv)
    what = f"d={d} heads={n_heads} layers={n_layers} L={L} {impl}"
    assert_close(hv.cpu().numpy(), hv64, what="hv " + what, rtol=2e-5, atol_scale=2e-5)
    g_hist, dg = eng.sasrec_bwd(Pd["layers"], n_heads, l_d, xsave, t(dhv, cuda))
    floor = 1e-6 * max(float(np.abs(v).max()) for v in G.values())
    for l in range(n_layers):
        for k, name in SAS_LAYER_KEYS.items():
            assert_close(dg[l][k].cpu().numpy(), G["transformer_block.%d.%s" % (l, name)], what=f"{what} layer {l} d{k}",
                         rtol=2e-5, atol_scale=2e-5, abs_floor=floor)
    valid = (h_d > 0).to(torch.int64)
    position = ((l_d[:, None] - torch.arange(L, device=cuda)[None, :]) * valid).contiguous()
    GP = eng.embedding_dense_backward(g_hist, position, Pd["pos_emb"].shape[0])
    assert_close(GP.cpu().numpy()[1:], G["p_embeddings.weight"][1:], what="d pos_emb " + what, rtol=2e-5, atol_scale=2e-5, abs_floor=floor)
    GI = eng.embedding_dense_backward(g_hist, h_d, n_items)
    assert_close(GI.cpu().numpy()[1:], G["i_embeddings.weight"][1:], what="d item_emb " + what, rtol=2e-5, atol_scale=2e-5, abs_floor=floor)


def test_sasrec_encode_layers_at_the_longest_history(cuda, eng):
    """nn.sasrec_encode_layers -- embeddings, rc_linear_* projections and feed-forward, rc_seq_attention, LayerNorm(residual), the
    pick of the last valid row -- at the longest history its attention takes (found by scanning rc_seq_attention_supported), two
    blocks, lengths {1, L - 1, L}: the output rows and the gradients of the item table, the position table and every block parameter
    against a float64 autograd restatement"""
    from oracle.torch_port import _TransformerLayer
    from rechorus_amd import nn as hnn
    from test_gpu_sasrec import _random_sasrec
    d, n_heads, n_layers, n_items = 64, 2, 2, 300
    L = scan_max(lambda L: eng.seq_attention_supported(L, d // n_heads), 1, 1 << 14)
    assert hnn.sasrec_layers_supported(d, n_heads, L) and not hnn.sasrec_layers_supported(d, n_heads, L + 1)
    assert not eng.sasrec_supported(d, n_layers, n_heads, L)          # (the register-resident encoders do not take it)
    rng = np.random.default_rng(L)
    P = _random_sasrec(rng, n_items, d, n_layers, L)
    lengths = np.array([1, L - 1, L], dtype=np.int64)
    B = len(lengths)
    hist = rng.integers(1, n_items, size=(B, L)).astype(np.int64) * (np.arange(L)[None, :] < lengths[:, None])
    hist[2, ::3] = 5                                            # a repeated item
    dhv = rng.normal(size=(B, d)).astype(np.float32)
    item_emb = t(P["i_embeddings.weight"], cuda).requires_grad_(True)
    pos_emb = t(P["p_embeddings.weight"], cuda).requires_grad_(True)
    blocks = []
    for l in range(n_layers):
        blk = _TransformerLayer(d, d, n_heads, 0.0)
        pre = "transformer_block.%d." % l
        blk.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in P.items() if k.startswith(pre)})
        blocks.append(blk.to(cuda))
    hv = hnn.sasrec_encode_layers(item_emb, pos_emb, blocks, n_heads, t(hist, cuda), t(lengths, cuda))
    (hv * t(dhv, cuda)).sum().backward()
    hv64, G = _sasrec64(P, hist, lengths, n_layers, n_heads, dhv)
    what = f"d={d} heads={n_heads} layers={n_layers} L={L}"
    assert_close(hv.detach().cpu().numpy(), hv64, what="hv " + what, rtol=2e-5, atol_scale=2e-5)
    floor = 1e-6 * max(float(np.abs(v).max()) for v in G.values())
    assert_close(item_emb.grad.cpu().numpy()[1:], G["i_embeddings.weight"][1:], what="d item_emb " + what, rtol=2e-5, atol_scale=2e-5,
                 abs_floor=floor)
    assert_close(pos_emb.grad.cpu().numpy()[1:], G["p_embeddings.weight"][1:], what="d pos_emb " + what, rtol=2e-5, atol_scale=2e-5,
                 abs_floor=floor)
    for l, blk in enumerate(blocks):
        for name, prm in blk.named_parameters():
            assert_close(prm.grad.cpu().numpy(), G["transformer_block.%d.%s" % (l, name)], what=f"{what} layer {l} d{name}", rtol=2e-5,
                         atol_scale=2e-5, abs_floor=floor)
