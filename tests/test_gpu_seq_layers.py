"""GPU: the shape-generic sequence-encoder layers (csrc/seq_layers.hip: rc_seq_* + the GEMMs of csrc/mlp.hip), i.e. SASRec outside
the register-resident kernels' envelope -- emb_size 128 / 48, histories of 100 and 200 positions with several blocks and with
dropout, five blocks -- against the reference's own outputs (tests/golden/sasrec_*.npz, sasrecdrop_*.npz: prediction, loss, every
parameter gradient, two fit() iterations) through the plugin's SASRec class; the kernels on their own against float64 restatements
of utils/layers.py:52-63 (general masks) and :110,117.
Reference: src/models/sequential/SASRec.py:51-86, src/utils/layers.py:9-63,92-118."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close, assert_update_close, load_golden
from oracle import sasrec_oracle as SO
from test_oracle_sasrec import CASES as ALL_CASES, DROP_CASES as ALL_DROP_CASES, params

pytestmark = pytest.mark.gpu

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)


def _model(g, cuda, dropout=0.0):
    from models.sequential.SASRec import SASRec
    n_items, d, n_layers, n_heads, hist_max = (int(x) for x in g["meta"][:5])
    args = argparse.Namespace(device=cuda, model_path="", buffer=1, num_neg=int(g["meta"][6]), dropout=dropout, test_all=0, emb_size=d,
                              num_layers=n_layers, num_heads=n_heads, history_max=hist_max)
    model = SASRec(args, argparse.Namespace(n_users=10, n_items=n_items))
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("P0/")}
    assert set(sd) == set(model.state_dict())
    model.load_state_dict(sd)
    return model.to(cuda)


def _batch(g, cuda, sfx=""):
    n = len(g["len" + sfx])
    return {"history_items": torch.from_numpy(g["hist" + sfx]).to(cuda), "lengths": torch.from_numpy(g["len" + sfx]).to(cuda),
            "item_id": torch.from_numpy(g["iid" + sfx]).to(cuda), "user_id": torch.zeros(n, dtype=torch.long, device=cuda),
            "batch_size": n, "phase": "train"}


def _generic(model, L, p=0.0):
    from rechorus_amd import engine
    return not engine.sasrec_supported(model.emb_size, model.num_layers, model.num_heads, L, p)


def _record(monkeypatch):
    from rechorus_amd import _lib
    from utils import layers
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda fn, *a: names.append(fn) or real(fn, *a))

    def no_torch_layers(*a, **k):
        raise AssertionError("the encoder ran the plugin's torch layers")
    monkeypatch.setattr(layers.TransformerLayer, "forward", no_torch_layers)
    monkeypatch.setattr(layers.MultiHeadAttention, "forward", no_torch_layers)
    return names


@pytest.mark.parametrize("case", ALL_CASES)
def test_sasrec_model_matches_reference_inside_and_outside_the_envelope(case, cuda, monkeypatch):
    """prediction, loss and every parameter gradient of the plugin's SASRec against the reference's own, for every golden shape;
    outside the envelope the encoder is rc_seq_* + rc_linear_* and never the torch layers"""
    g = load_golden(case)
    model = _model(g, cuda)
    model.train()
    generic = _generic(model, g["hist"].shape[1])
    names = _record(monkeypatch)
    out = model(_batch(g, cuda))
    loss = model.loss(out)
    loss.backward()
    monkeypatch.undo()
    if generic:
        n_layers = model.num_layers
        assert names.count("rc_seq_attention_fwd") == n_layers and names.count("rc_seq_attention_bwd") == n_layers, names
        assert names.count("rc_seq_add_layernorm_fwd") == 2 * n_layers and names.count("rc_seq_embed_fwd") == 1
        assert names.count("rc_linear_fwd") == 5 * n_layers
        assert not any(n.startswith("rc_sasrec_batch") or n in ("rc_sasrec_fwd", "rc_sasrec_bwd") for n in names)
    else:
        assert not any(n.startswith("rc_seq_") for n in names)
    assert_close(out["prediction"].detach().cpu().numpy(), g["pred"], what="prediction", atol_scale=2e-5)
    assert_close(loss.item(), g["loss"], what="loss", rtol=2e-5)
    G = params(g, "G/")
    floor = 1e-6 * max(float(np.abs(v).max()) for v in G.values())
    for name, p in model.named_parameters():
        assert_close(p.grad.cpu().numpy(), G[name], what="grad " + name, rtol=2e-5, atol_scale=5e-5, abs_floor=floor)


@pytest.mark.parametrize("case", ALL_DROP_CASES)
def test_sasrec_model_with_dropout_matches_reference(case, cuda, monkeypatch):
    """training mode: the reference with its nn.Dropout modules applying the counter-based mask (make_golden_sasrec.py) against the
    plugin's SASRec with the same seed -- the batch encoder inside the envelope, the generic layers outside, one mask stream"""
    g = load_golden(case)
    p = float(g["p"])
    model = _model(g, cuda, dropout=p)
    model.train()
    generic = _generic(model, g["hist"].shape[1], p)
    names = _record(monkeypatch)
    model.drop_seed.fill_(int(g["mask_seed"]) - 1)      # _encode bumps it once per forward
    out = model(_batch(g, cuda))
    loss = model.loss(out)
    loss.backward()
    monkeypatch.undo()
    assert generic == any(n.startswith("rc_seq_") for n in names)
    assert_close(out["prediction"].detach().cpu().numpy(), g["pred"], what="prediction", atol_scale=2e-5)
    assert_close(loss.item(), g["loss"], what="loss", rtol=2e-5)
    G = params(g, "G/")
    floor = 1e-6 * max(float(np.abs(v).max()) for v in G.values())
    for name, prm in model.named_parameters():
        assert_close(prm.grad.cpu().numpy(), G[name], what="grad " + name, rtol=2e-5, atol_scale=5e-5, abs_floor=floor)
    again = model(_batch(g, cuda))["prediction"].detach()
    assert not torch.equal(again, out["prediction"].detach())     # next forward, next mask
    model.eval()
    e1, e2 = model(_batch(g, cuda))["prediction"].detach(), model(_batch(g, cuda))["prediction"].detach()
    assert torch.equal(e1, e2)
    want = SO.forward(params(g), g["hist"], g["len"], g["iid"], int(g["meta"][3]))
    assert_close(e1.cpu().numpy(), want, what="eval prediction", atol_scale=2e-5)


GENERIC_CASES = [c for c in ALL_CASES if c in ("sasrec_d128_l1_h4", "sasrec_d128_l2_h8_L100", "sasrec_d64_l3_h4_L200", "sasrec_d48_l2_h3",
                                               "sasrec_d64_l5_h2")]


@pytest.mark.parametrize("case", GENERIC_CASES)
@pytest.mark.parametrize("tag,opt", [("SGD_l20.001", "SGD"), ("Adam_l20.0001", "Adam")])
def test_two_fit_iterations_outside_the_envelope_match_reference(case, tag, opt, cuda):
    """model(batch) -> loss -> backward -> HipOptimizer.step twice (the dense route BaseRunner.fit takes for these shapes) against
    the reference's own fit()"""
    from helpers.BaseRunner import BaseRunner
    g = load_golden(case)
    lr, l2 = (float(x) for x in g[tag + "_hyper"])
    model = _model(g, cuda)
    assert _generic(model, g["hist"].shape[1]) and not model.hip_rowwise_supported()
    a = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_args([])
    a.train, a.log_file, a.optimizer, a.lr, a.l2, a.engine = 1, "/tmp/rechorus_amd_test/log.txt", opt, lr, l2, "auto"
    runner = BaseRunner(a)
    model.optimizer = runner._build_optimizer(model)
    assert not runner._use_rowwise(model)
    model.train()
    for step, sfx in enumerate(("", "2"), 1):
        model.optimizer.zero_grad()
        loss = model.loss(model(_batch(g, cuda, sfx)))
        loss.backward()
        model.optimizer.step()
        assert_close(loss.item(), g[tag + "_losses"][step - 1], what=f"loss {step}", rtol=2e-5)
    P0, want, G1 = params(g), params(g, tag + "/"), params(g, "G/")
    ex = 2e-3 * lr if opt == "Adam" else 0.0
    n_ill = n_all = 0
    for name, p in model.state_dict().items():
        if opt == "Adam" and name.endswith("k_linear.bias"):     # analytically zero gradient (tests/test_gpu_sasrec.py)
            assert float(np.abs(p.cpu().numpy() - P0[name]).max()) <= 2.5 * lr
            continue
        if opt == "Adam":
            decay = 0.0 if "bias" in name else l2
            ill = np.abs(G1[name] + decay * P0[name]) < 1e-7
            n_ill += int((ill & (np.abs(want[name] - P0[name]) > 0)).sum())
            n_all += ill.size
            # (not strict: a row that is absent from the first batch starts from g = l2 * w, a few 1e-7 -- just past the listed
            #  threshold and still a 3 % lever on Adam's normalised step; at most 0.5 % of a tensor may sit within 20 x extra_atol)
            assert_update_close(p.cpu().numpy(), P0[name], want[name], what=name, extra_atol=ex, rtol=2e-4, exclude=ill)
        else:
            assert_update_close(p.cpu().numpy(), P0[name], want[name], what=name, rtol=2e-4)
    assert n_ill <= 0.005 * max(n_all, 1), f"{n_ill} of {n_all} elements excluded as ill-conditioned"


# ---- the kernels on their own ----------------------------------------------------------------------------------------------

def _attention64(q, k, v, H, mask):
    """utils/layers.py:30-32,52-63 in float64: head split, scores / sqrt(dk), mask -> -inf, softmax, NaN -> 0, @ V, heads merged"""
    B, L, D = q.shape
    dk = D // H
    split = lambda t: t.view(B, L, H, dk).transpose(1, 2)
    s = split(q) @ split(k).transpose(-2, -1) / dk ** 0.5
    s = s.masked_fill(mask == 0, float("-inf"))
    p = (s - s.max()).softmax(dim=-1)
    p = p.masked_fill(torch.isnan(p), 0)
    return (p @ split(v)).transpose(1, 2).reshape(B, L, D)


@pytest.mark.parametrize("B,L,H,dk,kind", [(5, 7, 2, 16, "causal"), (3, 70, 3, 20, "causal+len"), (4, 130, 1, 64, "mask"), (2, 33, 4, 8, "batchmask"),
                                            (2, 300, 2, 32, "causal+len"), (1, 1, 1, 4, "causal"), (3, 40, 2, 128, "mask+len"), (2, 9, 5, 3, "causal")])
def test_attention_kernels_vs_float64(B, L, H, dk, kind, cuda):
    """rc_seq_attention_fwd / _bwd: causal, arbitrary [L, L] and per-sequence [B, L, L] masks (with fully hidden rows), valid-row
    offsets, head widths that are no multiple of 4 -- values and dQ / dK / dV against autograd in float64"""
    from rechorus_amd import engine
    rng = np.random.default_rng(B * 1000 + L)
    D = H * dk
    mk = lambda: torch.from_numpy(rng.normal(0, 1.0, (B, L, D)).astype(np.float32)).to(cuda)
    q, k, v, w = mk(), mk(), mk(), mk()
    lengths = torch.from_numpy(rng.integers(1, L + 1, B).astype(np.int64)).to(cuda) if "len" in kind else torch.full((B,), L, dtype=torch.int64, device=cuda)
    lengths[0] = L
    off = engine.seq_offsets(lengths, L) if "len" in kind else None
    assert off is None or off.cpu().tolist() == [0] + np.cumsum(lengths.cpu().numpy()).tolist()
    causal = "causal" in kind
    mask = None
    full = torch.ones((B, 1, L, L), dtype=torch.bool, device=cuda)
    if causal:
        full &= torch.tril(torch.ones((L, L), dtype=torch.bool, device=cuda))
    if "mask" in kind:
        shape = (B, L, L) if kind == "batchmask" else (1, L, L)
        m = torch.from_numpy((rng.random(shape) < 0.7)).to(cuda)
        m[:, L // 2, :] = False          # a row that sees nothing: NaN -> 0 in the reference
        mask = m.to(torch.uint8).contiguous()
        full &= m[:, None, :, :]
    valid = torch.arange(L, device=cuda)[None, :] < lengths[:, None]
    full = full & valid[:, None, None, :]                 # keys beyond the sequence are not rows of the batch
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    want = _attention64(q64, k64, v64, H, full) * valid[:, :, None]
    (want * w.double()).sum().backward()
    qf, kf, vf = (t.reshape(B * L, D).contiguous() for t in (q, k, v))
    ctx, lse = engine.seq_attention_fwd(qf, kf, vf, off, B, L, H, mask=mask, causal=causal)
    assert_close(ctx.view(B, L, D).cpu().numpy(), want.detach().cpu().numpy(), what="ctx", rtol=1e-5, atol_scale=1e-5)
    dctx = (w * valid[:, :, None]).reshape(B * L, D).contiguous()
    dQ, dK, dV = engine.seq_attention_bwd(qf, kf, vf, off, B, L, H, lse, dctx, mask=mask, causal=causal)
    for name, got, ref in (("dQ", dQ, q64.grad), ("dK", dK, k64.grad), ("dV", dV, v64.grad)):
        ref = ref * valid[:, :, None]        # (a hidden row's own q / k / v receive nothing through valid rows)
        assert_close(got.view(B, L, D).cpu().numpy(), ref.cpu().numpy(), what=name, rtol=2e-5, atol_scale=2e-5)
    assert torch.equal(ctx, engine.seq_attention_fwd(qf, kf, vf, off, B, L, H, mask=mask, causal=causal)[0])     # deterministic


@pytest.mark.parametrize("rows,d,p", [(50, 64, 0.0), (333, 128, 0.3), (7, 48, 0.5), (1000, 512, 0.1), (40, 1024, 0.0), (3000, 16, 0.25)])
def test_add_layernorm_kernels_vs_float64(rows, d, p, cuda):
    """rc_seq_add_layernorm_fwd / _bwd against nn.LayerNorm in float64 with the mask of oracle/sasrec_oracle.dropout_keep (the batch
    encoder's stream: compact row, site, feature); with and without a residual, rows as B * L with offsets"""
    from rechorus_amd import engine
    rng = np.random.default_rng(rows + d)
    L = 10 if rows % 10 == 0 else 1
    B = rows // L
    lengths = rng.integers(1, L + 1, B).astype(np.int64)
    lengths[0] = L
    len_d = torch.from_numpy(lengths).to(cuda)
    off = engine.seq_offsets(len_d, L) if L > 1 else None
    valid = (np.arange(L)[None, :] < lengths[:, None]).reshape(-1) if L > 1 else np.ones(rows, dtype=bool)
    mk = lambda *s: torch.from_numpy(rng.normal(0, 1.0, s).astype(np.float32)).to(cuda)
    A, R, w, b, dy = mk(rows, d), mk(rows, d), 1 + 0.1 * mk(d), 0.1 * mk(d), mk(rows, d)
    site, seed_v = 3, 123456789
    seed = torch.tensor([seed_v], dtype=torch.int64, device=cuda)
    if p > 0:
        keep = SO.dropout_keep(seed_v, lengths if L > 1 else np.ones(rows, dtype=np.int64), L, d, 2, p)[site].reshape(rows, d)
    else:
        keep = np.ones((rows, d), dtype=np.float32)
    keep_t = torch.from_numpy(keep).to(cuda).double()
    vt = torch.from_numpy(valid).to(cuda)
    for with_r in (True, False):
        A64, R64, w64, b64 = (t.double().requires_grad_(True) for t in (A, R, w, b))
        z = A64 * keep_t + (R64 if with_r else 0)
        y64 = torch.nn.functional.layer_norm(z, (d,), w64, b64, 1e-5) * vt[:, None]
        (y64 * dy.double()).sum().backward()
        Y, xhat, rstd = engine.seq_add_layernorm_fwd(A, R if with_r else None, w, b, off, L, p, seed if p > 0 else None, site)
        assert_close(Y.cpu().numpy(), y64.detach().cpu().numpy(), what="Y", rtol=1e-5, atol_scale=1e-5)
        dA, dR, dw, db = engine.seq_add_layernorm_bwd(dy, xhat, rstd, w, off, L, p, seed if p > 0 else None, site, need_dR=with_r)
        assert_close(dA.cpu().numpy(), A64.grad.cpu().numpy(), what="dA", rtol=2e-5, atol_scale=2e-5)
        if with_r:
            assert_close(dR.cpu().numpy(), R64.grad.cpu().numpy(), what="dR", rtol=2e-5, atol_scale=2e-5)
        else:
            assert dR is None
        floor = 3e-7 * float(dy.abs().max()) * rows ** 0.5 * 4
        assert_close(dw.cpu().numpy(), w64.grad.cpu().numpy(), what="dw", rtol=2e-5, atol_scale=2e-5, abs_floor=floor)
        assert_close(db.cpu().numpy(), b64.grad.cpu().numpy(), what="db", rtol=2e-5, atol_scale=2e-5, abs_floor=floor)


def test_embed_and_pick_last(cuda):
    from rechorus_amd import engine
    rng = np.random.default_rng(3)
    for B, L, d in ((9, 13, 64), (4, 1, 20), (300, 50, 6)):
        I = torch.from_numpy(rng.normal(size=(40, d)).astype(np.float32)).to(cuda)
        P = torch.from_numpy(rng.normal(size=(L + 1, d)).astype(np.float32)).to(cuda)
        lengths = torch.from_numpy(rng.integers(1, L + 1, B).astype(np.int64)).to(cuda)
        hist = torch.from_numpy(rng.integers(1, 40, (B, L)).astype(np.int64)).to(cuda) * (torch.arange(L, device=cuda)[None, :] < lengths[:, None])
        X = engine.seq_embed(I, P, hist.contiguous(), lengths)
        valid = (hist > 0)
        pos = (lengths[:, None] - torch.arange(L, device=cuda)[None, :]) * valid
        want = (I[hist] + P[pos]) * valid[:, :, None]
        assert torch.equal(X.view(B, L, d), want)
        hv = engine.seq_pick_last(X, lengths, B, L)
        assert torch.equal(hv, want[torch.arange(B, device=cuda), lengths - 1])
        g = torch.from_numpy(rng.normal(size=(B, d)).astype(np.float32)).to(cuda)
        dX = engine.seq_pick_last_bwd(g, lengths, B, L).view(B, L, d)
        ref = torch.zeros_like(dX)
        ref[torch.arange(B, device=cuda), lengths - 1] = g
        assert torch.equal(dX, ref)
        # position-table gradient of arbitrary row gradients (zero on the padding): index_add over the position ids in float64
        gx = torch.from_numpy(rng.normal(size=(B, L, d)).astype(np.float32)).to(cuda) * valid[:, :, None]
        GP = engine.seq_pos_grad(gx.reshape(B * L, d).contiguous(), lengths, B, L, L + 3)
        want_gp = torch.zeros((L + 3, d), dtype=torch.float64, device=cuda).index_add_(0, pos.reshape(-1), gx.double().reshape(-1, d))
        want_gp[0] = 0          # (position 0 = the padding: its rows carry zero gradients)
        assert_close(GP.cpu().numpy(), want_gp.cpu().numpy(), what="pos grad", rtol=1e-5, atol_scale=1e-5, abs_floor=3e-7 * B ** 0.5 * 4)
        assert not bool(GP[0].any()) and not bool(GP[L + 1:].any())


def test_shapes_outside_every_kernel_are_refused_not_rerouted(cuda):
    from rechorus_amd import engine, nn as hnn
    assert hnn.sasrec_layers_supported(128, 4, 100) and hnn.sasrec_layers_supported(48, 3, 15) and hnn.sasrec_layers_supported(64, 2, 1024)
    assert not hnn.sasrec_layers_supported(66, 2, 20)        # emb_size no multiple of 4
    assert not hnn.sasrec_layers_supported(64, 3, 20)        # heads do not divide it
    assert not hnn.sasrec_layers_supported(64, 2, 1025)
    assert not engine.seq_attention_supported(10, 257)
