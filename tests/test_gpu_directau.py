"""GPU: DirectAU on the HIP engine (rc_directau_fwd / _bwd) against the reference's goldens (tests/golden/make_golden_directau.py)
and float64 restatements: training prediction, loss, both table gradients, two fit() iterations, eval predictions; batches of
1, 2 and identical rows, d = 4 and 256; B = 65,536 and a large B at d = 256 against a blocked float64 computation; bit-identical
reruns, hipGraph replay, --test_all ranks and the CLI on both data paths.  torch.pdist, torch.cdist and F.normalize raise
throughout.

Tolerances: prediction, loss and table gradients 2e-5 of the largest entry per tensor (the issue's bar).  The large batches
compare the row gradients at 2e-5 of the largest entry as well; the largest errors seen are printed (run with -s)."""
import argparse
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, assert_update_close, golden_cases, load_golden
from synth_data import make_dataset

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import directau_np  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

pytestmark = pytest.mark.gpu
CASES = golden_cases("directau_")
TOL = 2e-5


@pytest.fixture(autouse=True)
def no_torch_pairwise(monkeypatch):
    """nothing on the path may fall back to torch's pairwise distances or normalisation"""
    def refuse(*a, **k):
        raise AssertionError("torch pairwise / normalize called")
    monkeypatch.setattr(torch, "pdist", refuse)
    monkeypatch.setattr(torch, "cdist", refuse)
    monkeypatch.setattr(F, "normalize", refuse)


def _close(got, want, what, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-30)
    err = float(np.abs(got - want).max()) if want.size else 0.0
    assert err <= tol * scale, f"{what}: max |diff| {err:.3e} > {tol:g} * {scale:.3e}"
    return err / scale


def _model(g, dev):
    from models.general.DirectAU import DirectAU
    n_users, n_items, d, _, _ = (int(x) for x in g["meta"])
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=0, dropout=0, test_all=0, emb_size=d,
                           gamma=float(g["hyper"][0]))
    m = DirectAU(args, SimpleNamespace(n_users=n_users, n_items=n_items)).to(dev)
    with torch.no_grad():
        m.u_embeddings.weight.copy_(torch.from_numpy(g["U0"]))
        m.i_embeddings.weight.copy_(torch.from_numpy(g["I0"]))
    return m


def _feed(u, i, dev):
    return {"user_id": torch.from_numpy(u).to(dev), "item_id": torch.from_numpy(i).to(dev), "batch_size": len(u), "phase": "train"}


def _runner(opt, lr, l2, graph=0):
    from helpers.BaseRunner import BaseRunner
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.train, a.log_file = 1, "/tmp/rechorus_amd_test/log.txt"
    a.optimizer, a.lr, a.l2, a.graph, a.engine = opt, lr, l2, graph, "dense"
    return BaseRunner(a)


def _step(m, batch):
    m.optimizer.zero_grad()
    loss = m.loss(m(batch))
    loss.backward()
    m.optimizer.step()
    return loss.detach()


def _tables(m):
    return m.u_embeddings.weight.detach().cpu().numpy(), m.i_embeddings.weight.detach().cpu().numpy()


def _loss_close(got, want, what):
    if np.isnan(want):
        assert np.isnan(got), what
    else:
        assert abs(got - float(want)) <= TOL * max(1.0, abs(float(want))), (what, got, float(want))


@pytest.mark.parametrize("case", CASES)
def test_golden_case(case, cuda):
    g = load_golden(case)
    gamma, lr, l2 = (float(x) for x in g["hyper"])
    opt = str(g["opt"])
    m = _model(g, cuda)
    m.train()
    out = m(_feed(g["uid"], g["iid"], cuda))
    assert out["prediction"].shape == (len(g["uid"]), 1)
    loss = m.loss(out)
    loss.backward()
    _close(out["prediction"].detach().cpu().numpy(), g["pred"], case + " pred")
    _loss_close(loss.item(), g["loss"], case + " loss")
    _close(m.u_embeddings.weight.grad.cpu().numpy(), g["GU"], case + " GU")
    _close(m.i_embeddings.weight.grad.cpu().numpy(), g["GI"], case + " GI")

    m2 = _model(g, cuda)
    m2.optimizer = _runner(opt, lr, l2)._build_optimizer(m2)
    m2.train()
    extra = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
    prev = (g["U0"], g["I0"])
    for step, (u, i) in enumerate(((g["uid"], g["iid"]), (g["uid2"], g["iid2"])), 1):
        ls = float(_step(m2, _feed(u, i, cuda)).item())
        _loss_close(ls, g["losses"][step - 1], f"{case} loss step {step}")
        U, I = _tables(m2)
        assert_update_close(U, prev[0], g["U%d" % step], what=f"{case} U step {step}", extra_atol=extra, outlier_atol=lr)
        assert_update_close(I, prev[1], g["I%d" % step], what=f"{case} I step {step}", extra_atol=extra, outlier_atol=lr)
        prev = (g["U%d" % step], g["I%d" % step])
        with torch.no_grad():     # continue from the reference's tables: step 2 checks one step, not two compounded
            m2.u_embeddings.weight.copy_(torch.from_numpy(prev[0]))
            m2.i_embeddings.weight.copy_(torch.from_numpy(prev[1]))
    m2.eval()
    with torch.no_grad():
        ep = m2({"user_id": torch.from_numpy(g["eval_uid"]).to(cuda), "item_id": torch.from_numpy(g["eval_iid"]).to(cuda),
                 "batch_size": len(g["eval_uid"]), "phase": "test"})["prediction"]
    _close(ep.cpu().numpy(), g["eval_pred"], case + " eval pred")


def _rows_check(u, v, gamma, what, tol=TOL):
    """the fused loss on rows u, v [B, d] (device) against the float64 restatement -> (relative errors of loss, grad u, grad v)"""
    from rechorus_amd import nn as hnn
    uu, vv = u.clone().requires_grad_(True), v.clone().requires_grad_(True)
    loss = hnn.directau_loss(uu, vv, gamma)
    loss.backward()
    want = directau_np.loss_and_row_grads(u.double().cpu().numpy(), v.double().cpu().numpy(), gamma)
    el = abs(loss.item() - want[0]) / max(1.0, abs(want[0]))
    assert el <= tol, (what, loss.item(), want[0])
    return el, _close(uu.grad.cpu().numpy(), want[4], what + " grad u", tol), _close(vv.grad.cpu().numpy(), want[5], what + " grad v", tol)


@pytest.mark.parametrize("B,d", [(2, 4), (33, 4), (129, 256), (300, 36), (4096, 64)])
def test_edge_shapes_against_float64(B, d, cuda):
    gen = torch.Generator(device=cuda).manual_seed(B + d)
    u = torch.randn(B, d, device=cuda, generator=gen)
    v = torch.randn(B, d, device=cuda, generator=gen)
    u[1] = u[0]                 # duplicated ids are the normal case
    v[1] = v[0] * 7.0           # same direction, other length
    _rows_check(u, v, 0.3, f"B={B} d={d}")


def test_batch_of_one(cuda):
    from rechorus_amd import nn as hnn
    u = torch.randn(1, 64, device=cuda, requires_grad=True)
    v = torch.randn(1, 64, device=cuda, requires_grad=True)
    loss = hnn.directau_loss(u, v, 1.0)
    assert torch.isnan(loss).item()
    loss.backward()
    want = directau_np.loss_and_row_grads(u.detach().double().cpu().numpy(), v.detach().double().cpu().numpy(), 1.0)
    _close(u.grad.cpu().numpy(), want[4], "B=1 grad u")
    _close(v.grad.cpu().numpy(), want[5], "B=1 grad v")


def test_identical_rows_give_zero_uniformity_and_zero_gradient(cuda):
    from rechorus_amd import nn as hnn
    x = torch.randn(1, 64, device=cuda).expand(300, 64).contiguous()
    u = x.clone().requires_grad_(True)
    v = x.clone().requires_grad_(True)
    loss = hnn.directau_loss(u, v, 1.0)
    loss.backward()
    assert abs(loss.item()) < 1e-5
    assert u.grad.abs().max().item() < 1e-5 * (300 / x.norm(dim=1).min().item())
    assert v.grad.abs().max().item() < 1e-5 * (300 / x.norm(dim=1).min().item())
    assert abs(hnn.uniformity(x).item()) < 1e-5


def test_static_methods_match_the_fused_loss(cuda):
    """DirectAU.alignment / DirectAU.uniformity (the reference's static methods) on the HIP kernels compose to the fused loss"""
    from models.general.DirectAU import DirectAU
    from rechorus_amd import nn as hnn
    gen = torch.Generator(device=cuda).manual_seed(5)
    u0, v0 = torch.randn(200, 32, device=cuda, generator=gen), torch.randn(200, 32, device=cuda, generator=gen)
    a = [t.clone().requires_grad_(True) for t in (u0, v0)]
    b = [t.clone().requires_grad_(True) for t in (u0, v0)]
    composed = DirectAU.alignment(*a) + 0.3 * (DirectAU.uniformity(a[0]) + DirectAU.uniformity(a[1])) / 2
    composed.backward()
    fused = hnn.directau_loss(b[0], b[1], 0.3)
    fused.backward()
    assert abs(composed.item() - fused.item()) <= 1e-6 * max(1.0, abs(fused.item()))
    for x, y in zip(a, b):
        _close(x.grad.cpu().numpy(), y.grad.cpu().numpy(), "static methods vs fused", 1e-5)


def _blocked64(x):
    """float64 on the device, 2048-row blocks: (S, s, M) of the normalised rows"""
    xh = x.double() / x.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    n = (xh * xh).sum(1)
    s = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    M = torch.empty_like(xh)
    for a in range(0, x.shape[0], 2048):
        bl = slice(a, min(x.shape[0], a + 2048))
        E = torch.exp(-2.0 * (n[bl, None] + n[None, :] - 2.0 * xh[bl] @ xh.T).clamp_min(0.0))
        idx = torch.arange(bl.start, bl.stop, device=x.device)
        E[idx - a, idx] = 0.0
        s[bl] = E.sum(1)
        M[bl] = E @ xh
    return xh, 0.5 * s.sum(), s, M


@pytest.mark.parametrize("B,d", [(65536, 64), (16384, 256)])
def test_large_batch_against_blocked_float64(B, d, cuda):
    from rechorus_amd import engine
    gen = torch.Generator(device=cuda).manual_seed(B)
    u = torch.randn(B, d, device=cuda, generator=gen)
    v = torch.randn(B, d, device=cuda, generator=gen)
    ids = torch.randint(0, B // 4, (B,), device=cuda, generator=gen)    # repeated rows, gathered by the row pass
    gamma = 0.3
    out, pred, buf, _ = engine.directau_fwd(u, v, gamma, user_ids=ids, item_ids=ids.flip(0).contiguous(), prediction=True)
    g1 = torch.ones(1, device=cuda)
    gu, gv = engine.directau_bwd(g1, B, d, (1.0, gamma / 2, gamma / 2), buf)
    ru, rv = u[ids], v[ids.flip(0)]
    want_pred = (ru.double() * rv.double()).sum(1, keepdim=True)
    errs = {"pred": _close(pred.cpu().numpy(), want_pred.cpu().numpy(), "pred")}
    xu, Su, su, Mu = _blocked64(ru)
    xv, Sv, sv, Mv = _blocked64(rv)
    P = B * (B - 1) / 2.0
    uu, ui = torch.log(Su / P).item(), torch.log(Sv / P).item()
    align = ((xu - xv) ** 2).sum(1).mean().item()
    o = out.cpu().numpy().astype(np.float64)
    for k, (got, want) in enumerate(((o[1], align), (o[2], uu), (o[3], ui), (o[0], align + gamma * (uu + ui) / 2))):
        assert abs(got - want) <= TOL * max(1.0, abs(want)), (k, got, want)
    for (xh, S, s, M, g, x, name) in ((xu, Su, su, Mu, gu, ru, "u"), (xv, Sv, sv, Mv, gv, rv, "v")):
        sign = 1.0 if name == "u" else -1.0
        gh = sign * 2.0 * (xu - xv) / B - (2.0 * gamma / S) * (s[:, None] * xh - M)
        nrm = x.double().norm(dim=1, keepdim=True)
        want = (gh - xh * (xh * gh).sum(1, keepdim=True)) / nrm
        errs["grad_" + name] = _close(g.cpu().numpy(), want.cpu().numpy(), f"B={B} d={d} grad {name}")
    print(f"\nDirectAU B={B} d={d}: largest error / largest entry {errs} (tolerance {TOL:g})")


def test_reruns_are_bit_identical(cuda):
    from rechorus_amd import engine
    gen = torch.Generator(device=cuda).manual_seed(9)
    for B, d in ((4096, 64), (1000, 128), (77, 32)):      # chunked sweep, mid-size, one workgroup
        u, v = torch.randn(B, d, device=cuda, generator=gen), torch.randn(B, d, device=cuda, generator=gen)
        runs = []
        for _ in range(2):
            out, _, buf, _ = engine.directau_fwd(u, v, 0.7)
            gu, gv = engine.directau_bwd(torch.ones(1, device=cuda), B, d, (1.0, 0.35, 0.35), buf)
            runs.append([t.cpu().numpy().copy() for t in (out, gu, gv)])
        for a, b in zip(*runs):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_hipgraph_replay_is_bit_equal_to_eager(cuda):
    from rechorus_amd import graph as hgraph
    if not hgraph.usable():
        pytest.fail("hipGraph replay is disabled in this process")
    g = load_golden("directau_d64_g03_adam_b77")
    rng = np.random.default_rng(3)
    n_users, n_items = int(g["meta"][0]), int(g["meta"][1])
    batches = [(g["uid"], g["iid"])] + [(rng.integers(1, n_users, 77), rng.integers(1, n_items, (77, 1))) for _ in range(4)]
    results = []
    for replay in (False, True):
        m = _model(g, cuda)
        m.optimizer = _runner("Adam", 1e-3, 1e-5, graph=1)._build_optimizer(m)
        m.train()
        step = hgraph.GraphedStep(m) if replay else None
        losses = []
        for u, i in batches:          # 2 eager warm-up steps, then capture and 3 replays
            b = _feed(u.astype(np.int64), i.astype(np.int64), cuda)
            losses.append(step.run(b) if replay else _step(m, b).reshape(1))
        if replay:
            assert step.graph is not None
        torch.cuda.synchronize()
        results.append([*_tables(m), torch.cat(losses).cpu().numpy()])
    for a, b in zip(*results):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_test_all_ranks_equal_a_numpy_ranking(cuda):
    from oracle import sampler_oracle as S
    from rechorus_amd import engine
    g = load_golden("directau_d64_g03_adam_b77")
    m = _model(g, cuda)
    m.eval()
    n_users = int(g["meta"][0])
    rng = np.random.default_rng(1)
    sets = {u: set(rng.integers(1, int(g["meta"][1]), 5).tolist()) for u in range(n_users)}
    users, targets = g["eval_uid"], g["eval_iid"][:, 0]
    for u, t in zip(users, targets):
        sets[int(u)].add(int(t))
    ptr = np.zeros(n_users + 1, dtype=np.int64)
    flat = []
    for u in range(n_users):
        flat += sorted(sets[u])
        ptr[u + 1] = len(flat)
    feed = {"user_id": torch.from_numpy(users).to(cuda)}
    with torch.no_grad():
        vec, table = m.full_catalogue_vectors(feed)
        rank, _ = engine.full_catalogue_rank(vec.contiguous(), table, feed["user_id"], torch.from_numpy(targets).to(cuda),
                                             torch.from_numpy(ptr).to(cuda), torch.tensor(flat, dtype=torch.int64, device=cuda))
    U, I = _tables(m)
    want = S.full_catalogue_rank(U[users], I, users, targets, sets)
    s64 = U[users].astype(np.float64) @ I.astype(np.float64).T
    t64 = s64[np.arange(len(users)), targets]
    near = (np.abs(s64 - t64[:, None]) <= 1e-5 * (1 + np.abs(t64[:, None]))).sum(axis=1) - 1
    assert (np.abs(rank.cpu().numpy().astype(np.int64) - want) <= near).all(), (rank.cpu().numpy(), want)
    assert want.max() > 1


@pytest.fixture(scope="module")
def synth_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dau_data"))
    make_dataset(root, "synth", n_users=300, n_items=250, per_user=14, seed=5)
    return root


@pytest.mark.parametrize("pipeline_flag,test_all", [("1", "0"), ("1", "1"), ("0", "0")])
def test_cli_trains_one_epoch(pipeline_flag, test_all, synth_root, tmp_path, cuda, monkeypatch):
    import main
    from rechorus_amd import graph as hgraph, pipeline
    replays, sampled = [], []
    run0, sample0 = hgraph.GraphedStep.run, pipeline.DeviceDataset.sample_negatives
    # a run() that finds a captured graph replays it (warm-up steps and the capture itself run with graph still None)
    monkeypatch.setattr(hgraph.GraphedStep, "run", lambda self, b: replays.append(self.graph is not None) or run0(self, b))
    monkeypatch.setattr(pipeline.DeviceDataset, "sample_negatives", lambda self, seed: sampled.append(self.kind) or sample0(self, seed))
    log = str(tmp_path / "log" / "run.txt")
    res = main.run(["--model_name", "DirectAU", "--emb_size", "64", "--gamma", "0.3", "--lr", "1e-3", "--l2", "1e-5",
                    "--dataset", "synth", "--path", synth_root + "/", "--epoch", "1", "--batch_size", "256", "--num_workers", "0",
                    "--regenerate", "1", "--test_all", test_all, "--device_pipeline", pipeline_flag, "--log_file", log,
                    "--model_path", str(tmp_path / "m.pt"), "--topk", "5,10", "--save_final_results", "0"])
    text = open(log).read()
    assert re.search(r"Epoch 1\s+loss=-?[0-9.]+", text), text[-2000:]
    hr = float(re.search(r"HR@5:([0-9.]+)", res["test"]).group(1))
    assert 0.0 <= hr <= 1.0 and "NDCG@10" in res["test"]
    if pipeline_flag == "1":
        assert sampled == ["general_unsampled"]   # the device pipeline serves training, no sampler launch behind it
        assert sum(replays) >= 1                  # the dense step was captured and then replayed from the hipGraph
    else:
        assert not sampled
