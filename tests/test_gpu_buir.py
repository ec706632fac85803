"""GPU: BUIR on the HIP engine (rc_buir_fwd / _bwd / _query / _scores / _ema) against the reference's goldens
(tests/golden/make_golden_buir.py) and the float64 restatement (tests/buir_np.py): training prediction, loss, the four gradients,
two iterations in BUIRRunner's order with every table, eval predictions; a grid of batch and embedding sizes around the 64-row
tile; identical rows, a zero target row, an upstream gradient of 3; the target update bit-equal to the separately-rounded fp32
expression; bit-identical reruns, hipGraph replay, --test_all ranks and the CLI on both data paths.  F.normalize and F.linear
raise throughout.

Tolerance: 2e-5 of the largest entry per tensor, everywhere.  With RC_BUIR_TOL_REPORT=<file> the largest error every comparison
saw is written there (profiles/buir_tolerances.txt)."""
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
import buir_np  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

pytestmark = pytest.mark.gpu
CASES = golden_cases("buir_")
TOL = 2e-5
STATE = (("UO", "user_online"), ("UT", "user_target"), ("IO", "item_online"), ("IT", "item_target"))
SEEN = {}


@pytest.fixture(autouse=True)
def no_torch_normalize_or_linear(monkeypatch):
    """nothing on the path may fall back to torch's normalisation or dense layer"""
    def refuse(*a, **k):
        raise AssertionError("torch normalize / linear called")
    monkeypatch.setattr(F, "normalize", refuse)
    monkeypatch.setattr(F, "linear", refuse)
    monkeypatch.setattr(torch.nn.functional, "linear", refuse)


@pytest.fixture(scope="module", autouse=True)
def tolerance_report():
    yield
    path = os.environ.get("RC_BUIR_TOL_REPORT")
    if path and SEEN:
        with open(path, "w") as f:
            f.write("BUIR GPU tests (tests/test_gpu_buir.py, one MI355X): the largest error each comparison saw, as a fraction of the\n"
                    "tensor's largest entry, next to what it allows.\n\n")
            f.write("largest over all %d comparisons: %.3e (allowed %g)\n\n" % (len(SEEN), max(SEEN.values()), TOL))
            for k in sorted(SEEN):
                f.write("%s: %.3e (allowed %g)\n" % (k, SEEN[k], TOL))


def _close(got, want, what, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-30)
    err = float(np.abs(got - want).max()) if want.size else 0.0
    print(f"{what}: {err / scale:.3e} of the largest entry")
    SEEN[what] = max(SEEN.get(what, 0.0), err / scale)
    assert err <= tol * scale, f"{what}: max |diff| {err:.3e} > {tol:g} * {scale:.3e}"
    return err / scale


def _loss_close(got, want, what):
    want = float(want)
    err = abs(float(got) - want) / max(1.0, abs(want))
    print(f"{what}: {err:.3e}")
    SEEN[what] = max(SEEN.get(what, 0.0), err)
    assert err <= TOL, (what, got, want)


def _load_state(m, g, tag):
    with torch.no_grad():
        for key, name in STATE:
            getattr(m, name).weight.copy_(torch.from_numpy(g[key + tag]))
        m.predictor.weight.copy_(torch.from_numpy(g["W" + tag]))
        m.predictor.bias.copy_(torch.from_numpy(g["b" + tag]))


def _model(g, dev):
    from models.general.BUIR import BUIR
    n_users, n_items, d = (int(x) for x in g["meta"][:3])
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=0, dropout=0, test_all=0, emb_size=d,
                           momentum=float(g["hyper"][0]))
    m = BUIR(args, SimpleNamespace(n_users=n_users, n_items=n_items)).to(dev)
    _load_state(m, g, "0")
    return m


def _state(m):
    out = {key: getattr(m, name).weight.detach().cpu().numpy() for key, name in STATE}
    out["W"], out["b"] = m.predictor.weight.detach().cpu().numpy(), m.predictor.bias.detach().cpu().numpy()
    return out


def _feed(u, i, dev, phase="train"):
    return {"user_id": torch.from_numpy(np.asarray(u, np.int64)).to(dev), "item_id": torch.from_numpy(np.asarray(i, np.int64)).to(dev),
            "batch_size": len(u), "phase": phase}


def _runner(opt, lr, l2, graph=0):
    from helpers.BUIRRunner import BUIRRunner
    a, _ = BUIRRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.train, a.log_file = 1, "/tmp/rechorus_amd_test/log.txt"
    a.optimizer, a.lr, a.l2, a.graph, a.engine = opt, lr, l2, graph, "dense"
    return BUIRRunner(a)


def _step(m, batch, runner):
    """one batch in BUIRRunner's order"""
    m.optimizer.zero_grad()
    loss = m.loss(m(batch))
    loss.backward()
    m.optimizer.step()
    runner._after_step(m)
    return loss.detach()


@pytest.mark.parametrize("case", CASES)
def test_golden_case(case, cuda):
    g = load_golden(case)
    momentum, lr, l2 = (float(x) for x in g["hyper"])
    opt = str(g["opt"])
    m = _model(g, cuda)
    m.train()
    out = m(_feed(g["uid"], g["iid"], cuda))
    assert out["prediction"].shape == (len(g["uid"]), 1) and not out["prediction"].requires_grad
    loss = m.loss(out)
    loss.backward()
    _close(out["prediction"].detach().cpu().numpy(), g["pred"], case + " pred")
    _loss_close(loss.item(), g["loss"], case + " loss")
    _close(m.user_online.weight.grad.cpu().numpy(), g["GUO"], case + " grad user_online")
    _close(m.item_online.weight.grad.cpu().numpy(), g["GIO"], case + " grad item_online")
    _close(m.predictor.weight.grad.cpu().numpy(), g["GW"], case + " grad W")
    _close(m.predictor.bias.grad.cpu().numpy(), g["Gb"], case + " grad b")
    assert m.user_target.weight.grad is None and m.item_target.weight.grad is None

    m2 = _model(g, cuda)
    runner = _runner(opt, lr, l2)
    m2.optimizer = runner._build_optimizer(m2)
    m2.train()
    extra = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
    for step, (u, i) in enumerate(((g["uid"], g["iid"]), (g["uid2"], g["iid2"])), 1):
        ls = float(_step(m2, _feed(u, i, cuda), runner).item())
        _loss_close(ls, g["losses"][step - 1], f"{case} loss step {step}")
        got = _state(m2)
        for key in ("UO", "UT", "IO", "IT", "W", "b"):
            _close(got[key], g[f"{key}{step}"], f"{case} {key} step {step}")
            assert_update_close(got[key], g[f"{key}{step - 1}"], g[f"{key}{step}"], what=f"{case} {key} step {step}",
                                extra_atol=extra, outlier_atol=lr)
        # the targets moved by the separately-rounded expression on THIS run's online tables, bit for bit
        for t in ("U", "I"):
            assert np.array_equal(got[t + "T"], buir_np.ema(g[f"{t}T{step - 1}"], got[t + "O"], momentum)), (case, t, step)
        _load_state(m2, g, str(step))     # continue from the reference's state: step 2 checks one step, not two compounded
    m2.eval()
    with torch.no_grad():
        ep = m2(_feed(g["eval_uid"], g["eval_iid"], cuda, phase="test"))["prediction"]
    _close(ep.cpu().numpy(), g["eval_pred"], case + " eval pred")


def _random_problem(d, B, seed, n_users=50, n_items=40):
    rng = np.random.default_rng(seed)
    tabs = [(0.5 * rng.standard_normal((n, d))).astype(np.float32) for n in (n_users, n_users, n_items, n_items)]
    W = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    b = rng.standard_normal(d).astype(np.float32)
    pu = 1.0 / np.arange(1, n_users + 1)
    pi = 1.0 / np.arange(1, n_items + 1)
    uid = rng.choice(n_users, size=B, p=pu / pu.sum()).astype(np.int64)     # Zipf: ids repeat inside the batch
    iid = rng.choice(n_items, size=B, p=pi / pi.sum()).astype(np.int64)
    return tabs, W, b, uid, iid


def _fused_check(tabs, W, b, uid, iid, g0, what, dev):
    from rechorus_amd import nn as hnn
    t = [torch.from_numpy(a).to(dev) for a in tabs]
    t[0].requires_grad_(True)
    t[2].requires_grad_(True)
    Wt, bt = torch.from_numpy(W).to(dev).requires_grad_(True), torch.from_numpy(b).to(dev).requires_grad_(True)
    loss, pred = hnn.buir_loss(*t, Wt, bt, torch.from_numpy(uid).to(dev), torch.from_numpy(iid).to(dev))
    (loss * g0).backward()
    want = buir_np.table_grads(*tabs, W, b, uid, iid, g0)
    _loss_close(loss.item(), want[0], what + " loss")
    _close(pred.cpu().numpy(), want[1], what + " pred")
    for got, ref, name in ((t[0].grad, want[2], "grad user_online"), (t[2].grad, want[3], "grad item_online"),
                           (Wt.grad, want[4], "grad W"), (bt.grad, want[5], "grad b")):
        _close(got.cpu().numpy(), ref, f"{what} {name}")
    assert t[1].grad is None and t[3].grad is None


@pytest.mark.parametrize("d", [16, 48, 64, 128])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257])
def test_edge_grid_against_float64(B, d, cuda):
    g0 = 3.0 if (B + d) % 2 else 1.0      # the upstream gradient is a device scalar of any value
    _fused_check(*_random_problem(d, B, seed=1000 * d + B), g0, f"B={B} d={d} g0={g0:g}", cuda)


@pytest.mark.parametrize("B,d", [(257, 64), (65, 48)])
def test_every_row_the_same_pair(B, d, cuda):
    """Every entry of the prediction is ONE scalar here, the sum of 2 d products, and "2e-5 of the largest entry" is then a
    relative bound on that scalar.  Where the products cancel no fp32 computation meets it: for the pair (7, 3) of the B = 65,
    d = 48 tables the value is -0.0666 out of products whose absolute values add up to 41.6, and the reference's own fp32 run is
    8.5e-6 of the value away from float64.  So the pair is chosen, from the float64 oracle alone, as the one of the tables whose
    prediction is largest against the sum of its absolute terms: the bar stays what it is everywhere."""
    tabs, W, b, uid, iid = _random_problem(d, B, seed=B)
    UO, IO, W64, b64 = (a.astype(np.float64) for a in (tabs[0], tabs[2], W, b))
    PU, PI = UO @ W64.T + b64, IO @ W64.T + b64
    pred = UO @ PI.T + PU @ IO.T
    terms = np.abs(UO) @ np.abs(PI).T + np.abs(PU) @ np.abs(IO).T
    u, i = np.unravel_index(np.argmax(np.abs(pred) / terms), pred.shape)
    assert abs(pred[u, i]) >= 0.25 * terms[u, i]
    uid[:], iid[:] = u, i
    _fused_check(tabs, W, b, uid, iid, 1.0, f"same pair B={B} d={d}", cuda)


def test_many_tiles_per_workgroup(cuda):
    """B = 4,099 at d = 64: 65 tiles, the last one with three rows"""
    _fused_check(*_random_problem(64, 4099, seed=4099, n_users=300, n_items=300), 3.0, "B=4099 d=64 g0=3", cuda)


def test_more_tiles_than_workgroups(cuda):
    """B = 64 * 512 + 65: the grid is capped at 512 workgroups, the first two walk over a second tile"""
    B = 64 * 512 + 65
    _fused_check(*_random_problem(32, B, seed=5, n_users=300, n_items=300), 1.0, f"B={B} d=32", cuda)


@pytest.mark.parametrize("d", [16, 64])
def test_zero_target_row_forward(d, cuda):
    from rechorus_amd import engine
    tabs, W, b, uid, iid = _random_problem(d, 65, seed=d)
    tabs[3][iid[1]] = 0.0      # a zero item target row: n(0) = 0, no NaN
    tabs[1][uid[64]] = 0.0
    t = [torch.from_numpy(a).to(cuda) for a in tabs]
    with torch.no_grad():
        loss, pred = engine.buir_fwd(*t, torch.from_numpy(W).to(cuda), torch.from_numpy(b).to(cuda), torch.from_numpy(uid).to(cuda),
                                     torch.from_numpy(iid).to(cuda))
    want = buir_np.table_grads(*tabs, W, b, uid, iid)
    assert np.isfinite(loss.item())
    _loss_close(loss.item(), want[0], f"zero target row d={d} loss")
    _close(pred.cpu().numpy(), want[1], f"zero target row d={d} pred")


def test_a_loss_on_the_prediction_raises(cuda):
    from rechorus_amd import nn as hnn
    tabs, W, b, uid, iid = _random_problem(16, 5, seed=1)
    t = [torch.from_numpy(a).to(cuda).requires_grad_(k in (0, 2)) for k, a in enumerate(tabs)]
    _, pred = hnn.buir_loss(*t, torch.from_numpy(W).to(cuda).requires_grad_(True), torch.from_numpy(b).to(cuda),
                            torch.from_numpy(uid).to(cuda), torch.from_numpy(iid).to(cuda))
    with pytest.raises(RuntimeError, match="does not require grad"):
        pred.sum().backward()
    with pytest.raises(RuntimeError, match="no backward"):
        hnn.buir_scores(t[0], t[2], torch.from_numpy(W).to(cuda), torch.from_numpy(b).to(cuda), torch.from_numpy(uid).to(cuda),
                        torch.from_numpy(iid).to(cuda)[:, None])


@pytest.mark.parametrize("m", [0.995, 0.9, 0.5])
def test_ema_is_bit_equal_to_the_separately_rounded_expression(m, cuda):
    from rechorus_amd import engine
    rng = np.random.default_rng(int(m * 1000))
    shapes = ((1001, 48), (37, 16))      # unequal sizes; 1001 * 48 and 37 * 16 floats, neither row count a multiple of 4
    t = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    o = [(a + 0.1 * rng.standard_normal(a.shape)).astype(np.float32) for a in t]
    td, od = [torch.from_numpy(a).to(cuda) for a in t], [torch.from_numpy(a).to(cuda) for a in o]
    engine.ema_update(td[0], od[0], td[1], od[1], m)
    for k in range(2):
        assert np.array_equal(td[k].cpu().numpy(), buir_np.ema(t[k], o[k], m)), (m, k)
        assert np.array_equal(od[k].cpu().numpy(), o[k])
    # flat views whose length is no multiple of the vector width (the scalar tail)
    a, b = torch.from_numpy(t[0].reshape(-1)[:4 * 601 + 3].copy()).to(cuda), torch.from_numpy(o[0].reshape(-1)[:4 * 601 + 3].copy()).to(cuda)
    c, e = torch.from_numpy(t[1].reshape(-1)[:17].copy()).to(cuda), torch.from_numpy(o[1].reshape(-1)[:17].copy()).to(cuda)
    engine.ema_update(a, b, c, e, m)
    assert np.array_equal(a.cpu().numpy(), buir_np.ema(t[0].reshape(-1)[:4 * 601 + 3], o[0].reshape(-1)[:4 * 601 + 3], m))
    assert np.array_equal(c.cpu().numpy(), buir_np.ema(t[1].reshape(-1)[:17], o[1].reshape(-1)[:17], m))


def test_reruns_are_bit_identical(cuda):
    from rechorus_amd import engine
    for B, d in ((4099, 64), (257, 128), (77, 32)):
        tabs, W, b, uid, iid = _random_problem(d, B, seed=B + d, n_users=200, n_items=150)
        args = [torch.from_numpy(a).to(cuda) for a in (*tabs, W, b, uid, iid)]
        runs = []
        for _ in range(2):
            loss, pred = engine.buir_fwd(*args)
            outs = engine.buir_bwd(torch.full((1,), 3.0, device=cuda), *args)
            runs.append([x.cpu().numpy().copy() for x in (loss.reshape(1), pred, *outs)])
        for x, y in zip(*runs):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_hipgraph_replay_plus_ema_is_bit_equal_to_eager(cuda):
    from rechorus_amd import graph as hgraph
    if not hgraph.usable():
        pytest.fail("hipGraph replay is disabled in this process")
    g = load_golden("buir_d32_sgd_b160")
    rng = np.random.default_rng(3)
    n_users, n_items, B = int(g["meta"][0]), int(g["meta"][1]), int(g["meta"][3])
    batches = [(g["uid"], g["iid"])] + [(rng.integers(1, n_users, B), rng.integers(1, n_items, (B, 1))) for _ in range(5)]
    results = []
    for replay in (False, True):
        m = _model(g, cuda)
        runner = _runner("Adam", 1e-3, 1e-6, graph=1)
        m.optimizer = runner._build_optimizer(m)
        m.train()
        step = hgraph.GraphedStep(m) if replay else None
        losses = []
        for u, i in batches:          # 2 eager warm-up steps, then the capture and its replay, then 3 more replays
            feed = _feed(u, i, cuda)
            if replay:
                losses.append(step.run(feed))
                runner._after_step(m)     # the target update follows every replay, outside the graph
            else:
                losses.append(_step(m, feed, runner).reshape(1))
        if replay:
            assert step.graph is not None
        torch.cuda.synchronize()
        results.append([*_state(m).values(), torch.cat(losses).cpu().numpy()])
    for a, b in zip(*results):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(results[0][1], g["UT0"])      # the targets did move


def test_test_all_ranks_equal_a_numpy_ranking(cuda):
    from rechorus_amd import engine
    g = load_golden("buir_d32_sgd_b160")
    m = _model(g, cuda)
    _load_state(m, g, "2")
    m.eval()
    n_users, n_items = int(g["meta"][0]), int(g["meta"][1])
    rng = np.random.default_rng(1)
    sets = {u: set(rng.integers(1, n_items, 5).tolist()) for u in range(n_users)}
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
    # the oracle's scores of every item (the reference's op order), clicked items masked, column 0 the target
    every = np.tile(np.arange(n_items), (len(users), 1))
    s64 = buir_np.scores_reference_order(g["UO2"], g["IO2"], g["W2"], g["b2"], users, every)
    want, near = [], []
    for r, (u, t) in enumerate(zip(users, targets)):
        pred = np.concatenate([[s64[r, t]], s64[r, 1:]])
        seen = np.array([c for c in sets[int(u)] if 1 <= c < n_items], dtype=np.int64)
        pred[seen] = -np.inf
        want.append(int((pred >= pred[0]).sum()))
        near.append(int((np.abs(pred - pred[0]) <= 1e-5 * (1 + abs(pred[0]))).sum() - 1))
    got = rank.cpu().numpy().astype(np.int64)
    assert (np.abs(got - np.array(want)) <= np.array(near)).all(), (got, want)
    assert max(want) > 1


@pytest.fixture(scope="module")
def synth_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("buir_data"))
    make_dataset(root, "synth", n_users=300, n_items=250, per_user=14, seed=5)
    return root


@pytest.mark.parametrize("pipeline_flag,test_all,graph", [("1", "0", "1"), ("1", "1", "1"), ("0", "0", "1"), ("1", "0", "0")])
def test_cli_trains_one_epoch(pipeline_flag, test_all, graph, synth_root, tmp_path, cuda, monkeypatch):
    import main
    from models.general.BUIR import BUIR
    from rechorus_amd import graph as hgraph, pipeline
    replays, sampled, moved = [], [], []
    run0, sample0, update0 = hgraph.GraphedStep.run, pipeline.DeviceDataset.sample_negatives, BUIR._update_target

    def update(self):
        before = self.user_target.weight.detach().clone() if not moved else None
        update0(self)
        moved.append(True if before is None else bool((before != self.user_target.weight.detach()).any().item()))
    # a run() that finds a captured graph replays it (warm-up steps and the capture itself run with graph still None)
    monkeypatch.setattr(hgraph.GraphedStep, "run", lambda self, b: replays.append(self.graph is not None) or run0(self, b))
    monkeypatch.setattr(pipeline.DeviceDataset, "sample_negatives", lambda self, seed: sampled.append(self.kind) or sample0(self, seed))
    monkeypatch.setattr(BUIR, "_update_target", update)
    log = str(tmp_path / "log" / "run.txt")
    res = main.run(["--model_name", "BUIR", "--emb_size", "64", "--lr", "1e-3", "--l2", "1e-6", "--dataset", "synth",
                    "--path", synth_root + "/", "--epoch", "1", "--batch_size", "256", "--num_workers", "0", "--regenerate", "1",
                    "--test_all", test_all, "--device_pipeline", pipeline_flag, "--graph", graph, "--log_file", log,
                    "--model_path", str(tmp_path / "m.pt"), "--topk", "5,10", "--save_final_results", "0"])
    text = open(log).read()
    assert re.search(r"Epoch 1\s+loss=[0-9.]+", text), text[-2000:]
    hr = float(re.search(r"HR@5:([0-9.]+)", res["test"]).group(1))
    assert 0.0 <= hr <= 1.0 and "NDCG@10" in res["test"]
    assert len(moved) >= 3 and moved[0]          # one target update per batch, and the first one moved the table
    if pipeline_flag == "1":
        assert sampled == ["general_unsampled"]   # the device pipeline serves training, no sampler launch behind it
    else:
        assert not sampled
    if graph == "1":
        assert len(replays) == len(moved) and sum(replays) >= 1      # captured, replayed, an update behind every run()
    else:
        assert not replays
