"""GPU: CFKG's kernels, autograd node, trainer and model file against the float64 restatement (tests/cfkg_np.py) and the reference's
own numbers (tests/golden/cfkg_*.npz).

Shapes are the smallest at which a lane, slot or segment mistake shows: ids are drawn from a 40-row entity table (9 users first) so
rows repeat, the same entity is a head in one row and a tail in another, row 0 has t' = t (an exact tie: ACTIVE, and a score
difference of exactly 0), row 1's head row is its tail row, row 2's h' is another row's t, the first and the last table row occur,
and B runs over both sides of every multiple of the rows one workgroup of rc_cfkg_fwd_bwd takes (rc_cfkg_fwd_bwd_rows_per_block).
A hinge that could flip between fp32 and float64 is not excluded but never drawn: rows whose float64 |x| is below
1e-4 (|pos| + |neg| + margin) get new corrupted ids when the batch is made (the generator's condition for the goldens).

Tolerances (conftest.assert_close: |got - want| <= rtol |want| + atol_scale max|want|): 2e-6 / 2e-6 for scores, losses and
gradients = 10 x the largest error of the reference's own fp32 run against its float64 run on the goldens (2.0e-7, on GR;
profiles/cfkg_tolerances.txt).  The tables after an optimizer step go through conftest.assert_update_close at rtol 2e-5 with
extra_atol = 1e-3 lr for Adam / Adagrad, as every trainer test of the project: the step lr g / (sqrt(v) + eps) is ill-conditioned
where |g| ~ eps.  Nothing is excluded."""
import argparse
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close, assert_update_close, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cfkg_np  # noqa: E402
from cfkg_np import STATE_KEYS  # noqa: E402
from slrc_data import make_kg_dataset  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

pytestmark = pytest.mark.gpu
CASES = golden_cases("cfkg_d")
N_USERS, N_ROWS = 9, 40
T = dict(rtol=2e-6, atol_scale=2e-6)


def _dev(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _np(t).view(np.int32)


def _problem(d, n_rel, B, margin, seed=0):
    """tables and a [B, 4] training feed with the hand-set rows of the module docstring; no hinge near enough to 0 to flip"""
    rng = np.random.default_rng(100000 * d + 1000 * n_rel + 10 * B + seed)
    E = rng.normal(0, 0.3, (N_ROWS, d)).astype(np.float32)
    R = rng.normal(0, 0.3, (n_rel, d)).astype(np.float32)
    r = rng.integers(0, n_rel, B).astype(np.int64)
    h, hn = rng.integers(0, N_ROWS, B).astype(np.int64), rng.integers(0, N_ROWS, B).astype(np.int64)
    t, tn = rng.integers(N_USERS, N_ROWS, B).astype(np.int64), rng.integers(N_USERS, N_ROWS, B).astype(np.int64)
    fixed = np.zeros((B, 2), bool)           # pairs set by hand: not redrawn
    tn[0] = t[0]
    fixed[0, 0] = True
    if B >= 3:
        h[1] = t[1]
        hn[2], t[B - 1] = N_ROWS - 1, N_ROWS - 1      # the last row, as a corrupted head and as another row's tail
        h[2] = 0
        fixed[2, 1] = True
        r[B - 1] = n_rel - 1
    for _ in range(100):
        pred = cfkg_np.scores(E, R, np.stack([h, h, h, hn], 1), np.stack([t, t, tn, t], 1), np.repeat(r[:, None], 4, 1))
        x = margin - pred[:, :2] + pred[:, 2:]
        near = (np.abs(x) < 1e-4 * (np.abs(pred[:, :2]) + np.abs(pred[:, 2:]) + margin)) & ~np.stack([tn == t, hn == h], 1)
        if not near.any():
            break
        assert not (near & fixed).any()
        tn = np.where(near[:, 0], rng.integers(N_USERS, N_ROWS, B), tn)
        hn = np.where(near[:, 1], rng.integers(0, N_ROWS, B), hn)
    else:
        raise AssertionError("no batch without a near-tie hinge")
    return E, R, np.stack([h, h, h, hn], 1), np.stack([t, t, tn, t], 1), np.repeat(r[:, None], 4, 1)


def _batches(d):
    from rechorus_amd import engine
    rpb = engine.cfkg_fwd_bwd_rows_per_block(d)
    assert rpb == {16: 256, 32: 128, 64: 64, 128: 32}[d]
    return sorted({1, 3, 77, 130, rpb - 1, rpb, rpb + 1, 2 * rpb, 2 * rpb + 1})


@pytest.mark.parametrize("n_rel", [1, 4, 8])
@pytest.mark.parametrize("d", [16, 32, 64, 128])
def test_fused_front_against_float64(d, n_rel, cuda):
    from rechorus_amd import engine
    for B in _batches(d):
        for margin in (0.0, 1.0):
            E, R, head, tail, rel = _problem(d, n_rel, B, margin)
            want_pred, want_lv, want_rows, want_GR = cfkg_np.front(E, R, head, tail, rel, margin)
            dE, dR = _dev(cuda, E, R)
            cols = _dev(cuda, *cfkg_np.quad(head, tail, rel))
            tag = f"d={d} n_rel={n_rel} B={B} margin={margin}"
            pred, lv, rows, GR = engine.cfkg_fwd_bwd(dE, dR, *cols, margin=margin)
            assert_close(_np(pred), want_pred, what=f"pred {tag}", **T)
            assert_close(_np(lv), want_lv, what=f"loss_vec {tag}", **T)
            assert_close(_np(engine.reduce_sum(lv, 1.0 / B)).item(), want_lv.mean(), what=f"loss {tag}", **T)
            assert_close(_np(rows), want_rows, what=f"grows {tag}", **T)
            assert_close(_np(GR), want_GR, what=f"GR {tag}", **T)
            p = _np(pred)
            assert np.array_equal(p[:, 0], p[:, 1]) and p[0, 2] == p[0, 0]        # t' = t: a difference of exactly 0
            if margin == 0:      # ... and the tie is ACTIVE: t' takes w b, t takes w (-(s1 + s2) a + s2 c)
                assert np.abs(_np(rows)[0, 3]).max() > 0 and _np(lv)[0] >= 0
                assert_close(_np(rows)[0, 3], want_rows[0, 3], what=f"tie row {tag}", **T)
            # the same expression as the score kernel, bit for bit; without pred the rest is the same bits; so is a second run
            ids = _dev(cuda, head, tail, rel)
            assert np.array_equal(_bits(engine.cfkg_scores(dE, dR, *ids)), _bits(pred)), tag
            none, lv2, rows2, GR2 = engine.cfkg_fwd_bwd(dE, dR, *cols, margin=margin, want_pred=False)
            assert none is None
            for a, b in ((lv, lv2), (rows, rows2), (GR, GR2)):
                assert np.array_equal(_bits(a), _bits(b)), tag


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("Cn", [1, 100, 1025])
@pytest.mark.parametrize("d", [16, 32, 64, 128])
def test_scores_against_float64(d, Cn, shared, cuda):
    """the evaluation layout (one head and relation per row: read once per wave) and distinct heads, C = 1, a wave's share and past
    one workgroup's candidates; a row whose head changes in its LAST column takes the general path in that wave only"""
    from rechorus_amd import engine
    rng = np.random.default_rng(d + Cn)
    B, n_rel = 5, 4
    E, R = rng.normal(0, 0.3, (N_ROWS, d)).astype(np.float32), rng.normal(0, 0.3, (n_rel, d)).astype(np.float32)
    tail = rng.integers(N_USERS, N_ROWS, (B, Cn)).astype(np.int64)
    tail[0, 0], tail[B - 1, Cn - 1] = N_USERS, N_ROWS - 1
    if shared:
        head = np.repeat(rng.integers(0, N_USERS, B)[:, None], Cn, 1).astype(np.int64)
        rel = np.repeat(rng.integers(0, n_rel, B)[:, None], Cn, 1).astype(np.int64)
        head[1, Cn - 1] = (head[1, 0] + 1) % N_USERS
        rel[2, Cn // 2] = (rel[2, 0] + 1) % n_rel
    else:
        head, rel = rng.integers(0, N_ROWS, (B, Cn)).astype(np.int64), rng.integers(0, n_rel, (B, Cn)).astype(np.int64)
    head[0, 0], rel[B - 1, Cn - 1] = 0, n_rel - 1
    got = engine.cfkg_scores(*_dev(cuda, E, R, head, tail, rel))
    assert_close(_np(got), cfkg_np.scores(E, R, head, tail, rel), what=f"scores d={d} C={Cn} shared={shared}", **T)


@pytest.mark.parametrize("d,n_rel,B,Cn", [(16, 1, 1, 1), (32, 4, 3, 100), (64, 4, 77, 4), (64, 8, 2, 1025), (128, 8, 130, 5)])
def test_dense_gradients_of_the_autograd_node_against_float64(d, n_rel, B, Cn, cuda):
    from rechorus_amd import nn as hnn
    rng = np.random.default_rng(d + B + Cn)
    E, R = rng.normal(0, 0.3, (N_ROWS, d)).astype(np.float32), rng.normal(0, 0.3, (n_rel, d)).astype(np.float32)
    head, tail = rng.integers(0, N_ROWS, (B, Cn)).astype(np.int64), rng.integers(0, N_ROWS, (B, Cn)).astype(np.int64)
    rel = rng.integers(0, n_rel, (B, Cn)).astype(np.int64)
    head[0, 0], tail[0, 0] = 0, N_ROWS - 1
    if Cn >= 2:
        head[0, 1] = tail[0, 1]                  # head row = tail row: the two contributions cancel in E's gradient
        tail[B - 1, 1] = head[0, 0]              # a head of one candidate is the tail of another
    w = rng.normal(0, 1, (B, Cn)).astype(np.float32)
    dE, dR = (x.requires_grad_() for x in _dev(cuda, E, R))
    pred = hnn.cfkg_scores(dE, dR, *_dev(cuda, head, tail, rel))
    assert_close(_np(pred), cfkg_np.scores(E, R, head, tail, rel), what="node forward", **T)
    (pred * _dev(cuda, w)[0]).sum().backward()
    GE, GR = cfkg_np.dense_grads(E, R, head, tail, rel, w)
    assert_close(_np(dE.grad), GE, what=f"GE d={d} B={B} C={Cn}", **T)
    assert_close(_np(dR.grad), GR, what=f"GR d={d} B={B} C={Cn}", **T)


@pytest.mark.parametrize("d,n_rel,B,margin,opt,lr,l2", [(16, 1, 3, 0.0, "SGD", 0.1, 1e-4), (64, 4, 77, 1.0, "Adam", 1e-3, 1e-5),
                                                      (32, 8, 130, 0.5, "Adagrad", 0.01, 1e-4), (128, 4, 33, 0.0, "Adam", 1e-3, 0.0)])
def test_trainer_step_against_float64(d, n_rel, B, margin, opt, lr, l2, cuda):
    """two steps: E row-wise (rows outside the batch bit-identical, their state untouched), R densely (every row, every step)"""
    from rechorus_amd import engine
    E, R, head, tail, rel = _problem(d, n_rel, B, margin, seed=6)      # (a seed at which step 2's hinges are off the edge too)
    dE, dR = _dev(cuda, E, R)
    ids = _dev(cuda, head, tail, rel)
    tr = engine.CfkgTrainer(dE, dR, margin=margin, opt=opt, lr=lr, l2=l2)
    wE, wR, st = E.astype(np.float64), R.astype(np.float64), None
    touched = np.unique(np.stack(cfkg_np.quad(head, tail, rel)[:4]))
    rest = np.setdiff1d(np.arange(N_ROWS), touched)
    extra = 1e-3 * lr if opt != "SGD" else 0.0
    for step_no in (1, 2):
        pE, pR = wE, wR
        want_loss, wE, wR, st = cfkg_np.step(wE, wR, head, tail, rel, margin, opt, lr, l2, st, step_no)
        if step_no == 2:      # the second step's hinges are evaluated on moved tables: they must not sit on the edge either
            p = cfkg_np.scores(pE, pR, head, tail, rel)
            x = margin - p[:, :2] + p[:, 2:]
            assert not ((np.abs(x) < 1e-4 * (np.abs(p[:, :2]) + np.abs(p[:, 2:]) + margin)) & (x != 0)).any()
        loss = tr.step(*ids)
        assert_close(loss.item(), want_loss, what=f"{opt} loss step {step_no}", **T)
        assert_update_close(_np(dE), pE, wE, what=f"{opt} E step {step_no}", rtol=2e-5, extra_atol=extra, strict=True)
        assert_update_close(_np(dR), pR, wR, what=f"{opt} R step {step_no}", rtol=2e-5, extra_atol=extra, strict=True)
        assert np.array_equal(_bits(dE)[rest], E.view(np.int32)[rest])
        for s in tr.state["E"].values():
            assert not _np(s)[rest].any()


@pytest.mark.parametrize("d,n_rel,B", [(16, 1, 3), (64, 4, 130), (128, 8, 77)])
def test_rowwise_sgd_without_weight_decay_agrees_with_the_dense_path_on_every_row(d, n_rel, B, cuda):
    from rechorus_amd import engine, nn as hnn
    margin, lr = 0.5, 0.1
    E, R, head, tail, rel = _problem(d, n_rel, B, margin, seed=9)
    ids = _dev(cuda, head, tail, rel)
    dE, dR = (x.requires_grad_() for x in _dev(cuda, E, R))
    pred = hnn.cfkg_scores(dE, dR, *ids)
    torch.nn.MarginRankingLoss(margin=margin)(pred[:, :2].flatten(), pred[:, 2:].flatten(), torch.ones(2 * B, device=cuda)).backward()
    wantE, wantR = E - lr * _np(dE.grad), R - lr * _np(dR.grad)
    rE, rR = _dev(cuda, E, R)
    engine.CfkgTrainer(rE, rR, margin=margin, opt="SGD", lr=lr, l2=0.0).step(*ids)
    assert_update_close(_np(rE), E, wantE, what="E", rtol=2e-5, strict=True)
    assert_update_close(_np(rR), R, wantR, what="R", rtol=2e-5, strict=True)


@pytest.mark.parametrize("opt", ["SGD", "Adam", "Adagrad"])
def test_two_runs_of_the_step_are_bit_identical(opt, cuda):
    from rechorus_amd import engine
    E, R, head, tail, rel = _problem(64, 4, 300, 0.5, seed=13)
    runs = []
    for _ in range(2):
        dE, dR = _dev(cuda, E, R)
        ids = _dev(cuda, head, tail, rel)
        tr = engine.CfkgTrainer(dE, dR, margin=0.5, opt=opt, lr=0.01, l2=1e-4)
        losses = [tr.step(*ids).clone() for _ in range(3)]
        runs.append([_bits(x) for x in (dE, dR, *losses, *tr.state["E"].values(), *tr.state["R"].values())])
    assert len(runs[0]) == len(runs[1]) and all(np.array_equal(a, b) for a, b in zip(*runs))


# ---- the goldens ---------------------------------------------------------------------------------------------------------------------

def _model(g, dev, test_all=0):
    from models.general.CFKG import CFKG
    n_users, n_items, n_entities, n_rel, d, B, seed, redraw = (int(x) for x in g["meta"])
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=1, dropout=0, test_all=test_all, emb_size=d,
                           margin=float(g["hyper"][2]))
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, n_entities=n_entities, n_relations=n_rel)
    m = CFKG(args, corpus).to(dev)
    m.load_state_dict({STATE_KEYS[k]: torch.from_numpy(g[k + "0"]) for k in ("E", "R")})     # a reference state_dict loads
    return m


def _runner(opt, lr, l2):
    from helpers.BaseRunner import BaseRunner
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.train, a.log_file = 1, "/tmp/rechorus_amd_test/log.txt"
    a.optimizer, a.lr, a.l2, a.graph, a.engine = opt, lr, l2, 0, "dense"
    return BaseRunner(a)


@pytest.mark.parametrize("case", CASES)
def test_golden_case(case, cuda):
    g = load_golden(case)
    lr, l2, margin = (float(x) for x in g["hyper"])
    opt = str(g["opt"])
    B = g["head"].shape[0]
    head, tail, rel = _dev(cuda, g["head"], g["tail"], g["rel"])
    feed = {"head_id": head, "tail_id": tail, "relation_id": rel, "batch_size": B, "phase": "train"}
    m = _model(g, cuda)
    m.train()
    out = m(feed)
    assert_close(_np(out["prediction"]), g["pred"], what=case + " pred", **T)
    loss = m.loss(out)
    loss.backward()
    assert_close(loss.item(), float(g["loss"]), what=case + " loss", **T)
    sd = dict(m.named_parameters())
    for k in ("E", "R"):
        assert_close(_np(sd[STATE_KEYS[k]].grad), g["G" + k], what=f"{case} G{k}", **T)
    # the fused front on the same feed: the reference's pred, loss and (summed per row) gradients
    from rechorus_amd import engine
    E0, R0 = _dev(cuda, g["E0"], g["R0"])
    cols = _dev(cuda, *cfkg_np.quad(g["head"], g["tail"], g["rel"]))
    pred, lv, rows, GR = engine.cfkg_fwd_bwd(E0, R0, *cols, margin=margin)
    assert_close(_np(pred), g["pred"], what=case + " fused pred", **T)
    assert_close(engine.reduce_sum(lv, 1.0 / B).item(), float(g["loss"]), what=case + " fused loss", **T)
    assert_close(_np(GR), g["GR"], what=case + " fused GR", **T)
    acc = np.zeros(g["E0"].shape)
    np.add.at(acc, np.stack(cfkg_np.quad(g["head"], g["tail"], g["rel"])[:4], 1).reshape(-1), _np(rows).astype(np.float64).reshape(4 * B, -1))
    assert_close(acc, g["GE"], what=case + " fused GE", **T)
    if margin == 0:      # the exact tie of row 0 came back active
        assert _np(pred)[0, 0] == _np(pred)[0, 2] and np.abs(_np(rows)[0, 3]).max() > 0
    extra = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
    # the dense path: the optimizer BaseRunner builds, one step
    m2 = _model(g, cuda)
    m2.optimizer = _runner(opt, lr, l2)._build_optimizer(m2)
    m2.train()
    m2.optimizer.zero_grad()
    m2.loss(m2(feed)).backward()
    m2.optimizer.step()
    sd2 = m2.state_dict()
    for k in ("E", "R"):
        assert_update_close(_np(sd2[STATE_KEYS[k]]), g[k + "0"], g[k + "1"], what=f"{case} dense step {k}", rtol=2e-5, extra_atol=extra,
                            strict=True)
    # the row-wise path: the first step of a row of the batch is torch.optim's (zero state), the other rows of E do not move; R is
    # dense and equals torch.optim's on every row
    m3 = _model(g, cuda)
    loss3 = m3.hip_train_step(feed, opt, lr, l2)
    assert_close(loss3.item(), float(g["loss"]), what=case + " row-wise loss", **T)
    sd3 = m3.state_dict()
    W = _np(sd3[STATE_KEYS["E"]])
    r = np.unique(np.concatenate([g["head"].reshape(-1), g["tail"].reshape(-1)]))
    assert_update_close(W[r], g["E0"][r], g["E1"][r], what=f"{case} row-wise step E", rtol=2e-5, extra_atol=extra, strict=True)
    rest = np.setdiff1d(np.arange(W.shape[0]), r)
    assert len(rest) and np.array_equal(W[rest].view(np.int32), g["E0"][rest].view(np.int32)), case
    assert_update_close(_np(sd3[STATE_KEYS["R"]]), g["R0"], g["R1"], what=f"{case} row-wise step R", rtol=2e-5, extra_atol=extra, strict=True)
    assert sorted(sd3.keys()) == sorted(g["state_keys"].tolist())


# ---- the model file through main.py on a synthetic KGReader corpus -------------------------------------------------------------------

@pytest.fixture(scope="module")
def kg_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("cfkg_data"))
    make_kg_dataset(root, "synth_kg", n_users=40, n_items=30, per_user=7, n_neg=20, seed=11)
    return root


@pytest.mark.parametrize("include_attr", ["0", "1"])
@pytest.mark.parametrize("test_all", ["0", "1"])
@pytest.mark.parametrize("engine_flag", ["dense", "rowwise"])
def test_cli_trains_one_epoch(engine_flag, test_all, include_attr, kg_root, tmp_path, cuda, monkeypatch):
    import main
    from rechorus_amd import engine
    steps, calls = [], []
    step0, fwd0 = engine.CfkgTrainer.step, engine.cfkg_scores

    def scores(E, R, head, tail, rel):
        pred = fwd0(E, R, head, tail, rel)
        calls.append((head.shape[1], R.shape[0], E.shape[0]))
        if head.shape[1] != 4:      # an evaluation batch: ranks of column 0 against float64 scoring of the SAME tables
            want = cfkg_np.scores(_np(E), _np(R), _np(head), _np(tail), _np(rel))
            got = _np(pred)
            assert np.array_equal((got[:, 1:] > got[:, :1]).sum(1), (want[:, 1:] > want[:, :1]).sum(1))
            assert (_np(head) == _np(head)[:, :1]).all() and not _np(rel).any() and _np(tail).min() >= 41
        return pred
    monkeypatch.setattr(engine.CfkgTrainer, "step", lambda self, *a, **k: steps.append(1) or step0(self, *a, **k))
    monkeypatch.setattr(engine, "cfkg_scores", scores)
    log = str(tmp_path / "log" / "run.txt")
    res = main.run(["--model_name", "CFKG", "--emb_size", "64", "--margin", "1", "--include_attr", include_attr, "--lr", "1e-3",
                    "--l2", "1e-6", "--dataset", "synth_kg", "--path", kg_root + "/", "--epoch", "1", "--batch_size", "64",
                    "--num_workers", "0", "--regenerate", "1", "--test_all", test_all, "--engine", engine_flag,
                    "--log_file", log, "--model_path", str(tmp_path / "m.pt"), "--topk", "5,10", "--save_final_results", "0"])
    text = open(log).read()
    m = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", text)
    assert m and np.isfinite(float(m.group(1))), text[-2000:]
    hr = float(re.search(r"HR@5:([0-9.]+)", res["test"]).group(1))
    assert 0.0 <= hr <= 1.0 and "NDCG@10" in res["test"]
    assert bool(steps) == (engine_flag == "rowwise")          # the row-wise trainer trained, or the autograd node did
    widths = {c[0] for c in calls}
    assert (4 in widths) == (engine_flag == "dense")
    # evaluation went through rc_cfkg_scores: the whole catalogue (31 rows) under --test_all, else the files' 20 sampled negatives
    assert (widths - {4}) == ({31} if test_all == "1" else {21})
    assert {c[1] for c in calls} == ({4} if include_attr == "1" else {3})      # "buy", two item relations, and the attribute
