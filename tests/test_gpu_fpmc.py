"""GPU: FPMC's kernels, autograd node, trainer and model file against the float64 restatement (tests/fpmc_np.py) and the reference's
own numbers (tests/golden/fpmc_*.npz).

Shapes are the smallest at which a lane, slot or segment mistake shows: ids are drawn from 7 users and 11 items, so users, last
items and candidates repeat across tuples, a candidate repeats inside a tuple, a negative equals the positive, lid equals a candidate
and row 0 and the last row occur; every (d, C) at which rc_fpmc_fwd_bwd changes its layout (rc_fpmc_fwd_bwd_layout: lane-groups per
tuple, rows per lane-group, register / streaming) is run on both sides of the change.

Tolerances (conftest.assert_close: |got - want| <= rtol |want| + atol_scale max|want|): scores 1e-5 / 1e-5, everything else at most
2e-5 / 2e-5.  Looser, with the reason: the tables after an Adam / Adagrad step go through conftest.assert_update_close with
extra_atol = 1e-3 lr -- the step lr g / (sqrt(v) + eps) is ill-conditioned where |g| ~ eps, so a 1e-7-relative change of such a
gradient (another fp32 summation order) moves the step by 1e-4 relative; 0.1 % of the largest possible step bounds it.
RC_TOL_REPORT=<file> records every comparison (profiles/fpmc_tolerances.txt)."""
import argparse
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close, assert_update_close, golden_cases, load_golden
from synth_data import make_dataset

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import fpmc_np  # noqa: E402
from fpmc_np import TABLES  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

pytestmark = pytest.mark.gpu
CASES = golden_cases("fpmc_")
N_USERS, N_ITEMS = 7, 11
SHAPES = [(16, 1, 2), (32, 3, 5), (64, 7, 100), (128, 5, 33), (64, 130, 64), (64, 65, 65), (128, 2, 100)]
ATTR = {"UI": "ui_embeddings", "LI": "li_embeddings", "IU": "iu_embeddings", "IL": "il_embeddings"}


def _problem(d, B, Cn, seed=0, sd=0.3):
    """tables (TABLES order) and ids with the repetitions the module docstring names"""
    rng = np.random.default_rng(1000 * d + 10 * B + Cn + seed)
    T = [rng.normal(0, sd, (n, d)).astype(np.float32) for n in (N_USERS, N_ITEMS, N_ITEMS, N_ITEMS)]
    uid = rng.integers(0, N_USERS, B).astype(np.int64)
    lid = rng.integers(0, N_ITEMS, B).astype(np.int64)
    iid = rng.integers(0, N_ITEMS, (B, Cn)).astype(np.int64)
    iid[0, 1] = iid[0, 0]                      # a negative equals the positive
    if Cn >= 3:
        iid[0, 2] = iid[0, 1]                  # a candidate repeats inside the tuple
    lid[B - 1] = iid[B - 1, Cn - 1]            # lid equals a candidate
    uid[0], lid[0], iid[B - 1, 0] = 0, 0, 0    # row 0 ...
    uid[B - 1], iid[0, Cn - 1] = N_USERS - 1, N_ITEMS - 1      # ... and the last row occur
    if B >= 2:
        lid[1] = N_ITEMS - 1
    return T, uid, lid, iid


def _dev(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def _np(t):
    return t.detach().cpu().numpy()


def _layout_edges():
    """(d, C) on both sides of every change of rc_fpmc_fwd_bwd's layout, found by scanning the dispatcher"""
    from rechorus_amd import engine
    edges = []
    for d in (16, 32, 64, 128):
        prev = engine.fpmc_fwd_bwd_layout(d, 2)
        for Cn in range(3, 420):
            cur = engine.fpmc_fwd_bwd_layout(d, Cn)
            if cur != prev:
                edges += [(d, Cn - 1), (d, Cn)]
            prev = cur
        assert prev is None, d                                # the scan reached the streaming path
    return sorted(set(edges))


def _check_front(d, B, Cn, dev):
    from rechorus_amd import engine
    T, uid, lid, iid = _problem(d, B, Cn)
    want_pred = fpmc_np.scores(*T, uid, lid, iid)
    want_lv, want_g = fpmc_np.bpr(want_pred)
    want_u, want_l = fpmc_np.query_grads(T[2], T[3], iid, want_g)
    dT = _dev(dev, *T)
    ids = _dev(dev, uid, lid, iid)
    tag = f"d={d} B={B} C={Cn}"
    assert_close(_np(engine.fpmc_scores(*dT, *ids)), want_pred, what=f"scores {tag}")
    for want_p in (True, False):
        pred, lv, g, ug, lg = engine.fpmc_fwd_bwd(*dT, *ids, want_pred=want_p)
        if want_p:
            assert_close(_np(pred), want_pred, what=f"fwd_bwd pred {tag}")
        else:
            assert pred is None
        assert_close(_np(lv), want_lv, rtol=2e-5, atol_scale=2e-5, what=f"loss_vec {tag}")
        assert_close(_np(g), want_g, rtol=2e-5, atol_scale=2e-5, what=f"gpred {tag}")
        assert_close(_np(ug), want_u, rtol=2e-5, atol_scale=2e-5, what=f"ugrad {tag}")
        assert_close(_np(lg), want_l, rtol=2e-5, atol_scale=2e-5, what=f"lgrad {tag}")


@pytest.mark.parametrize("d,B,Cn", SHAPES)
def test_scores_and_fused_step_against_float64(d, B, Cn, cuda):
    _check_front(d, B, Cn, cuda)


def test_fused_step_on_both_sides_of_every_layout_change(cuda):
    from rechorus_amd import engine
    edges = _layout_edges()
    # per width: every lane-group count below a full wave, every rows-per-group bucket, and the register / streaming edge
    assert len(edges) >= 4 * 2 * 9 and (64, 100) in edges and (64, 101) in edges
    assert engine.fpmc_fwd_bwd_layout(64, 100) is not None and engine.fpmc_fwd_bwd_layout(64, 101) is None
    for d, Cn in edges:
        _check_front(d, 5, Cn, cuda)     # five tuples: more than one per wave where tuples share a wave, a ragged last workgroup


@pytest.mark.parametrize("Cn", [1, 1025])
def test_scores_at_one_candidate_and_past_a_thousand(Cn, cuda):
    from rechorus_amd import engine
    for d in (16, 64, 128):
        T, uid, lid, iid = _problem(d, 3, max(Cn, 2))
        iid = np.ascontiguousarray(iid[:, :Cn])
        got = engine.fpmc_scores(*_dev(cuda, *T), *_dev(cuda, uid, lid, iid))
        assert got.shape == (3, Cn)
        assert_close(_np(got), fpmc_np.scores(*T, uid, lid, iid), what=f"scores d={d} C={Cn}")


@pytest.mark.parametrize("d,B,Cn", SHAPES)
def test_dense_gradients_of_the_autograd_node_against_float64(d, B, Cn, cuda):
    from rechorus_amd import nn as hnn
    T, uid, lid, iid = _problem(d, B, Cn)
    params = [t.requires_grad_(True) for t in _dev(cuda, *T)]
    ids = _dev(cuda, uid, lid, iid)
    pred = hnn.fpmc_scores(*params, *ids)
    loss = hnn.bpr_loss(pred)
    loss.backward()
    want_lv, want_g = fpmc_np.bpr(fpmc_np.scores(*T, uid, lid, iid))
    assert_close(loss.item(), want_lv.mean(), rtol=2e-5, atol_scale=2e-5, what="loss")
    for k, p, want in zip(TABLES, params, fpmc_np.dense_grads(*T, uid, lid, iid, want_g)):
        assert_close(_np(p.grad), want, rtol=2e-5, atol_scale=2e-5, what=f"dense grad {k} d={d} B={B} C={Cn}")
    # an arbitrary loss on the scores: the node's backward takes any dL/dpred
    for p in params:
        p.grad = None
    w = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (B, Cn)).astype(np.float32)).to(cuda)
    (hnn.fpmc_scores(*params, *ids) * w).sum().backward()
    for k, p, want in zip(TABLES, params, fpmc_np.dense_grads(*T, uid, lid, iid, _np(w))):
        assert_close(_np(p.grad), want, rtol=2e-5, atol_scale=2e-5, what=f"dense grad {k} (weighted sum)")


def _trainer(T, dev, opt, lr, l2):
    from rechorus_amd import engine
    tabs = dict(zip(TABLES, _dev(dev, *T)))
    return engine.FpmcTrainer(*(tabs[k] for k in TABLES), opt=opt, lr=lr, l2=l2), tabs


@pytest.mark.parametrize("opt,lr,l2", [("SGD", 0.5, 1e-4), ("Adam", 1e-3, 1e-6), ("Adagrad", 0.01, 1e-4)])
@pytest.mark.parametrize("d,B,Cn", [(16, 1, 2), (64, 7, 100), (128, 5, 33), (64, 130, 64), (32, 3, 5)])
def test_trainer_step_against_float64(d, B, Cn, opt, lr, l2, cuda):
    T, uid, lid, iid = _problem(d, B, Cn)
    # rows outside the batch exist on every table: the batch's ids leave users / items out at these sizes only by chance, so one
    # user and one item are taken out of the batch by hand
    uid[uid == 3] = 2
    lid[lid == 5] = 4
    iid[iid == 5] = 4
    tr, tabs = _trainer(T, cuda, opt, lr, l2)
    ids = _dev(cuda, uid, lid, iid)
    before = {k: tabs[k].clone() for k in TABLES}
    want = dict(zip(TABLES, T))
    states = None
    for step_no in (1, 2):
        loss = tr.step(*ids)
        want_loss, want_new, states = fpmc_np.step(want, uid, lid, iid, opt, lr, l2, states, step_no)
        assert loss.shape == (1,) and tr.hyper.step == step_no
        assert_close(loss.item(), want_loss, rtol=2e-5, atol_scale=2e-5, what=f"{opt} loss step {step_no}")
        extra = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
        for k in TABLES:
            assert_update_close(_np(tabs[k]), want[k], want_new[k], what=f"{opt} {k} step {step_no}", rtol=2e-5, extra_atol=extra,
                                strict=True)
            for name, idx in (("m", 0), ("v", 1)):
                st = tr.state[k].get(name)
                if st is not None:
                    assert_close(_np(st), states[k][idx], rtol=2e-5, atol_scale=2e-5, what=f"{opt} {k} {name} step {step_no}")
        # continue from the float64 tables narrowed to fp32: step 2 checks one step from a non-zero state, not two compounded
        for k in TABLES:
            tabs[k].copy_(torch.from_numpy(want_new[k].astype(np.float32)))
            for name, idx in (("m", 0), ("v", 1)):
                if tr.state[k].get(name) is not None:
                    tr.state[k][name].copy_(torch.from_numpy(states[k][idx].astype(np.float32)))
        want = {k: want_new[k].astype(np.float32) for k in TABLES}
    # rows of every table (and of its state) outside the batch are bit-unchanged
    rows = {"UI": uid, "LI": lid, "IU": iid, "IL": iid}
    for k in TABLES:
        out = np.setdiff1d(np.arange(T[TABLES.index(k)].shape[0]), rows[k])
        assert out.size > 0, k
        out = torch.from_numpy(out).to(cuda)
        assert torch.equal(tabs[k][out].view(torch.int32), before[k][out].view(torch.int32)), k
        for st in tr.state[k].values():
            assert not st[out].any(), k


@pytest.mark.parametrize("opt", ["SGD", "Adam", "Adagrad"])
def test_two_runs_of_the_step_are_bit_identical(opt, cuda):
    T, uid, lid, iid = _problem(64, 130, 64)
    ids = _dev(cuda, uid, lid, iid)
    runs = []
    for _ in range(2):
        tr, tabs = _trainer(T, cuda, opt, 0.01, 1e-5)
        losses = [tr.step(*ids).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs.append([tabs[k] for k in TABLES] + losses + [s for k in TABLES for s in tr.state[k].values()])
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("d,B,Cn", [(32, 3, 5), (64, 130, 64), (128, 2, 100)])
def test_rowwise_sgd_without_weight_decay_agrees_with_the_dense_path_on_every_row(d, B, Cn, cuda):
    from rechorus_amd import nn as hnn
    T, uid, lid, iid = _problem(d, B, Cn)
    ids = _dev(cuda, uid, lid, iid)
    lr = 0.5
    tr, tabs = _trainer(T, cuda, "SGD", lr, 0.0)
    loss_row = tr.step(*ids)
    params = [t.requires_grad_(True) for t in _dev(cuda, *T)]
    loss_dense = hnn.bpr_loss(hnn.fpmc_scores(*params, *ids))
    loss_dense.backward()
    assert_close(loss_row.item(), loss_dense.item(), what="loss")
    for k, p in zip(TABLES, params):
        dense = p.detach() - lr * p.grad
        assert_update_close(_np(tabs[k]), _np(p), _np(dense), what=f"row-wise vs dense {k}", rtol=2e-5, strict=True)


def _model(g, dev, test_all=0):
    from models.sequential.FPMC import FPMC
    n_users, n_items, d, B, K, seed, redraw = (int(x) for x in g["meta"])
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=K, dropout=0, test_all=test_all, emb_size=d, history_max=20)
    m = FPMC(args, SimpleNamespace(n_users=n_users, n_items=n_items)).to(dev)
    with torch.no_grad():
        for k in TABLES:
            getattr(m, ATTR[k]).weight.copy_(torch.from_numpy(g[k + "0"]))
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
    lr, l2 = (float(x) for x in g["hyper"])
    opt = str(g["opt"])
    B = int(g["meta"][3])
    uid, lid, iid = _dev(cuda, g["uid"], g["lid"], g["iid"])
    feed = {"user_id": uid, "last_item_id": lid, "item_id": iid, "batch_size": B, "phase": "train"}
    m = _model(g, cuda)
    m.train()
    out = m(feed)
    assert_close(_np(out["prediction"]), g["pred"], what=case + " pred")
    loss = m.loss(out)
    loss.backward()
    assert_close(loss.item(), float(g["loss"]), what=case + " loss")
    for k in TABLES:
        assert_close(_np(getattr(m, ATTR[k]).weight.grad), g["G" + k], rtol=2e-5, atol_scale=2e-5, what=f"{case} G{k}")
    extra = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
    # the dense path: the optimizer BaseRunner builds, one step
    m2 = _model(g, cuda)
    m2.optimizer = _runner(opt, lr, l2)._build_optimizer(m2)
    m2.train()
    m2.optimizer.zero_grad()
    m2.loss(m2(feed)).backward()
    m2.optimizer.step()
    for k in TABLES:
        assert_update_close(_np(getattr(m2, ATTR[k]).weight), g[k + "0"], g[k + "1"], what=f"{case} dense step {k}", rtol=2e-5,
                            extra_atol=extra, strict=True)
    # the row-wise path: the first step of a row of the batch is torch.optim's (zero state); the other rows do not move
    m3 = _model(g, cuda)
    loss3 = m3.hip_train_step(feed, opt, lr, l2)
    assert_close(loss3.item(), float(g["loss"]), what=case + " row-wise loss")
    rows = {"UI": g["uid"], "LI": g["lid"], "IU": g["iid"], "IL": g["iid"]}
    for k in TABLES:
        r = np.unique(rows[k])
        W = _np(getattr(m3, ATTR[k]).weight)
        assert_update_close(W[r], g[k + "0"][r], g[k + "1"][r], what=f"{case} row-wise step {k}", rtol=2e-5, extra_atol=extra, strict=True)
        rest = np.setdiff1d(np.arange(W.shape[0]), r)
        assert np.array_equal(W[rest].view(np.int32), g[k + "0"][rest].view(np.int32)), (case, k)


# ---- the model file through main.py's classes on a synthetic SeqReader corpus ------------------------------------------------------

@pytest.fixture(scope="module")
def synth_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("fpmc_data"))
    make_dataset(root, "synth", n_users=120, n_items=90, per_user=8, n_neg=99, seed=11)
    return root


@pytest.mark.parametrize("engine_flag,test_all", [("dense", "0"), ("rowwise", "1")])
def test_cli_trains_one_epoch(engine_flag, test_all, synth_root, tmp_path, cuda, monkeypatch):
    import main
    from rechorus_amd import engine
    steps, fwd = [], []
    step0, fwd0 = engine.FpmcTrainer.step, engine.fpmc_scores
    monkeypatch.setattr(engine.FpmcTrainer, "step", lambda self, *a, **k: steps.append(1) or step0(self, *a, **k))
    monkeypatch.setattr(engine, "fpmc_scores", lambda *a, **k: fwd.append(a[-1].shape[1]) or fwd0(*a, **k))
    log = str(tmp_path / "log" / "run.txt")
    res = main.run(["--model_name", "FPMC", "--emb_size", "64", "--lr", "1e-3", "--l2", "1e-6", "--history_max", "20",
                    "--dataset", "synth", "--path", synth_root + "/", "--epoch", "1", "--batch_size", "256", "--num_workers", "0",
                    "--regenerate", "1", "--test_all", test_all, "--engine", engine_flag, "--num_neg", "4", "--log_file", log,
                    "--model_path", str(tmp_path / "m.pt"), "--topk", "5,10", "--save_final_results", "0"])
    text = open(log).read()
    m = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", text)
    assert m and np.isfinite(float(m.group(1))), text[-2000:]
    hr = float(re.search(r"HR@5:([0-9.]+)", res["test"]).group(1))
    assert 0.0 <= hr <= 1.0 and "NDCG@10" in res["test"]
    assert bool(steps) == (engine_flag == "rowwise")          # the row-wise trainer trained, or the autograd node did
    assert (5 in fwd) == (engine_flag == "dense")
    # evaluation went through rc_fpmc_scores: the whole catalogue (91 rows) under --test_all, else the files' sampled negatives
    eval_widths = set(fwd) - {5}
    assert eval_widths == {91} if test_all == "1" else (eval_widths and 91 not in eval_widths and min(eval_widths) > 50)


def _corpus_and_model(synth_root, dev, test_all):
    from helpers.SeqReader import SeqReader
    from models.sequential.FPMC import FPMC
    args = SimpleNamespace(path=synth_root + "/", dataset="synth", sep="\t", device=dev, model_path="", buffer=1, num_neg=4, dropout=0,
                           test_all=test_all, emb_size=32, history_max=20)
    corpus = SeqReader(args)
    torch.manual_seed(3)
    model = FPMC(args, corpus).to(dev)
    with torch.no_grad():
        for k in TABLES:
            getattr(model, ATTR[k]).weight.normal_(0, 0.3)
    return corpus, model


@pytest.mark.parametrize("test_all", [0, 1])
def test_device_feed_equals_the_host_feed_and_ranks_equal_float64_scoring(test_all, synth_root, cuda):
    from rechorus_amd import engine, pipeline
    from models.sequential.FPMC import FPMC
    corpus, model = _corpus_and_model(synth_root, cuda, test_all)
    T = [_np(getattr(model, ATTR[k]).weight) for k in TABLES]
    runner = _runner("Adam", 1e-3, 0.0)
    for phase in ("train", "dev", "test"):
        ds = FPMC.Dataset(model, corpus, phase)
        assert pipeline.dataset_kind(ds) == "last_item"
        if phase == "train":
            ds.actions_before_epoch()
        host = ds.collate_batch([ds._get_feed_dict(i) for i in range(len(ds))])
        dd = pipeline.DeviceDataset(ds, cuda)
        if phase == "train":
            dd.sample_negatives(seed=1)
        feed = dd.feed(torch.arange(len(ds), device=cuda))
        assert sorted(feed) == sorted(host)
        assert feed["batch_size"] == host["batch_size"] and feed["phase"] == host["phase"] == phase
        assert torch.equal(feed["user_id"].cpu(), host["user_id"]) and torch.equal(feed["last_item_id"].cpu(), host["last_item_id"])
        if phase == "train":      # each side draws its own negatives
            assert torch.equal(feed["item_id"][:, 0].cpu(), host["item_id"][:, 0]) and feed["item_id"].shape == host["item_id"].shape
            continue
        assert torch.equal(feed["item_id"].cpu(), host["item_id"])
        # evaluation: the runner's ranks against ranks of the float64 scores
        uid, lid, iid = (host[k].numpy() for k in ("user_id", "last_item_id", "item_id"))
        want = fpmc_np.scores(*T, uid, lid, iid)
        ds.prepare()
        if test_all:
            assert iid.shape[1] == corpus.n_items
            for r, u in enumerate(uid):       # clicked items are masked by item id = column (reference BaseRunner.py:243-250)
                seen = list(corpus.train_clicked_set[u] | corpus.residual_clicked_set[u])
                want[r, seen] = -np.inf
            got = runner._streamed_test_all_ranks(ds)
        else:
            got = engine.target_rank(runner._predict_device(ds).contiguous())
        want_rank = fpmc_np.ranks(want)
        # a rank may differ only in a row where a competitor is closer to the target than the score tolerance (1e-5 of the scale)
        finite = np.where(np.isfinite(want), want, 0.0)
        gap = np.abs(np.where(np.isfinite(want[:, 1:]), want[:, 1:] - want[:, :1], np.inf)).min(axis=1)
        clear = gap > 2e-5 * np.abs(finite).max()
        assert clear.mean() > 0.99
        assert np.array_equal(_np(got).astype(np.int64)[clear], want_rank[clear]), phase
