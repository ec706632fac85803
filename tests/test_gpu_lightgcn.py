"""GPU: LightGCN on the HIP engine (rc_lgcn_propagate_fwd/bwd) against the reference's goldens (tests/golden/make_golden_lightgcn.py)
and float64 restatements: forward tables, scores, loss, gradients, two fit() iterations, forced chunk splitting, skewed and
Amazon-Book-shaped graphs, hipGraph replay, the evaluation cache, --test_all ranks and the CLI.  torch.sparse.mm raises throughout."""
import argparse
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close, assert_update_close, golden_cases, load_golden
from synth_data import make_dataset, make_impression_dataset

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

pytestmark = pytest.mark.gpu
CASES = golden_cases("lightgcn_")


@pytest.fixture(autouse=True)
def no_torch_sparse(monkeypatch):
    """nothing on the path may fall back to torch's sparse products"""
    def refuse(*a, **k):
        raise AssertionError("torch.sparse.mm called")
    monkeypatch.setattr(torch.sparse, "mm", refuse)


def _clicked(g):
    out = {}
    for u, i in zip(g["train_u"].tolist(), g["train_i"].tolist()):
        out.setdefault(u, set()).add(i)
    return out


def _model(g, dev, chunk=None, impression=False):
    from models.general.LightGCN import LightGCN, LightGCNImpression
    n_users, n_items, d, L, _, K, _ = (int(x) for x in g["meta"])
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=K, dropout=0, test_all=0, emb_size=d, n_layers=L)
    if impression:
        args.loss_n = "BPR"
        args.train_max_pos_item = args.test_max_pos_item = 1
        args.train_max_neg_item = args.test_max_neg_item = K
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, train_clicked_set=_clicked(g))
    m = (LightGCNImpression if impression else LightGCN)(args, corpus)
    if chunk is not None:
        m.encoder.set_chunk(chunk)
    m = m.to(dev)
    with torch.no_grad():
        m.encoder.embedding_dict["user_emb"].copy_(torch.from_numpy(g["U0"]))
        m.encoder.embedding_dict["item_emb"].copy_(torch.from_numpy(g["I0"]))
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
    """one iteration of BaseRunner.fit's dense loop (helpers/BaseRunner.py: zero_grad, forward, loss, backward, step)"""
    m.optimizer.zero_grad()
    loss = m.loss(m(batch))
    loss.backward()
    m.optimizer.step()
    return loss.detach()


def _tables(m):
    e = m.encoder.embedding_dict
    return e["user_emb"].detach().cpu().numpy(), e["item_emb"].detach().cpu().numpy()


def _check_case(case, cuda, chunk=None):
    g = load_golden(case)
    n_users = int(g["meta"][0])
    lr, l2 = (float(x) for x in g["hyper"])
    opt = str(g["opt"])
    m = _model(g, cuda, chunk)
    m.train()
    u_all, i_all = m.encoder.tables()
    assert u_all.is_contiguous() and i_all.is_contiguous() and u_all.shape[0] == n_users
    assert u_all.data_ptr() + u_all.numel() * 4 == i_all.data_ptr()     # two halves of one buffer
    assert_close(u_all.detach().cpu().numpy(), g["fwd_U"], what=case + " fwd U")
    assert_close(i_all.detach().cpu().numpy(), g["fwd_I"], what=case + " fwd I")
    out = m(_feed(g["uid"], g["iid"], cuda))
    loss = m.loss(out)
    loss.backward()
    assert_close(out["prediction"].detach().cpu().numpy(), g["pred"], what=case + " pred")
    assert_close(loss.item(), g["loss"], what=case + " loss")
    e = m.encoder.embedding_dict
    assert_close(e["user_emb"].grad.cpu().numpy(), g["GU"], what=case + " GU")
    assert_close(e["item_emb"].grad.cpu().numpy(), g["GI"], what=case + " GI")

    m2 = _model(g, cuda, chunk)
    m2.optimizer = _runner(opt, lr, l2)._build_optimizer(m2)
    m2.train()
    extra = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
    prev = (g["U0"], g["I0"])
    losses = []
    for step, (u, i) in enumerate(((g["uid"], g["iid"]), (g["uid2"], g["iid2"])), 1):
        losses.append(float(_step(m2, _feed(u, i, cuda)).item()))
        U, I = _tables(m2)
        assert_update_close(U, prev[0], g["U%d" % step], what=f"{case} U step {step}", extra_atol=extra, outlier_atol=lr)
        assert_update_close(I, prev[1], g["I%d" % step], what=f"{case} I step {step}", extra_atol=extra, outlier_atol=lr)
        prev = (g["U%d" % step], g["I%d" % step])
        with torch.no_grad():     # continue from the reference's tables, so that step 2 checks one step, not two compounded
            m2.encoder.embedding_dict["user_emb"].copy_(torch.from_numpy(prev[0]))
            m2.encoder.embedding_dict["item_emb"].copy_(torch.from_numpy(prev[1]))
    assert_close(np.array(losses), g["losses"], what=case + " losses")

    m2.eval()
    with torch.no_grad():
        ep = m2({"user_id": torch.from_numpy(g["eval_uid"]).to(cuda), "item_id": torch.from_numpy(g["eval_iid"]).to(cuda),
                 "batch_size": len(g["eval_uid"]), "phase": "test"})["prediction"]
    assert_close(ep.cpu().numpy(), g["eval_pred"], what=case + " eval pred")
    return m


@pytest.mark.parametrize("case", CASES)
def test_golden_case(case, cuda):
    _check_case(case, cuda)


@pytest.mark.parametrize("case", CASES)
def test_forced_chunk_splitting_and_run_to_run_bits(case, cuda):
    """chunk length 7 splits the hub and every row past 7 edges into chunks (combine pass); the results stay the reference's,
    and two runs give the same bits"""
    _check_case(case, cuda, chunk=7)
    g = load_golden(case)
    m = _model(g, cuda, chunk=7)
    assert m.encoder.n_parts > 0
    runs = []
    for _ in range(2):
        m.zero_grad()
        out = m(_feed(g["uid"], g["iid"], cuda))
        m.loss(out).backward()
        u_all, i_all = m.encoder.tables()
        e = m.encoder.embedding_dict
        runs.append([t.detach().cpu().numpy().copy() for t in (u_all, i_all, e["user_emb"].grad, e["item_emb"].grad)])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _propagate_both(n_users, n_items, u, i, d, L, cuda, chunk=None, seed=0):
    """(graph, E_0, G, HIP forward, HIP backward, float64 forward, float64 backward) on the graph of the interactions (u, i)"""
    import scipy.sparse as sp
    from rechorus_amd import engine, lgcn
    indptr, indices, data = lgcn.build_norm_adj(n_users, n_items, (u, i))
    graph = lgcn.LgcnGraph.build(n_users, n_items, indptr, indices, data, cuda, chunk=chunk)
    rng = np.random.default_rng(seed)
    N = n_users + n_items
    E = rng.normal(0, 0.1, (N, d)).astype(np.float32)
    G = rng.normal(0, 0.1, (N, d)).astype(np.float32)
    Et, Gt = torch.from_numpy(E).to(cuda), torch.from_numpy(G).to(cuda)
    fwd = engine.lgcn_propagate_fwd(graph, Et[:n_users].contiguous(), Et[n_users:].contiguous(), L).cpu().numpy()
    gu, gi = engine.lgcn_propagate_bwd(graph, Gt[:n_users].contiguous(), Gt[n_users:].contiguous(), L)
    bwd = torch.cat([gu, gi]).cpu().numpy()
    A = sp.csr_matrix((data.astype(np.float64), indices, indptr), shape=(N, N))
    acc, e = E.astype(np.float64), E.astype(np.float64)
    for _ in range(L):
        e = A @ e
        acc = acc + e
    h = G.astype(np.float64) / (L + 1)
    for _ in range(L):
        h = A @ h + G.astype(np.float64) / (L + 1)
    return graph, fwd, bwd, acc / (L + 1), h


def test_skewed_graph_with_a_20k_hub(cuda):
    """one item of degree 25,000, one user of degree 3,000, thousands of isolated rows: default plan and forced splitting"""
    rng = np.random.default_rng(5)
    n_users, n_items = 30000, 6000
    u = [rng.integers(1, 20000, 40000), rng.choice(np.arange(1, n_users), 25000, replace=False), np.full(3000, 7)]
    i = [rng.zipf(1.3, 40000) % 4000 + 1, np.full(25000, 3), rng.choice(np.arange(1, 5000), 3000, replace=False)]
    u, i = np.concatenate(u), np.concatenate(i)
    for chunk, d, L in ((None, 64, 3), (100, 32, 2), (None, 256, 1), (None, 4, 8), (64, 48, 0)):
        graph, fwd, bwd, fwd64, bwd64 = _propagate_both(n_users, n_items, u, i, d, L, cuda, chunk)
        assert int(np.diff(graph.tensors["indptr"].cpu().numpy()).max()) >= 20000
        assert_close(fwd, fwd64, what=f"skewed fwd d{d} L{L} chunk {chunk}")
        assert_close(bwd, bwd64, what=f"skewed bwd d{d} L{L} chunk {chunk}")


def test_amazon_book_shape_against_float64(cuda):
    n_users, n_items, n_inter = 52643, 91599, 2984108
    rng = np.random.default_rng(9)
    u = rng.integers(0, n_users, int(n_inter * 2.2))
    i = (rng.zipf(1.2, u.size) - 1) % n_items
    key = np.unique(u * n_items + i)
    assert key.size >= n_inter
    key = np.sort(rng.choice(key, n_inter, replace=False))
    _, fwd, bwd, fwd64, bwd64 = _propagate_both(n_users, n_items, key // n_items, key % n_items, 64, 3, cuda)
    assert_close(fwd, fwd64, what="amazon-book fwd")
    assert_close(bwd, bwd64, what="amazon-book bwd")


def test_hipgraph_replay_is_bit_equal_to_eager(cuda):
    from rechorus_amd import graph as hgraph
    if not hgraph.usable():
        pytest.fail("hipGraph replay is disabled in this process")
    g = load_golden(CASES[0])
    rng = np.random.default_rng(3)
    batches = [(g["uid"], g["iid"])] + [(rng.integers(1, int(g["meta"][0]), 64), rng.integers(1, int(g["meta"][1]), (64, 2)))
                                        for _ in range(4)]
    results = []
    for replay in (False, True):
        m = _model(g, cuda)
        m.optimizer = _runner("Adam", 1e-3, 1e-8, graph=1)._build_optimizer(m)
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


def test_eval_cache(cuda, tmp_path):
    from rechorus_amd import engine
    g = load_golden(CASES[0])
    m = _model(g, cuda)
    m.optimizer = _runner("Adam", 1e-3, 1e-8)._build_optimizer(m)
    feed = {"user_id": torch.from_numpy(g["eval_uid"]).to(cuda), "item_id": torch.from_numpy(g["eval_iid"]).to(cuda),
            "batch_size": len(g["eval_uid"]), "phase": "test"}

    def recompute():
        e = m.encoder.embedding_dict
        out = engine.lgcn_propagate_fwd(m.encoder.graph(), e["user_emb"].detach(), e["item_emb"].detach(), m.encoder.n_layers)
        U, I = out[:m.user_num], out[m.user_num:]
        return (U[feed["user_id"]][:, None, :] * I[feed["item_id"]]).sum(-1)

    def predict():
        with torch.no_grad():
            return m(feed)["prediction"]

    m.eval()
    p1 = predict()
    cached = m.encoder._eval_tables
    p2 = predict()
    assert m.encoder._eval_tables is cached                      # the second batch reused the tables
    assert torch.equal(p1, p2)
    assert_close(p1.cpu().numpy(), recompute().cpu().numpy(), what="cache vs recomputation")
    m.save_model(str(tmp_path / "m.pt"))
    # a training step invalidates it
    m.train()
    _step(m, _feed(g["uid"], g["iid"], cuda))
    m.eval()
    p3 = predict()
    assert not torch.equal(p3, p1)
    assert_close(p3.cpu().numpy(), recompute().cpu().numpy(), what="after a step")
    # load_model invalidates it
    m.load_model(str(tmp_path / "m.pt"))
    assert m.encoder._eval_tables is None
    assert torch.equal(predict(), p1)
    # the checkpoint holds the reference's keys only
    assert sorted(torch.load(str(tmp_path / "m.pt")).keys()) == sorted(g["state_keys"].tolist())


def test_test_all_ranks_equal_a_numpy_ranking(cuda):
    """--test_all through full_catalogue_vectors + rc_full_catalogue_rank vs the reference's ranking restated in numpy
    (oracle/sampler_oracle.py: target + every item, clicked columns -inf, rank = #scores >= the target's) on the propagated tables"""
    from oracle import sampler_oracle as S
    from rechorus_amd import engine
    g = load_golden("lightgcn_d64_l3_k1_adam")
    m = _model(g, cuda)
    m.eval()
    n_users = int(g["meta"][0])
    sets = {u: set() for u in range(n_users)}
    sets.update(_clicked(g))
    users, targets = g["eval_uid"], g["eval_iid"][:, 0]
    for u, t in zip(users, targets):
        sets[int(u)].add(int(t))          # the dev / test target sits in the residual clicked set
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
        U, I = (t.cpu().numpy() for t in m.encoder.tables())
    want = S.full_catalogue_rank(U[users], I, users, targets, sets)
    s64 = U[users].astype(np.float64) @ I.astype(np.float64).T
    t64 = s64[np.arange(len(users)), targets]
    near = (np.abs(s64 - t64[:, None]) <= 1e-5 * (1 + np.abs(t64[:, None]))).sum(axis=1) - 1   # fp32 vs fp64 near-ties
    diff = np.abs(rank.cpu().numpy().astype(np.int64) - want)
    assert (diff <= near).all(), (rank.cpu().numpy(), want)
    assert want.max() > 1


@pytest.fixture(scope="module")
def synth_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("lgcn_data"))
    make_dataset(root, "synth", n_users=300, n_items=250, per_user=14, seed=4)
    make_impression_dataset(root, "imp", n_users=200, n_items=100, n_imp=12, seed=2)
    return root


@pytest.mark.parametrize("test_all", ["0", "1"])
def test_cli_trains_one_epoch(test_all, synth_root, tmp_path, cuda):
    import main
    log = str(tmp_path / "log" / "run.txt")
    res = main.run(["--model_name", "LightGCN", "--emb_size", "64", "--n_layers", "3", "--lr", "1e-3", "--l2", "1e-8",
                    "--dataset", "synth", "--path", synth_root + "/", "--epoch", "1", "--batch_size", "256", "--num_workers", "0",
                    "--regenerate", "1", "--test_all", test_all, "--log_file", log, "--model_path", str(tmp_path / "m.pt"),
                    "--topk", "5,10", "--save_final_results", "0"])
    text = open(log).read()
    assert re.search(r"Epoch 1\s+loss=[0-9.]+", text), text[-2000:]
    hr = float(re.search(r"HR@5:([0-9.]+)", res["test"]).group(1))
    assert 0.0 <= hr <= 1.0 and "NDCG@10" in res["test"]


def test_cli_impression_variant(synth_root, tmp_path, cuda):
    import main
    log = str(tmp_path / "log" / "run.txt")
    res = main.run(["--model_name", "LightGCN", "--model_mode", "Impression", "--emb_size", "32", "--n_layers", "2", "--lr", "5e-3",
                    "--l2", "0", "--loss_n", "BPR", "--dataset", "imp", "--path", synth_root + "/", "--epoch", "2",
                    "--batch_size", "128", "--num_workers", "0", "--regenerate", "1", "--metric", "NDCG,HR", "--topk", "1,2,3",
                    "--main_metric", "NDCG@2", "--log_file", log, "--model_path", str(tmp_path / "m.pt"), "--save_final_results", "0"])
    assert "NDCG@2" in res["test"]


def test_impression_forward_returns_u_v_and_i_v(cuda):
    g = load_golden(CASES[1])
    m = _model(g, cuda, impression=True)
    m.eval()
    feed = _feed(g["uid"], g["iid"], cuda)
    with torch.no_grad():
        out = m(feed)
        U, I = m.encoder.tables()
    B, C = g["iid"].shape
    assert out["u_v"].shape == (B, C, U.shape[1]) and out["i_v"].shape == (B, C, U.shape[1])
    assert torch.equal(out["u_v"][:, 3], U[feed["user_id"]]) and torch.equal(out["i_v"], I[feed["item_id"]])
    assert_close(out["prediction"].cpu().numpy(), g["pred"], what="impression pred")
