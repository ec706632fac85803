"""GPU: the plugin surface end to end -- HipEmbedding autograd, BaseRunner-style training loop in
dense (exact reference semantics) and row-wise mode, and the CLI driver on a synthetic dataset."""
import argparse
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close, assert_update_close, load_golden
from synth_data import make_dataset

pytestmark = pytest.mark.gpu

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)


def test_hip_embedding_forward_backward(cuda):
    from rechorus_amd.nn import HipEmbedding
    rng = np.random.default_rng(0)
    for n_rows, d, shape in ((50, 64, (7, 5)), (9, 48, (33,)), (300, 128, (4, 3, 2))):
        emb = HipEmbedding(n_rows, d).to(cuda)
        W = emb.weight.detach().cpu().numpy()
        ids = rng.integers(0, n_rows, size=shape).astype(np.int64)
        out = emb(torch.from_numpy(ids).to(cuda))
        assert out.shape == shape + (d,)
        assert np.array_equal(out.detach().cpu().numpy(), W[ids])
        coef = rng.normal(size=shape + (d,)).astype(np.float32)
        (out * torch.from_numpy(coef).to(cuda)).sum().backward()
        want = np.zeros((n_rows, d), dtype=np.float64)
        np.add.at(want, ids.reshape(-1), coef.reshape(-1, d).astype(np.float64))
        assert_close(emb.weight.grad.cpu().numpy(), want, what="dense grad")
    assert "weight" in dict(emb.named_parameters())  # state_dict key as nn.Embedding


def _bprmf(cuda, n_users, n_items, d, K):
    from models.general.BPRMF import BPRMF
    args = argparse.Namespace(device=cuda, model_path="", buffer=1, num_neg=K, dropout=0, test_all=0, emb_size=d)
    corpus = argparse.Namespace(n_users=n_users, n_items=n_items)
    return BPRMF(args, corpus).to(cuda)


def _runner(opt, lr, l2, engine="dense"):
    from helpers.BaseRunner import BaseRunner
    p = BaseRunner.parse_runner_args(argparse.ArgumentParser())
    a = p.parse_args([])
    a.train, a.log_file = 1, "/tmp/rechorus_amd_test/log.txt"
    a.optimizer, a.lr, a.l2, a.engine = opt, lr, l2, engine
    return BaseRunner(a)


@pytest.mark.parametrize("case", ["bprmf_k1_d64", "bprmf_k99_d64_zipf", "bprmf_k5_d48"])
@pytest.mark.parametrize("tag,opt", [("SGD_l20.001", "SGD"), ("Adam_l20.0001", "Adam"), ("Adagrad_l20.0001", "Adagrad")])
def test_model_loss_backward_optimizer_matches_reference_fit(case, tag, opt, cuda):
    """the reference's call order model(batch) -> model.loss -> backward -> optimizer.step through
    the plugin classes (autograd Functions + HipOptimizer) vs the reference's own fit() results"""
    g = load_golden(case)
    lr, l2 = (float(x) for x in g[tag + "_hyper"])
    n_users, n_items, d = g["U0"].shape[0], g["I0"].shape[0], g["U0"].shape[1]
    model = _bprmf(cuda, n_users, n_items, d, g["iid"].shape[1] - 1)
    sd = model.state_dict()
    assert set(sd) == {"u_embeddings.weight", "i_embeddings.weight"}  # reference checkpoint keys
    model.load_state_dict({"u_embeddings.weight": torch.from_numpy(g["U0"]),
                           "i_embeddings.weight": torch.from_numpy(g["I0"])})
    runner = _runner(opt, lr, l2)
    model.optimizer = runner._build_optimizer(model)
    for step, (u, i) in enumerate(((g["uid"], g["iid"]), (g["uid2"], g["iid2"])), 1):
        batch = {"user_id": torch.from_numpy(u).to(cuda), "item_id": torch.from_numpy(i).to(cuda),
                 "batch_size": len(u), "phase": "train"}
        model.optimizer.zero_grad()
        out = model(batch)
        if step == 1:
            assert_close(out["prediction"].detach().cpu().numpy(), g["pred"], what="prediction")
        loss = model.loss(out)
        loss.backward()
        if step == 1:
            assert_close(model.u_embeddings.weight.grad.cpu().numpy(), g["GU"], what="GU")
            assert_close(model.i_embeddings.weight.grad.cpu().numpy(), g["GI"], what="GI")
        model.optimizer.step()
        assert_close(loss.item(), g[tag + "_losses"][step - 1], what=f"loss {step}")
    ex = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
    assert_update_close(model.u_embeddings.weight.detach().cpu().numpy(), g["U0"], g[tag + "_U2"], what="dU", extra_atol=ex)
    assert_update_close(model.i_embeddings.weight.detach().cpu().numpy(), g["I0"], g[tag + "_I2"], what="dI", extra_atol=ex)


@pytest.fixture(scope="module")
def dataset_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("data"))
    make_dataset(root, "synth", n_users=400, n_items=300, per_user=14, seed=1)
    return root


# (plain SGD on a batch-mean loss with 0.01-scale init needs a large step: |grad| ~ 1e-5 per element)
@pytest.mark.parametrize("engine,opt,lr", [("dense", "Adam", "5e-3"), ("rowwise", "SGD", "40"), ("rowwise", "Adam", "5e-3")])
def test_cli_trains_and_reports_like_the_reference(engine, opt, lr, dataset_root, tmp_path, cuda):
    import main
    log = str(tmp_path / "log" / "run.txt")
    res = main.run(["--model_name", "BPRMF", "--emb_size", "32", "--lr", lr, "--l2", "0", "--dataset", "synth",
                    "--path", dataset_root + "/", "--epoch", "6", "--num_neg", "4", "--batch_size", "128",
                    "--num_workers", "0", "--optimizer", opt, "--engine", engine, "--regenerate", "1",
                    "--log_file", log, "--model_path", str(tmp_path / "model" / "m.pt"), "--topk", "5,10",
                    "--save_final_results", "1"])
    text = open(log).read()
    before = float(re.search(r"Test Before Training: \(HR@5:([0-9.]+)", text).group(1))
    losses = [float(x) for x in re.findall(r"Epoch \d+\s+loss=([0-9.]+)", text)]
    assert len(losses) >= 2 and losses[-1] < losses[0], losses
    assert "Best Iter(dev)=" in text and "Test After Training: (HR@5:" in text
    after = float(re.search(r"HR@5:([0-9.]+)", res["test"]).group(1))
    assert 0.0 <= before <= 1.0 and after > before, (before, after)
    assert os.path.exists(str(tmp_path / "model" / "m.pt"))
    rec = tmp_path / "log" / "run" / "rec-BPRMF-test.csv"
    assert rec.exists() and len(open(rec).read().splitlines()) == 401


def test_sharded_engine_single_rank_on_hip(cuda):
    """ShardedBprmf's local ops on the HIP engine (W = 1: no collectives) vs the oracle; the
    routing itself is covered by the gloo tests (tests/test_sharded_gloo.py)"""
    from oracle import bprmf_oracle as O
    from rechorus_amd.sharded import ShardedBprmf
    rng = np.random.default_rng(11)
    n_users, n_items, d, B, C = 57, 300, 64, 64, 20
    U = rng.normal(0, 0.05, (n_users, d)).astype(np.float32)
    I = rng.normal(0, 0.05, (n_items, d)).astype(np.float32)
    for opt, lr, l2 in (("SGD", 0.1, 1e-3), ("Adam", 1e-2, 0.0)):
        m = ShardedBprmf(n_users, n_items, d, opt=opt, lr=lr, l2=l2, device=cuda)
        m.load_global(torch.from_numpy(U).to(cuda), torch.from_numpy(I).to(cuda))
        Un, In = U.copy(), I.copy()
        sU, sI = O.new_state(Un, opt), O.new_state(In, opt)
        for step in (1, 2):
            uid = rng.integers(0, n_users, size=B).astype(np.int64)
            iid = rng.integers(0, n_items, size=(B, C)).astype(np.int64)
            loss = float(m.step(torch.from_numpy(uid).to(cuda), torch.from_numpy(iid).to(cuda)))
            want, _ = O.bprmf_train_step(Un, In, sU, sI, uid, iid, opt=opt, lr=lr, l2=l2, step=step, rowwise=True)
            assert_close(loss, want, what=f"{opt} loss {step}")
        Ug, Ig = m.gather_global()
        ex = 1e-3 * lr if opt == "Adam" else 0.0
        assert_update_close(Ug.cpu().numpy(), U, Un, what="dU", extra_atol=ex)
        assert_update_close(Ig.cpu().numpy(), I, In, what="dI", extra_atol=ex)


# ---- NeuMF / SASRec model files of the mirror: reference checkpoints load, same outputs -----------

def _load_state(model, g, cuda):
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("P0/")}
    assert set(sd) == set(model.state_dict()), "state_dict keys differ from the reference's"
    model.load_state_dict(sd)
    return model.to(cuda)


@pytest.mark.parametrize("case", ["neumf_d64_l64_k4", "neumf_d128_l64_k4", "neumf_d32_l32_k9",
                                  "neumfml_d32_l64x32_k4", "neumfml_d64_l128x64x32_k9"])  # ml: --layers with several entries
def test_neumf_model_file_matches_reference(case, cuda):
    from models.general.NeuMF import NeuMF
    g = load_golden(case)
    n_users, n_items, d = g["P0/mf_u_embeddings.weight"].shape[0], g["P0/mf_i_embeddings.weight"].shape[0], int(g["meta"][2])
    layers = [int(x) for x in g["meta"][6:]]
    args = argparse.Namespace(device=cuda, model_path="", buffer=1, num_neg=4, dropout=0, test_all=0, emb_size=d,
                              layers=str(layers))
    model = _load_state(NeuMF(args, argparse.Namespace(n_users=n_users, n_items=n_items)), g, cuda)
    batch = {"user_id": torch.from_numpy(g["uid"]).to(cuda), "item_id": torch.from_numpy(g["iid"]).to(cuda),
             "batch_size": len(g["uid"]), "phase": "train"}
    out = model(batch)
    assert_close(out["prediction"].detach().cpu().numpy(), g["pred"], what="prediction")
    loss = model.loss(out)
    loss.backward()
    assert_close(loss.item(), g["loss"], what="loss")
    for name, p in model.named_parameters():
        assert_close(p.grad.cpu().numpy(), g["G/" + name], what="grad " + name, atol_scale=2e-5)


@pytest.mark.parametrize("case", ["neumfdrop_d64_l64_k4_p0.2", "neumfdrop_d32_l128_k9_p0.5"])
def test_neumf_model_file_trains_with_dropout_in_the_kernels(case, cuda):
    """--dropout p: train mode runs rc_neumf_fwd / rc_neumf_bwd with drop_p > 0 (no torch layers); with the
    model's mask seed set to the golden's, prediction and autograd gradients equal the reference's run with
    that mask; eval mode is the plain head"""
    from models.general.NeuMF import NeuMF
    from rechorus_amd import nn as hnn
    g = load_golden(case)
    n_users, n_items, d, l1 = (g["P0/mf_u_embeddings.weight"].shape[0], g["P0/mf_i_embeddings.weight"].shape[0],
                               int(g["meta"][2]), int(g["meta"][6]))
    args = argparse.Namespace(device=cuda, model_path="", buffer=1, num_neg=4, dropout=float(g["p"]), test_all=0, emb_size=d,
                              layers=str([l1]))
    model = NeuMF(args, argparse.Namespace(n_users=n_users, n_items=n_items))
    assert "drop_seed" not in model.state_dict()  # checkpoints keep the reference's keys
    model = _load_state(model, g, cuda)
    batch = {"user_id": torch.from_numpy(g["uid"]).to(cuda), "item_id": torch.from_numpy(g["iid"]).to(cuda),
             "batch_size": len(g["uid"]), "phase": "train"}
    model.train()
    calls = []
    real = hnn.engine.neumf_fwd
    hnn.engine.neumf_fwd = lambda *a, **k: calls.append(a[3:]) or real(*a, **k)
    try:
        model.drop_seed.fill_(int(g["mask_seed"]) - 1)  # forward() bumps it once
        out = model(batch)
    finally:
        hnn.engine.neumf_fwd = real
    assert calls and calls[0][0] == pytest.approx(float(g["p"]))
    assert_close(out["prediction"].detach().cpu().numpy(), g["pred"], what="prediction")
    loss = model.loss(out)
    loss.backward()
    assert_close(loss.item(), g["loss"], what="loss")
    for name, p in model.named_parameters():
        assert_close(p.grad.cpu().numpy(), g["G/" + name], what="grad " + name, atol_scale=2e-5)
    again = model(batch)["prediction"].detach()
    assert not torch.equal(again, out["prediction"].detach())  # next forward, next mask
    model.eval()
    e1, e2 = model(batch)["prediction"].detach(), model(batch)["prediction"].detach()
    assert torch.equal(e1, e2)
    want_eval, _ = __import__("oracle.neumf_oracle", fromlist=["x"]).forward({k[3:]: v for k, v in g.items() if k.startswith("P0/")},
                                                                          g["uid"], g["iid"])
    assert_close(e1.cpu().numpy(), want_eval, what="eval prediction")


@pytest.mark.parametrize("case", ["sasrec_d64_l1_h1", "sasrec_d64_l1_h4_L50", "sasrec_d64_l2_h2", "sasrec_d32_l1_h4", "sasrec_d64_l1_h2_L100"])
def test_sasrec_model_file_matches_reference(case, cuda):
    from models.sequential.SASRec import SASRec
    g = load_golden(case)
    n_items, d, n_layers, n_heads, hist_max = (int(x) for x in g["meta"][:5])
    args = argparse.Namespace(device=cuda, model_path="", buffer=1, num_neg=4, dropout=0, test_all=0, emb_size=d,
                              num_layers=n_layers, num_heads=n_heads, history_max=hist_max)
    model = _load_state(SASRec(args, argparse.Namespace(n_users=10, n_items=n_items)), g, cuda)
    batch = {"history_items": torch.from_numpy(g["hist"]).to(cuda), "lengths": torch.from_numpy(g["len"]).to(cuda),
             "item_id": torch.from_numpy(g["iid"]).to(cuda), "user_id": torch.zeros(len(g["len"]), dtype=torch.long, device=cuda),
             "batch_size": len(g["len"]), "phase": "train"}
    out = model(batch)
    assert_close(out["prediction"].detach().cpu().numpy(), g["pred"], what="prediction", atol_scale=2e-5)
    loss = model.loss(out)
    loss.backward()
    assert_close(loss.item(), g["loss"], what="loss", rtol=2e-5)
    G = {k[2:]: v for k, v in g.items() if k.startswith("G/")}
    floor = 1e-6 * max(float(np.abs(v).max()) for v in G.values())
    for name, p in model.named_parameters():
        assert_close(p.grad.cpu().numpy(), G[name], what="grad " + name, rtol=2e-5, atol_scale=5e-5, abs_floor=floor)
    # the torch fall-back of the same module (what unsupported shapes use) agrees with the HIP encoder
    hv_hip = model.forward(batch)["prediction"].detach()
    hv_torch = model._encode_torch(batch["history_items"], batch["lengths"]).detach()
    pred_torch = (hv_torch[:, None, :] * model.i_embeddings.weight.detach()[batch["item_id"]]).sum(-1)
    assert_close(hv_hip.cpu().numpy(), pred_torch.cpu().numpy(), what="hip vs torch encoder", rtol=1e-4, atol_scale=1e-4)


@pytest.mark.parametrize("model_args", [
    ["--model_name", "NeuMF", "--emb_size", "32", "--layers", "[32]", "--lr", "5e-3"],
    ["--model_name", "SASRec", "--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--history_max", "10", "--lr", "3e-3"],
    ["--model_name", "NeuMF", "--emb_size", "32", "--layers", "[32]", "--lr", "5e-3", "--engine", "rowwise"],
    ["--model_name", "NeuMF", "--emb_size", "32", "--layers", "[32]", "--lr", "5e-3", "--dropout", "0.2"],
    ["--model_name", "NeuMF", "--emb_size", "32", "--layers", "[32]", "--lr", "5e-3", "--dropout", "0.2", "--engine", "rowwise"],
    ["--model_name", "SASRec", "--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--history_max", "10", "--lr", "3e-3",
     "--engine", "rowwise"],
    ["--model_name", "SASRec", "--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--history_max", "10", "--lr", "3e-3",
     "--dropout", "0.2"],
    ["--model_name", "SASRec", "--emb_size", "32", "--num_layers", "2", "--num_heads", "2", "--history_max", "10", "--lr", "3e-3",
     "--dropout", "0.2", "--engine", "rowwise"],
    # outside the register-resident encoders' envelope: the shape-generic layers (csrc/seq_layers.hip), dense updates, hipGraph replay
    ["--model_name", "SASRec", "--emb_size", "128", "--num_layers", "2", "--num_heads", "8", "--history_max", "10", "--lr", "2e-3",
     "--dropout", "0.2"],
    ["--model_name", "SASRec", "--emb_size", "48", "--num_layers", "5", "--num_heads", "3", "--history_max", "10", "--lr", "2e-3"],
])
def test_cli_neumf_and_sasrec(model_args, dataset_root, tmp_path, cuda):
    import main
    log = str(tmp_path / "log" / "run.txt")
    res = main.run(model_args + ["--l2", "1e-6", "--dataset", "synth", "--path", dataset_root + "/", "--epoch", "5",
                                 "--num_neg", "4", "--batch_size", "128", "--num_workers", "0", "--regenerate", "1",
                                 "--log_file", log, "--model_path", str(tmp_path / "model" / "m.pt"), "--topk", "5,10",
                                 "--save_final_results", "0"])
    text = open(log).read()
    losses = [float(x) for x in re.findall(r"Epoch \d+\s+loss=([0-9.]+)", text)]
    assert len(losses) >= 2 and losses[-1] < losses[0], losses
    before = float(re.search(r"Test Before Training: \(HR@5:([0-9.]+)", text).group(1))
    after = float(re.search(r"HR@5:([0-9.]+)", res["test"]).group(1))
    assert after > before, (before, after)


@pytest.mark.parametrize("tag,lr,l2", [("lr1_l20.0001", 1.0, 1e-4), ("lr0.001_l20", 1e-3, 0.0)])
def test_adadelta_through_the_plugin_matches_the_reference(tag, lr, l2, cuda):
    """--optimizer Adadelta (helpers/BaseRunner.py:37-38): model(batch) -> loss -> backward -> HipOptimizer.step on the
    engine (rc_dense_update_multi, MODE_ADADELTA) vs three fit() iterations of the reference itself"""
    from rechorus_amd import nn as hnn
    g = np.load(os.path.join(ROOT, "tests", "golden", "adadelta_bprmf_d64.npz"))
    n_users, n_items, d = g["U0"].shape[0], g["I0"].shape[0], g["U0"].shape[1]
    model = _bprmf(cuda, n_users, n_items, d, g["iid1"].shape[1] - 1)
    model.load_state_dict({"u_embeddings.weight": torch.from_numpy(g["U0"]), "i_embeddings.weight": torch.from_numpy(g["I0"])})
    runner = _runner("Adadelta", lr, l2)
    model.optimizer = runner._build_optimizer(model)
    assert isinstance(model.optimizer, hnn.HipOptimizer)
    for step in (1, 2, 3):
        u, i = g[f"uid{step}"], g[f"iid{step}"]
        batch = {"user_id": torch.from_numpy(u).to(cuda), "item_id": torch.from_numpy(i).to(cuda), "batch_size": len(u), "phase": "train"}
        model.optimizer.zero_grad()
        loss = model.loss(model(batch))
        loss.backward()
        model.optimizer.step()
        assert_close(float(loss), float(g[tag + "_losses"][step - 1]), what=f"loss {step}")
        assert_update_close(model.u_embeddings.weight.detach().cpu().numpy(), g["U0"], g[f"{tag}_U{step}"], what=f"dU {step}",
                            extra_atol=1e-6 * lr)
        assert_update_close(model.i_embeddings.weight.detach().cpu().numpy(), g["I0"], g[f"{tag}_I{step}"], what=f"dI {step}",
                            extra_atol=1e-6 * lr)
