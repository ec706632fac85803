"""GPU: ComiRec on the HIP engine (rc_comirec_fwd / _bwd / _score_max) against the reference's goldens
(tests/golden/make_golden_comirec.py) and the float64 restatement (tests/comirec_np.py): interests, selection, training
prediction, loss, every parameter gradient, two fit() iterations, evaluation predictions; kernel-level forward, selection and
backward at the envelope's corners and at sizes off every tile; the evaluation head at 1, 100 and n_items - 1 candidates;
bit-identical reruns, the refusal outside the envelope and the CLI on both data paths and under --test_all.

Tolerances: 2e-5 of the tensor's largest entry.  Exceptions, each for a named reason (comirec_np.grad_floor): the gradient of
W2's bias is exactly 0 in exact arithmetic and round-off in every implementation (floor: 1e-5 of W2's largest weight gradient);
the attention-path gradients are exact zeros in the reference at L = 1 (floor: 1e-6 of the batch's largest gradient entry);
under Adam and Adagrad the step of W2's bias is that round-off normalised to +-lr, so it is bounded by lr, not compared.
The hard selection is compared on every golden row with two or more valid positions (the generator asserted a top-2 gap of
1e-3 there); at kernel level on every row whose float64 gap is at least 1e-4 of the largest |target_pred|, and the rows under
it may be at most 3 % of the rows with two or more positions.  The backward is compared on ALL rows with the kernel's own
selection imposed on the oracle.  Each comparison prints the largest error it saw (run with -s)."""
import argparse
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_update_close, golden_cases, load_golden
from synth_data import make_dataset

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import comirec_np  # noqa: E402
from comirec_np import PARAM_KEYS, TOL, golden_grads, golden_params, grad_floor, rel_err  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

pytestmark = pytest.mark.gpu
CASES = golden_cases("comirec_")
ATTR = {"I": "i_embeddings.weight", "Pos": "p_embeddings.weight", "W1": "W1.weight", "b1": "W1.bias", "W2": "W2.weight",
        "b2": "W2.bias"}


def _check(got, want, what, floor=0.0, tol=TOL):
    if torch.is_tensor(got):
        got = got.detach().cpu().numpy()
    err = rel_err(got, want, floor)
    print(f"COMIREC_TOL {what}: {err:.3e} (allowed {tol:g})")
    assert err <= tol, f"{what}: largest error / largest entry {err:.3e} > {tol:g}"
    return err


def _model(g, dev, prefix="P0_"):
    from models.sequential.ComiRec import ComiRec
    n_items, d, A, K, L, B, C, add_pos, seed = (int(x) for x in g["meta"])
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=C - 1, dropout=0, test_all=0, emb_size=d, attn_size=A, K=K,
                           add_pos=add_pos, history_max=L)
    m = ComiRec(args, SimpleNamespace(n_users=50, n_items=n_items)).to(dev)
    _load(m, g, prefix)
    return m


def _load(m, g, prefix):
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(torch.from_numpy(g[prefix + k.replace(".", "__")]))


def _param(m, k):
    obj = m
    for part in ATTR[k].split("."):
        obj = getattr(obj, part, None)
        if obj is None:
            return None
    return obj


def _feed(hist, lengths, iid, dev, phase="train"):
    return {"user_id": torch.zeros(len(lengths), dtype=torch.long, device=dev), "item_id": torch.from_numpy(iid).to(dev),
            "history_items": torch.from_numpy(hist).to(dev), "lengths": torch.from_numpy(lengths).to(dev), "batch_size": len(lengths),
            "phase": phase}


def _runner(opt, lr, l2):
    from helpers.BaseRunner import BaseRunner
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.train, a.log_file = 1, "/tmp/rechorus_amd_test/log.txt"
    a.optimizer, a.lr, a.l2, a.graph, a.engine = opt, lr, l2, 0, "dense"
    return BaseRunner(a)


@pytest.mark.parametrize("case", CASES)
def test_golden_case(case, cuda):
    from rechorus_amd import nn as hnn
    g = load_golden(case)
    lr, l2 = (float(x) for x in g["hyper"])
    opt = str(g["opt"])
    m = _model(g, cuda)
    m.train()
    batch = _feed(g["hist"], g["lengths"], g["item_id"], cuda)
    with torch.no_grad():
        _, interests, sel = hnn.comirec_user_vector(*m._tensors(), batch["history_items"], batch["lengths"],
                                                    batch["item_id"][:, 0].contiguous(), details=True)
    _check(interests, g["interests"], case + " interests")
    valid = (g["hist"] > 0).sum(1)
    multi = valid >= 2
    assert np.array_equal(sel.cpu().numpy()[multi], g["sel"][multi]), case + " sel"
    assert interests[torch.from_numpy(valid == 0).to(cuda)].abs().sum().item() == 0.0      # no valid position: zero interests
    out = m(batch)
    loss = m.loss(out)
    loss.backward()
    _check(out["prediction"], g["pred"], case + " pred")
    assert abs(loss.item() - float(g["loss"])) <= TOL * max(1.0, abs(float(g["loss"]))), (case, loss.item(), float(g["loss"]))
    want = golden_grads(g)
    for k in PARAM_KEYS:
        if want[k] is not None:
            _check(_param(m, k).grad, want[k], f"{case} grad {k}", grad_floor(want, k))

    m2 = _model(g, cuda)
    m2.optimizer = _runner(opt, lr, l2)._build_optimizer(m2)
    m2.train()
    extra = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
    keep = g["keep"]
    batches = ((g["hist"][keep], g["lengths"][keep], g["item_id"][keep]), (g["hist2"], g["lengths2"], g["item_id2"]))
    for step, (h, n, i) in enumerate(batches, 1):
        m2.optimizer.zero_grad()
        ls = m2.loss(m2(_feed(h, n, i, cuda)))
        ls.backward()
        m2.optimizer.step()
        want_ls = float(g["losses"][step - 1])
        assert abs(ls.item() - want_ls) <= TOL * max(1.0, abs(want_ls)), (case, step, ls.item(), want_ls)
        for k, v in m2.state_dict().items():
            key = k.replace(".", "__")
            if k == "W2.bias" and opt in ("Adam", "Adagrad"):
                # its gradient is round-off around an exact 0 (a softmax ignores a shift of its row), in the reference as well, and
                # Adam / Adagrad normalise whatever it is to a step of size lr in either direction: the step can only be bounded
                moved = np.abs(v.detach().cpu().numpy().astype(np.float64) - g["P%d_" % (step - 1) + key])
                assert moved.max() <= lr * 1.001 + 1e-7, (case, step, moved.max(), lr)
                continue
            assert_update_close(v.detach().cpu().numpy(), g["P%d_" % (step - 1) + key], g["P%d_" % step + key],
                                what=f"{case} {k} step {step}", extra_atol=extra, outlier_atol=lr)
        _load(m2, g, "P%d_" % step)     # continue from the reference's parameters: step 2 checks one step, not two compounded
    m2.eval()
    with torch.no_grad():
        ep = m2(_feed(g["eval_hist"], g["eval_lengths"], g["eval_iid"], cuda, phase="test"))["prediction"]
    assert ep.shape == g["eval_pred"].shape
    _check(ep, g["eval_pred"], case + " eval pred")


def _random_problem(B, L, d, A, K, add_pos, seed):
    """parameters at N(0, 0.5), histories of every length in [0, L] with repeated ids, an all-padding row and a zero id between
    two valid ones where the shape has room"""
    rng = np.random.default_rng(seed)
    n_items = 300
    f32 = np.float32
    P = {"I": rng.normal(0, 0.5, (n_items, d)).astype(f32), "Pos": rng.normal(0, 0.5, (L + 1, d)).astype(f32) if add_pos else None,
         "W1": rng.normal(0, 0.5, (A, d)).astype(f32), "b1": rng.normal(0, 0.5, A).astype(f32),
         "W2": rng.normal(0, 0.5, (K, A)).astype(f32), "b2": rng.normal(0, 0.5, K).astype(f32)}
    lengths = rng.integers(1, L + 1, B).astype(np.int64)
    lengths[0] = L
    pz = 1.0 / np.arange(1, n_items)
    pz /= pz.sum()
    hist = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        hist[b, :lengths[b]] = rng.choice(np.arange(1, n_items), size=lengths[b], p=pz)
    if B >= 3:
        hist[B // 2] = 0
    if L >= 3:
        hist[0, 1] = 0
    target = rng.integers(1, n_items, B).astype(np.int64)
    d_user = rng.normal(0, 1.0, (B, d)).astype(f32)
    return P, hist, lengths, target, d_user


SHAPES = [(1, 1, 4, 1, 1, 1), (3, 2, 4, 1, 2, 1), (65, 20, 64, 8, 4, 1), (257, 64, 256, 64, 16, 1), (129, 256, 36, 5, 3, 0),
          (4099, 20, 64, 8, 4, 1)]


@pytest.mark.parametrize("B,L,d,A,K,add_pos", SHAPES)
def test_kernels_against_float64(B, L, d, A, K, add_pos, cuda):
    from rechorus_amd import engine
    P, hist, lengths, target, d_user = _random_problem(B, L, d, A, K, add_pos, seed=B + 7 * L + d)
    dev = {k: (None if v is None else torch.from_numpy(v).to(cuda)) for k, v in P.items()}
    h, n, t = (torch.from_numpy(x).to(cuda) for x in (hist, lengths, target))
    interests, attn, sel, user = engine.comirec_fwd(dev["I"], dev["Pos"], dev["W1"], dev["b1"], dev["W2"], dev["b2"], h, n, targets=t)
    what = f"B={B} L={L} d={d} A={A} K={K}"
    f = comirec_np.forward(P, hist, lengths)
    _check(interests, f["interests"], what + " interests")
    _check(attn, f["a"], what + " attention")
    tp = comirec_np.target_pred(f["interests"], P["I"], target)
    gap = comirec_np.top2_gap(tp)
    multi = (hist > 0).sum(1) >= 2
    clear = gap >= 1e-4 * np.abs(tp).max() if K >= 2 else np.ones(B, dtype=bool)
    sel_np = sel.cpu().numpy().astype(np.int64)
    assert np.array_equal(sel_np[clear], tp.argmax(1)[clear]), what + " sel"
    skipped = int((multi & ~clear).sum())
    print(f"COMIREC_SEL {what}: {skipped} of {int(multi.sum())} rows with >= 2 positions under the gap")
    assert skipped <= 0.03 * max(int(multi.sum()), 1)
    assert ((sel_np >= 0) & (sel_np < K)).all()
    _check(user, f["interests"][np.arange(B), sel_np], what + " user")

    du = torch.from_numpy(d_user).to(cuda)
    got = engine.comirec_bwd(dev["I"], dev["Pos"], dev["W1"], dev["b1"], dev["W2"], h, n, attn, sel, user, du)
    want = comirec_np.backward_user(P, hist, lengths, f, sel_np, d_user.astype(np.float64))
    names = ("g_hist", "g_x", "W1", "b1", "W2", "b2")
    ref = {"I": want[0], "Pos": want[1] if add_pos else None, "W1": want[2], "b1": want[3], "W2": want[4], "b2": want[5]}
    for name, key, a, b in zip(names, ("I", "Pos", "W1", "b1", "W2", "b2"), got, want):
        if name == "g_x" and not add_pos:
            assert a is None
            continue
        _check(a, b, f"{what} {name}", grad_floor(ref, key))
    invalid = torch.from_numpy(hist <= 0).to(cuda)
    assert got[0][invalid].abs().sum().item() == 0.0            # rows at invalid positions are written as zeros
    if add_pos:
        assert got[1][invalid].abs().sum().item() == 0.0
    # only row sel[b] of W2 / b2 receives anything: an interest no sequence selected has an exactly zero row
    unused = np.setdiff1d(np.arange(K), sel_np)
    assert got[4][torch.from_numpy(unused).to(cuda)].abs().sum().item() == 0.0


@pytest.mark.parametrize("C", [1, 100, 999])
@pytest.mark.parametrize("d,K", [(64, 4), (36, 3), (256, 16), (4, 1)])
def test_score_max_against_float64(C, d, K, cuda):
    from rechorus_amd import engine
    rng = np.random.default_rng(C + d)
    n_items, B = 1000, 5
    I = rng.normal(0, 0.5, (n_items, d)).astype(np.float32)
    interests = rng.normal(0, 0.5, (B, K, d)).astype(np.float32)
    if C == n_items - 1:
        iid = np.stack([rng.permutation(np.arange(1, n_items)) for _ in range(B)]).astype(np.int64)     # the whole catalogue
    else:
        iid = rng.integers(0, n_items, (B, C)).astype(np.int64)
    pred = engine.comirec_score_max(torch.from_numpy(interests).to(cuda), torch.from_numpy(I).to(cuda), torch.from_numpy(iid).to(cuda))
    want = np.einsum("bkd,bcd->bck", interests.astype(np.float64), I.astype(np.float64)[iid]).max(-1)
    assert pred.shape == (B, C)
    _check(pred, want, f"score_max C={C} d={d} K={K}")


def test_eval_forward_refuses_autograd_and_model_eval_runs_without_it(cuda):
    from rechorus_amd import nn as hnn
    g = load_golden("comirec_d64_a8_k4_l20_adam_b77")
    m = _model(g, cuda, "P2_")
    batch = _feed(g["eval_hist"], g["eval_lengths"], g["eval_iid"], cuda, phase="test")
    with pytest.raises(RuntimeError, match="no backward"):
        hnn.comirec_scores(*m._tensors(), batch["history_items"], batch["lengths"], batch["item_id"])
    m.eval()
    ep = m(batch)["prediction"]          # the model's evaluation phase needs no torch.no_grad() around it
    assert not ep.requires_grad
    _check(ep, g["eval_pred"], "eval phase of the model file")


def test_reruns_are_bit_identical(cuda):
    from rechorus_amd import engine
    for shape in ((4099, 20, 64, 8, 4, 1), (129, 256, 36, 5, 3, 0), (65, 20, 64, 8, 4, 1)):
        B, L, d, A, K, add_pos = shape
        P, hist, lengths, target, d_user = _random_problem(*shape, seed=11)
        dev = {k: (None if v is None else torch.from_numpy(v).to(cuda)) for k, v in P.items()}
        h, n, t, du = (torch.from_numpy(x).to(cuda) for x in (hist, lengths, target, d_user))
        runs = []
        for _ in range(2):
            interests, attn, sel, user = engine.comirec_fwd(dev["I"], dev["Pos"], dev["W1"], dev["b1"], dev["W2"], dev["b2"], h, n,
                                                            targets=t)
            grads = engine.comirec_bwd(dev["I"], dev["Pos"], dev["W1"], dev["b1"], dev["W2"], h, n, attn, sel, user, du)
            runs.append([x.cpu().numpy().copy() for x in (interests, attn, sel, user) + tuple(x for x in grads if x is not None)])
        for a, b in zip(*runs):
            assert a.tobytes() == b.tobytes(), shape


@pytest.mark.parametrize("flags", [dict(emb_size=6), dict(emb_size=260), dict(K=0), dict(K=17), dict(attn_size=65),
                                   dict(history_max=0), dict(history_max=257)])
def test_shape_outside_the_envelope_raises_from_init(flags, cuda):
    from models.sequential.ComiRec import ComiRec
    a = dict(device=cuda, model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=64, attn_size=8, K=2, add_pos=1,
             history_max=20)
    a.update(flags)
    with pytest.raises(ValueError, match="outside the envelope"):
        ComiRec(SimpleNamespace(**a), SimpleNamespace(n_users=5, n_items=6))


def test_history_longer_than_the_envelope_is_refused_not_rerouted(cuda):
    from rechorus_amd import engine
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=cuda)
    with pytest.raises(ValueError, match="outside the envelope"):
        engine.comirec_fwd(z(9, 64), None, z(8, 64), z(8), z(4, 8), z(4), z(3, 300, dt=torch.int64), z(3, dt=torch.int64))


@pytest.fixture(scope="module")
def synth_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("comirec_data"))
    make_dataset(root, "synth", n_users=300, n_items=250, per_user=14, seed=5)
    return root


@pytest.mark.parametrize("pipeline_flag,test_all", [("1", "0"), ("1", "1"), ("0", "0")])
def test_cli_trains_one_epoch(pipeline_flag, test_all, synth_root, tmp_path, cuda, monkeypatch):
    import main
    from rechorus_amd import graph as hgraph, nn as hnn
    replays, fused = [], []
    run0, fwd0 = hgraph.GraphedStep.run, hnn.comirec_user_vector
    monkeypatch.setattr(hgraph.GraphedStep, "run", lambda self, b: replays.append(1) or run0(self, b))
    monkeypatch.setattr(hnn, "comirec_user_vector", lambda *a, **k: fused.append(1) or fwd0(*a, **k))
    log = str(tmp_path / "log" / "run.txt")
    res = main.run(["--model_name", "ComiRec", "--emb_size", "64", "--attn_size", "8", "--K", "4", "--add_pos", "1",
                    "--history_max", "20", "--lr", "1e-3", "--l2", "1e-6", "--dataset", "synth", "--path", synth_root + "/",
                    "--epoch", "1", "--batch_size", "256", "--num_workers", "0", "--regenerate", "1", "--test_all", test_all,
                    "--device_pipeline", pipeline_flag, "--log_file", log, "--model_path", str(tmp_path / "m.pt"),
                    "--topk", "5,10", "--save_final_results", "0"])
    text = open(log).read()
    m = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", text)
    assert m and np.isfinite(float(m.group(1))), text[-2000:]
    hr = float(re.search(r"HR@5:([0-9.]+)", res["test"]).group(1))
    assert 0.0 <= hr <= 1.0 and "NDCG@10" in res["test"]
    assert fused and not replays      # the fused forward trained; the shuffled dense step runs eagerly, never from a hipGraph
