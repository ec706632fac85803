"""GPU: ContraRec on the HIP engine against the reference's fixtures (tests/golden/make_golden_contrarec.py) and the float64
restatement (tests/contrarec_np.py): the contrastive-loss kernels (rc_contra_loss_fwd / _bwd) at one tile, across the view
boundary, at the first batch that splits the sweep into column chunks and the one before it, at every label mode, with a zero
feature row and bit-identical on a rerun; the forward-indexed position embedding and its table gradient; the model file against
the goldens (prediction, features, the three losses, every gradient, two fit() iterations, evaluation); the CLI.

Tolerance: the project's cap, 2e-5 of the tensor's largest entry (conftest.assert_close with rtol = 0); nothing is excluded.
Exceptions, each for a named reason:
  * B = 1 (N = 2): the reference's loss is ~3e-11 and its gradients ~1e-12, the effect of its 1e-10 guards: |loss| and |grad| are
    bounded by 1e-6 absolutely, not compared relatively.
  * the key biases of the attention (k_linear.bias) have a gradient that is exactly 0 in exact arithmetic -- a softmax ignores a
    shift of its row -- and round-off in every implementation, the reference included: it gets a floor of 1e-6 of the batch's
    largest gradient entry, and under Adam / Adagrad, which normalise whatever it is to a step of size lr in either direction,
    its update over the two iterations is bounded by 2 lr, not compared.
  * a feature row of all zeros has the gradient g / 1e-12: it is compared on its own scale, the other rows on theirs.
Each comparison prints the largest error it saw (run with -s); RC_TOL_REPORT collects them for tools/tolerance_report.py."""
import argparse
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT, assert_close, assert_update_close, golden_cases, load_golden
from synth_data import make_dataset

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import contrarec_np  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

pytestmark = pytest.mark.gpu
CASES = [c for c in golden_cases("contrarec_d") if not c.endswith(("_grads", "_after"))]
F64_FILES = ("contraloss_f64", "contraloss_f64_b1025_d64", "contraloss_f64_b1025_d32")
TOL = 2e-5


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _check(got, want, what, floor=0.0):
    got, want = _np(got).astype(np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-300)
    print(f"CONTRAREC_TOL {what}: {float(np.abs(got - want).max()) / scale:.3e} of the largest entry (allowed {TOL:g})")
    assert_close(got, want, rtol=0.0, atol_scale=TOL, what=what, abs_floor=floor)


def _check_scalar(got, want, what):
    _check(np.array([float(got)]), np.array([float(want)]), what)


# ---- the contrastive-loss kernels ---------------------------------------------------------------------------------------------

def _labels(mode, B, rng):
    if mode == "none":
        return None
    if mode == "distinct":
        return rng.permutation(B).astype(np.int64) + 1
    if mode == "equal":
        return np.full(B, 7, dtype=np.int64)
    pz = 1.0 / np.arange(1, 41)
    return rng.choice(np.arange(1, 41), size=B, p=pz / pz.sum()).astype(np.int64)      # Zipf


def _run_loss(x, labels, t, dev):
    """x [B, 2, d] float32 -> (loss, dva, dvb) of the kernels, through the autograd node"""
    from rechorus_amd import nn as hnn
    va = torch.from_numpy(np.ascontiguousarray(x[:, 0])).to(dev).requires_grad_(True)
    vb = torch.from_numpy(np.ascontiguousarray(x[:, 1])).to(dev).requires_grad_(True)
    lab = None if labels is None else torch.from_numpy(labels).to(dev)
    loss = hnn.contra_loss(va, vb, lab, t)
    loss.backward()
    return loss.item(), va.grad, vb.grad


def _compare_loss(x, labels, t, want, what, dev, zero_row=None):
    loss, dva, dvb = _run_loss(x, labels, t, dev)
    wl, wa, wb = want
    B = x.shape[0]
    if B == 1:      # N = 2: the 1e-10 guards' effect on both sides
        print(f"CONTRAREC_TOL {what}: |loss| {abs(loss):.3e}, |grad| {max(float(dva.abs().max()), float(dvb.abs().max())):.3e} (bound 1e-6)")
        assert abs(loss) <= 1e-6 and abs(wl) <= 1e-6
        assert float(dva.abs().max()) <= 1e-6 and float(dvb.abs().max()) <= 1e-6 and np.abs(wa).max() <= 1e-6 and np.abs(wb).max() <= 1e-6
        return
    _check_scalar(loss, wl, what + " loss")
    got, ref = np.stack([_np(dva), _np(dvb)], 1), np.stack([wa, wb], 1)
    if zero_row is not None:      # its gradient is g / 1e-12: on its own scale
        _check(got[zero_row, 0], ref[zero_row, 0], what + " grad of the zero row")
        got, ref = np.delete(got, zero_row, 0), np.delete(ref, zero_row, 0)
    _check(got, ref, what + " grad")


def _f64_cases():
    out = []
    for f in F64_FILES:
        g = load_golden(f)
        for i in range(int(g["n"])):
            B, d, distinct = (int(v) for v in g["shape_%d" % i])
            out.append(pytest.param(f, i, id=f"B{B}-d{d}-t{float(g['t_%d' % i]):g}-{distinct or 'none'}"))
    return out


@pytest.mark.parametrize("fname,i", _f64_cases())
def test_contra_loss_against_the_float64_fixture(fname, i, cuda):
    g = load_golden(fname)
    B, d, distinct = (int(v) for v in g["shape_%d" % i])
    t = float(g["t_%d" % i])
    labels = g["labels_%d" % i] if distinct else None
    x = (g["x_%d" % i].astype(np.float32) / np.float32(32.0))      # exact in fp32
    grad = g["grad_%d" % i].astype(np.float64)
    _compare_loss(x, labels, t, (float(g["loss_%d" % i]), grad[:, 0], grad[:, 1]), f"fixture B={B} d={d} t={t:g}", cuda)


def _split_batch():
    from rechorus_amd import engine
    return engine.contra_first_split_batch()


def _kernel_cases():
    s = _split_batch()      # the smallest batch whose sweep is split into column chunks (17: N = 34, two column blocks)
    return [
        # B,  d,   t,    labels,     zero row
        (1, 64, 0.2, "equal", False),            # N = 2
        (1, 4, 1.0, "none", False),
        (2, 4, 0.2, "equal", False),             # both labels equal: every other row is a positive
        (16, 64, 0.2, "zipf", False),            # N = 32: exactly one tile
        (17, 64, 0.2, "zipf", False),            # the view boundary inside a tile
        (s, 128, 0.05, "distinct", False),       # the first split ...
        (s - 1, 128, 0.05, "distinct", False),   # ... and the batch before it
        (s, 256, 1.0, "none", False),
        (33, 4, 1.0, "equal", False),
        (33, 64, 0.2, "zipf", True),             # the max(|x|, 1e-12) branch
        (300, 256, 0.05, "zipf", False),
        (300, 64, 0.2, "distinct", False),
        (1025, 128, 0.2, "none", False),
        (1025, 64, 1.0, "equal", False),
    ]


@pytest.mark.parametrize("B,d,t,mode,zero", _kernel_cases())
def test_contra_loss_against_float64_numpy(B, d, t, mode, zero, cuda):
    from rechorus_amd import engine
    rng = np.random.default_rng(1000 * B + d)
    x = rng.normal(0, 1.0, (B, 2, d)).astype(np.float32)
    zero_row = None
    if zero:
        zero_row = B // 2
        x[zero_row, 0] = 0.0
    labels = _labels(mode, B, rng)
    want = contrarec_np.contra_loss(x[:, 0], x[:, 1], labels, t)
    what = f"B={B} d={d} t={t:g} labels={mode} chunks={engine.contra_layout(d, B)[0]}"
    _compare_loss(x, labels, t, want, what, cuda, zero_row)


def test_the_split_batch_is_where_the_layout_says(cuda):
    from rechorus_amd import _lib, engine
    s = _split_batch()
    assert engine.contra_layout(64, s)[0] == 2 and engine.contra_layout(64, s - 1)[0] == 1
    for B in (s - 1, s, 4096):
        assert _lib.load().rc_contra_workspace_bytes(64, B) == engine.contra_layout(64, B)[2]


def test_contra_loss_reruns_are_bit_identical(cuda):
    for B, d, mode in ((300, 64, "zipf"), (1025, 128, "none"), (17, 4, "equal")):
        rng = np.random.default_rng(B)
        x = rng.normal(0, 1.0, (B, 2, d)).astype(np.float32)
        labels = _labels(mode, B, rng)
        runs = [_run_loss(x, labels, 0.2, cuda) for _ in range(2)]
        assert runs[0][0] == runs[1][0]
        for a, b in zip(runs[0][1:], runs[1][1:]):
            assert _np(a).tobytes() == _np(b).tobytes(), (B, d, mode)


def test_backward_refuses_a_workspace_another_forward_overwrote(cuda):
    from rechorus_amd import engine, nn as hnn
    ws = engine.ContraWorkspace()
    a = torch.randn(8, 16, device=cuda, requires_grad=True)
    b = torch.randn(8, 16, device=cuda, requires_grad=True)
    first = hnn.contra_loss(a, b, None, 0.2, workspace=ws)
    hnn.contra_loss(a, b, None, 0.2, workspace=ws)
    with pytest.raises(RuntimeError, match="workspace"):
        first.backward()


# ---- the forward-indexed position embedding -------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 20, 50])
@pytest.mark.parametrize("d", [4, 64, 128])
def test_forward_position_embed_and_its_table_gradient(L, d, cuda):
    from rechorus_amd import engine
    rng = np.random.default_rng(L * 1000 + d)
    B, n_items = 37, 90
    I = rng.normal(0, 0.5, (n_items, d)).astype(np.float32)
    Pos = rng.normal(0, 0.5, (L + 1, d)).astype(np.float32)
    lengths = rng.integers(0, L + 1, B).astype(np.int64)
    lengths[:3] = (0, 1, L)
    hist = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        hist[b, :lengths[b]] = rng.integers(1, n_items, lengths[b])
    h, n = torch.from_numpy(hist).to(cuda), torch.from_numpy(lengths).to(cuda)
    X = engine.seq_embed_fwdpos(torch.from_numpy(I).to(cuda), torch.from_numpy(Pos).to(cuda), h, n)
    want = contrarec_np.embed_fwdpos(I, Pos, hist, lengths)
    assert X.shape == (B * L, d)
    _check(X.view(B, L, d), want, f"embed L={L} d={d}")
    invalid = torch.from_numpy(np.arange(L)[None, :] >= lengths[:, None]).to(cuda)
    assert X.view(B, L, d)[invalid].abs().sum().item() == 0.0      # the padding is written as zeros
    dX = rng.normal(0, 1.0, (B, L, d)).astype(np.float32)
    G = engine.seq_pos_grad_fwdpos(torch.from_numpy(dX).to(cuda).view(B * L, d), n, B, L, L + 1)
    _check(G, contrarec_np.pos_grad_fwdpos(dX, lengths, L + 1), f"pos grad L={L} d={d}")
    assert G[L].abs().sum().item() == 0.0      # row L of the table is never used


# ---- the model file against the goldens ----------------------------------------------------------------------------------------------

def _load_case(case):
    return contrarec_np.load_case(os.path.join(GOLDEN_DIR, case + ".npz"))


def _load(m, g, prefix):
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(torch.from_numpy(g[prefix + k.replace(".", "__")]))


def _model(g, dev, prefix="P0_"):
    from models.sequential.ContraRec import ContraRec
    n_items, d, L, B, C, seed = (int(x) for x in g["meta"])
    lr, l2, gamma, ctc_temp, ccc_temp = (float(x) for x in g["hyper"])
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=C - 1, dropout=0, test_all=0, emb_size=d, history_max=L,
                           gamma=gamma, beta_a=3, beta_b=3, ctc_temp=ctc_temp, ccc_temp=ccc_temp, encoder="BERT4Rec", batch_size=B)
    m = ContraRec(args, SimpleNamespace(n_users=50, n_items=n_items)).to(dev)
    _load(m, g, prefix)
    return m


def _feed(g, suffix, dev, phase="train"):
    t = lambda a: torch.from_numpy(a).to(dev)
    if phase != "train":
        return {"item_id": t(g["eval_iid"]), "history_items": t(g["eval_hist"]), "lengths": t(g["eval_lengths"]), "batch_size": 8,
                "phase": phase}
    return {"item_id": t(g["item_id" + suffix]), "history_items": t(g["hist" + suffix]), "history_items_a": t(g["hist" + suffix + "_a"]),
            "history_items_b": t(g["hist" + suffix + "_b"]), "lengths": t(g["lengths" + suffix]), "batch_size": len(g["lengths" + suffix]),
            "phase": phase}


def _runner(opt, lr, l2):
    from helpers.BaseRunner import BaseRunner
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.train, a.log_file = 1, "/tmp/rechorus_amd_test/log.txt"
    a.optimizer, a.lr, a.l2, a.graph, a.engine = opt, lr, l2, 0, "dense"
    return BaseRunner(a)


@pytest.mark.parametrize("case", CASES)
def test_golden_case(case, cuda):
    g = _load_case(case)
    n_items, d, L, B, C, seed = (int(x) for x in g["meta"])
    lr, l2, gamma, ctc_temp, ccc_temp = (float(x) for x in g["hyper"])
    opt = str(g["opt"])
    m = _model(g, cuda)
    m.train()
    out = m(_feed(g, "", cuda))
    ctc, ccc = m.ctc_loss(out), m.ccc_loss(out)
    loss = ctc + gamma * ccc
    loss.backward()
    _check(out["prediction"], g["pred"], case + " pred")
    feats = torch.stack([torch.nn.functional.normalize(v.detach(), dim=-1) for v in out["views"]], 1)
    _check(feats, g["features"], case + " features")
    _check_scalar(ctc.item(), g["ctc"], case + " ctc loss")
    if B == 1:
        assert abs(ccc.item()) <= 1e-6 and abs(float(g["ccc"])) <= 1e-6      # N = 2: the 1e-10 guard's effect
    else:
        _check_scalar(ccc.item(), g["ccc"], case + " ccc loss")
    _check_scalar(loss.item(), g["loss"], case + " loss")
    params = dict(m.named_parameters())
    gmax = max(float(np.abs(g["G_" + k.replace(".", "__")]).max()) for k in params)
    for k, p in params.items():
        floor = 1e-6 * gmax if k.endswith("k_linear.bias") else 0.0      # exactly 0 in exact arithmetic: see the module docstring
        _check(p.grad, g["G_" + k.replace(".", "__")], f"{case} grad {k}", floor)

    m2 = _model(g, cuda)
    m2.optimizer = _runner(opt, lr, l2)._build_optimizer(m2)
    m2.train()
    for step, suffix in enumerate(("", "2")):
        m2.optimizer.zero_grad()
        ls = m2.loss(m2(_feed(g, suffix, cuda)))
        ls.backward()
        m2.optimizer.step()
        _check_scalar(ls.item(), g["losses"][step], f"{case} fit() loss {step + 1}")
    extra = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
    for k, v in m2.state_dict().items():
        key = k.replace(".", "__")
        if k.endswith("k_linear.bias") and opt in ("Adam", "Adagrad"):
            moved = np.abs(_np(v).astype(np.float64) - g["P0_" + key])
            assert moved.max() <= 2 * lr * 1.001 + 1e-7, (case, k, moved.max(), lr)
            continue
        assert_update_close(_np(v), g["P0_" + key], g["P2_" + key], what=f"{case} {k} after two iterations", extra_atol=extra,
                            outlier_atol=2 * lr)
    _load(m2, g, "P2_")
    m2.eval()
    ep = m2(_feed(g, "", cuda, phase="test"))["prediction"]      # the evaluation phase needs no torch.no_grad() around it
    assert ep.shape == g["eval_pred"].shape and not ep.requires_grad
    _check(ep, g["eval_pred"], case + " eval pred")


def test_three_b_pass_equals_three_passes(cuda):
    """the training forward encodes the history and its two views as ONE pass over 3 B sequences: the encoder is per sequence, so
    each view equals a pass of its own (to the tolerance: a GEMM over another row count may tile differently)"""
    g = _load_case("contrarec_d64_l20_adam_b77")
    m = _model(g, cuda)
    feed = _feed(g, "", cuda)
    with torch.no_grad():
        out = m(feed)
        for view, key in zip(out["views"], ("history_items_a", "history_items_b")):
            alone = m.encoder(m.i_embeddings.weight, feed[key], feed["lengths"])
            _check(view, _np(alone), "3 B pass against a pass of " + key)


# ---- CLI --------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("contrarec_data"))
    make_dataset(root, "synth", n_users=300, n_items=250, per_user=14, seed=5)
    return root


@pytest.mark.parametrize("batch_size,test_all", [("4096", "0"), ("256", "1")])
def test_cli_trains_one_epoch(batch_size, test_all, synth_root, tmp_path, cuda, monkeypatch):
    """the reference's example line (batch 4096) and a multi-batch epoch under --test_all"""
    import main
    from rechorus_amd import graph as hgraph, nn as hnn
    replays, native = [], []
    run0, loss0 = hgraph.GraphedStep.run, hnn.contra_loss
    monkeypatch.setattr(hgraph.GraphedStep, "run", lambda self, b: replays.append(1) or run0(self, b))
    monkeypatch.setattr(hnn, "contra_loss", lambda *a, **k: native.append(a[0].shape[0]) or loss0(*a, **k))
    log = str(tmp_path / "log" / "run.txt")
    res = main.run(["--model_name", "ContraRec", "--emb_size", "64", "--lr", "1e-4", "--l2", "1e-6", "--history_max", "20",
                    "--encoder", "BERT4Rec", "--num_neg", "1", "--ctc_temp", "1", "--ccc_temp", "0.2", "--batch_size", batch_size,
                    "--gamma", "1", "--dataset", "synth", "--path", synth_root + "/", "--epoch", "1", "--num_workers", "0",
                    "--regenerate", "1", "--test_all", test_all, "--log_file", log, "--model_path", str(tmp_path / "m.pt"),
                    "--topk", "5,10", "--save_final_results", "0"])
    text = open(log).read()
    m = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", text)
    assert m and np.isfinite(float(m.group(1))), text[-2000:]
    hr = float(re.search(r"HR@5:([0-9.]+)", res["test"]).group(1))
    assert 0.0 <= hr <= 1.0 and "NDCG@10" in res["test"]
    assert native and not replays      # the loss kernels trained; the shuffled dense step runs eagerly, never from a hipGraph
    assert max(native) <= int(batch_size) and (batch_size == "4096" or len(native) > 1)
