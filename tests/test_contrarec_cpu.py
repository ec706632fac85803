"""CPU: ContraRec's host side against the reference's fixtures (tests/golden/make_golden_contrarec.py) -- the float64 restatement
of the encoder, both losses and their gradients (tests/contrarec_np.py) against every golden, the Dataset's augmentations bit
for bit, flags, state_dict keys, the three refusals, the loss kernels' shape envelope and the class lookup.  No kernel runs.

Tolerance: the goldens are float32 results of the reference, the restatement is float64: 2e-5 of the tensor's largest entry.
The B = 1 golden's context-context loss is ~3e-11 and its gradients ~1e-12 (the effect of the reference's 1e-10): those are
compared by the absolute bound 1e-6.  The contraloss_f64 fixtures are float64 on both sides: 1e-9 of the largest entry (the
stored gradients are rounded to fp32: 1e-7)."""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import contrarec_np  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

CASES = [c for c in golden_cases("contrarec_d") if not c.endswith(("_grads", "_after"))]
F64_FILES = ("contraloss_f64", "contraloss_f64_b1025_d64", "contraloss_f64_b1025_d32")
TOL = 2e-5


def rel_err(got, want, floor=0.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(float(np.abs(want).max()), floor, 1e-300))


def load_case(case):
    return contrarec_np.load_case(os.path.join(GOLDEN_DIR, case + ".npz"))


def params(g, prefix="P0_"):
    return {k: g[prefix + k.replace(".", "__")] for k in g["state_keys"].tolist()}


def f64_cases():
    """every case of the three contraloss_f64 files -> (B, d, t, labels | None, x [B, 2, d] float64, loss, grad)"""
    out = []
    for f in F64_FILES:
        g = load_golden(f)
        for i in range(int(g["n"])):
            B, d, distinct = (int(v) for v in g["shape_%d" % i])
            labels = g["labels_%d" % i] if distinct else None
            out.append((B, d, float(g["t_%d" % i]), labels, g["x_%d" % i].astype(np.float64) / 32.0, float(g["loss_%d" % i]),
                        g["grad_%d" % i]))
    return out


def _args(**kw):
    a = dict(device="cpu", model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=64, history_max=20, gamma=1.0,
             beta_a=3, beta_b=3, ctc_temp=1.0, ccc_temp=0.2, encoder="BERT4Rec", batch_size=256)
    a.update(kw)
    return SimpleNamespace(**a)


def test_golden_cases_exist_and_fit_the_size_limit():
    assert len(CASES) == 5, CASES
    shapes = set()
    for c in CASES:
        for part in ("", "_grads", "_after"):
            assert os.path.getsize(os.path.join(GOLDEN_DIR, c + part + ".npz")) < 1 << 20
        g = load_case(c)
        n_items, d, L, B, C, seed = (int(x) for x in g["meta"])
        assert n_items <= 200
        shapes.add((d, L, B, str(g["opt"])))
        assert set(np.unique(g["lengths"]).tolist()) <= {1, min(2, L), max(L - 1, 1), L}
        assert g["hist_a"].shape == g["hist"].shape == g["hist_b"].shape
        assert g["hist_a"].max() <= n_items and g["hist"].max() < n_items     # the mask token is n_items
    assert shapes == {(64, 20, 77, "Adam"), (32, 7, 160, "SGD"), (128, 50, 33, "Adagrad"), (4, 1, 3, "SGD"), (64, 20, 1, "Adam")}
    g = load_case("contrarec_d32_l7_sgd_b160")
    assert len(np.unique(g["item_id"][:, 0])) <= 5          # many positives per row
    assert (load_case("contrarec_d64_l20_adam_b77")["hist_a"] == 200).any()   # a masked position
    got = [(B, d, t, None if lab is None else len(np.unique(lab)) <= n) for (B, d, t, lab, _, _, _), n in
           zip(f64_cases(), (1, 7, 40, 0, 3000, 2))]
    assert got == [(2, 4, 0.2, True), (33, 64, 0.2, True), (300, 128, 0.05, True), (33, 64, 0.2, None), (1025, 64, 0.2, True),
                   (1025, 32, 1.0, True)]
    for f in F64_FILES + ("contrarec_augment",):
        assert os.path.getsize(os.path.join(GOLDEN_DIR, f + ".npz")) < 1 << 20


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference(case):
    g = load_case(case)
    n_items, d, L, B, C, seed = (int(x) for x in g["meta"])
    lr, l2, gamma, ctc_temp, ccc_temp = (float(x) for x in g["hyper"])
    P = params(g)
    r = contrarec_np.train_step(P, g["hist"], g["hist_a"], g["hist_b"], g["lengths"], g["item_id"], ctc_temp, ccc_temp, gamma)
    errs = {"pred": rel_err(r["pred"], g["pred"]), "features": rel_err(r["features"], g["features"]),
            "ctc": abs(r["ctc"] - float(g["ctc"])) / max(1.0, abs(float(g["ctc"])))}
    if B == 1:      # N = 2: the loss is the 1e-10 guard's effect, ~3e-11
        assert abs(r["ccc"]) <= 1e-6 and abs(float(g["ccc"])) <= 1e-6
    else:
        errs["ccc"] = abs(r["ccc"] - float(g["ccc"])) / max(1.0, abs(float(g["ccc"])))
    errs["loss"] = abs(r["loss"] - float(g["loss"])) / max(1.0, abs(float(g["loss"])))
    gmax = max(float(np.abs(g["G_" + k.replace(".", "__")]).max()) for k in P)
    for k in P:
        # a gradient that is exactly 0 in exact arithmetic (the key biases: a softmax is invariant to a shift of its row) is pure
        # round-off in the reference: floor of 1e-6 of the batch's largest gradient entry
        errs["G " + k] = rel_err(r["G"][k], g["G_" + k.replace(".", "__")], 1e-6 * gmax / TOL)
    ev = contrarec_np.predict(params(g, "P2_"), g["eval_hist"], g["eval_lengths"], g["eval_iid"])
    errs["eval_pred"] = rel_err(ev, g["eval_pred"])
    print(case, {k: "%.2e" % v for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if v > TOL}
    assert not bad, bad


def test_float64_contra_loss_reproduces_the_float64_fixture():
    for B, d, t, labels, x, loss, grad in f64_cases():
        got, dva, dvb = contrarec_np.contra_loss(x[:, 0], x[:, 1], labels, t)
        g = np.stack([dva, dvb], 1)
        print("contraloss_f64 B=%d d=%d t=%g: loss err %.2e, grad err %.2e" % (B, d, t, abs(got - loss), rel_err(g, grad)))
        assert abs(got - loss) <= 1e-9 * max(1.0, abs(loss))
        assert rel_err(g, grad) <= 1e-7      # the fixture's gradient is the float64 one rounded to fp32


def test_encoder_backward_agrees_with_autograd_in_float64():
    import torch
    from utils import layers
    rng = np.random.default_rng(7)
    n_items, d, L, B = 12, 8, 5, 6
    blocks = torch.nn.ModuleList([layers.TransformerLayer(d_model=d, d_ff=d, n_heads=2) for _ in range(2)]).double()
    I = torch.tensor(rng.normal(0, 0.5, (n_items + 1, d)), requires_grad=True)
    Pos = torch.tensor(rng.normal(0, 0.5, (L + 1, d)), requires_grad=True)
    with torch.no_grad():
        for p in blocks.parameters():
            p.copy_(torch.tensor(rng.normal(0, 0.5, tuple(p.shape))))
    lengths = np.array([1, 2, 5, 4, 3, 5])
    hist = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        hist[b, :lengths[b]] = rng.integers(1, n_items + 1, lengths[b])
    P = {"i_embeddings.weight": I.detach().numpy(), "encoder.p_embeddings.weight": Pos.detach().numpy()}
    P.update({"encoder.transformer_block." + k: v.detach().numpy() for k, v in blocks.state_dict().items()})
    hv, cache = contrarec_np.encode(P, hist, lengths)
    dhv = rng.normal(0, 1, hv.shape)
    G = {k: np.zeros(v.shape) for k, v in P.items()}
    contrarec_np.encode_bwd(P, hist, lengths, cache, dhv, G)
    h, n = torch.from_numpy(hist), torch.from_numpy(lengths)
    valid = torch.arange(L)[None, :] < n[:, None]
    seq = I[h] + Pos[torch.arange(L)[None, :] * valid.long()]
    for blk in blocks:
        seq = blk(seq, valid.view(B, 1, 1, L))
    out = (seq * valid[:, :, None])[torch.arange(B), n - 1]
    assert rel_err(hv, out.detach().numpy()) <= 1e-12
    (out * torch.from_numpy(dhv)).sum().backward()
    want = {"i_embeddings.weight": I.grad, "encoder.p_embeddings.weight": Pos.grad}
    want.update({"encoder.transformer_block." + k: p.grad for k, p in blocks.named_parameters()})
    scale = max(float(v.abs().max()) for v in want.values())
    for k, v in want.items():
        assert rel_err(G[k], v.numpy(), scale) <= 1e-10, k


def test_dataset_reproduces_the_reference_augmentations_bit_for_bit():
    from models.sequential.ContraRec import ContraRec
    g = load_golden("contrarec_augment")
    ds = object.__new__(ContraRec.Dataset)
    ds.model = SimpleNamespace(beta_a=int(g["beta"][0]), beta_b=int(g["beta"][1]), mask_token=int(g["mask_token"]))
    off = g["offsets"]
    assert len(off) == 41 and sorted(set(np.diff(off).tolist())) == list(range(1, 21))
    np.random.seed(int(g["seed"]))
    kinds = set()
    for s in range(40):
        seq = g["items"][off[s]:off[s + 1]]
        before = seq.copy()
        for name in ("a", "b"):
            view = ds.augment(seq)
            assert np.array_equal(view, g[name][off[s]:off[s + 1]]), (s, name)
            kinds.add("mask" if (view == ds.model.mask_token).any() else "reorder")
        assert np.array_equal(seq, before)      # the history itself is left as it is
    assert kinds == {"mask", "reorder"}


def test_get_feed_dict_adds_the_two_views_in_training_only_and_collate_pads_them():
    from models.BaseModel import SequentialModel
    from models.sequential.ContraRec import ContraRec
    assert issubclass(ContraRec.Dataset, SequentialModel.Dataset)
    assert ContraRec.Dataset._get_feed_dict is not SequentialModel.Dataset._get_feed_dict      # keeps the DataLoader path
    his = {1: [(3, 0), (4, 1), (5, 2), (6, 3)], 2: [(7, 0), (8, 1)]}
    for phase in ("train", "test"):
        ds = object.__new__(ContraRec.Dataset)
        ds.model = SimpleNamespace(beta_a=3, beta_b=3, mask_token=9, history_max=20, test_all=0)
        ds.corpus, ds.phase = SimpleNamespace(user_his=his, n_items=9), phase
        ds.data = {"user_id": [1, 2], "item_id": [6, 8], "position": [3, 1], "neg_items": [[2], [2]]}
        feeds = [ds._get_feed_dict(i) for i in range(2)]
        assert ("history_items_a" in feeds[0]) == ("history_items_b" in feeds[0]) == (phase == "train")
        batch = ds.collate_batch(feeds)
        assert batch["history_items"].tolist() == [[3, 4, 5], [7, 0, 0]] and batch["lengths"].tolist() == [3, 1]
        if phase == "train":
            for k in ("history_items_a", "history_items_b"):
                assert tuple(batch[k].shape) == (2, 3) and batch[k][1, 1:].tolist() == [0, 0]
                assert sorted(x for x in batch[k][0].tolist() if x != 9) == [x for x in (3, 4, 5) if x in batch[k][0].tolist()]


def test_class_lookup_flags_and_log_args():
    import main
    cls = main.find_class("model", ("ContraRec", ""))
    assert cls.__name__ == "ContraRec" and cls.reader == "SeqReader" and cls.runner == "BaseRunner"
    assert cls.__module__ == "models.contrarec_model"
    import models.sequential.ContraRec as facade
    assert facade.ContraRec is cls
    assert cls.extra_log_args == ["gamma", "num_neg", "batch_size", "ctc_temp", "ccc_temp", "encoder"]
    # the labels of the context-context term are candidate column 0 as the forward sees it: the runner shuffles as the reference's
    assert not getattr(cls, "candidate_permutation_equivariant", False)
    assert not hasattr(cls, "hip_train_step")
    d, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
    assert (d.emb_size, d.gamma, d.beta_a, d.beta_b, d.ctc_temp, d.ccc_temp, d.encoder, d.history_max, d.num_neg) == \
        (64, 1, 3, 3, 1, 0.2, "BERT4Rec", 20, 1)
    assert isinstance(d.beta_a, int) and isinstance(d.gamma, (int, float))
    a, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args(["--ccc_temp", "0.5", "--encoder", "Caser", "--gamma", "0.1"])
    assert (a.ccc_temp, a.encoder, a.gamma) == (0.5, "Caser", 0.1)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_match_the_reference(case):
    from models.sequential.ContraRec import ContraRec
    g = load_case(case)
    n_items, d, L, B, C, seed = (int(x) for x in g["meta"])
    m = ContraRec(_args(emb_size=d, history_max=L, batch_size=B), SimpleNamespace(n_users=5, n_items=n_items))
    assert sorted(m.state_dict().keys()) == sorted(g["state_keys"].tolist())
    assert "encoder.p_embeddings.weight" in m.state_dict() and "encoder.transformer_block.1.masked_attn_head.q_linear.weight" in m.state_dict()
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == g["P0_" + k.replace(".", "__")].shape, k
    assert m.i_embeddings.weight.shape[0] == n_items + 1 and m.mask_token == n_items
    assert 0.005 < float(m.i_embeddings.weight.std()) < 0.02      # BaseModel.init_weights


@pytest.mark.parametrize("flags,names", [
    (dict(encoder="GRU4Rec"), "--encoder GRU4Rec"), (dict(encoder="Caser"), "--encoder Caser"),
    (dict(emb_size=6), "--emb_size"), (dict(emb_size=1028), "--emb_size"), (dict(history_max=1025), "--history_max"),
    (dict(history_max=0), "--history_max"),
    (dict(emb_size=260), "--emb_size"), (dict(batch_size=(1 << 19) + 1), "--batch_size")])
def test_refusals_raise_in_init_and_name_the_flag(flags, names):
    from models.sequential.ContraRec import ContraRec
    with pytest.raises(ValueError, match=names):
        ContraRec(_args(**flags), SimpleNamespace(n_users=5, n_items=6))


def test_unknown_encoder_is_invalid_and_the_envelope_edges_construct():
    from models.sequential.ContraRec import ContraRec
    with pytest.raises(ValueError, match="Invalid sequence encoder"):
        ContraRec(_args(encoder="LSTM"), SimpleNamespace(n_users=5, n_items=6))
    for flags in (dict(emb_size=4, history_max=1, batch_size=1), dict(emb_size=256, history_max=1024, batch_size=1 << 19)):
        ContraRec(_args(**flags), SimpleNamespace(n_users=5, n_items=6))


def test_forward_refuses_cpu_tensors():
    import torch
    from models.sequential.ContraRec import ContraRec
    m = ContraRec(_args(), SimpleNamespace(n_users=5, n_items=6))
    feed = {"item_id": torch.ones(2, 2, dtype=torch.int64), "history_items": torch.ones(2, 3, dtype=torch.int64),
            "lengths": torch.tensor([3, 3]), "phase": "test", "batch_size": 2}
    with pytest.raises(RuntimeError, match="GPU only"):
        m(feed)


def test_check_shape_at_and_just_outside_every_edge():
    from rechorus_amd import _lib, engine
    lib = _lib.load()
    top = 1 << 19
    for d, B in ((4, 1), (256, 1), (4, top), (256, top), (64, 4096), (36, 77)):
        assert lib.rc_contra_check_shape(d, B) == _lib.RC_OK, (d, B)
        chunks, per, nbytes = engine.contra_layout(d, B)
        assert lib.rc_contra_workspace_bytes(d, B) == nbytes > 0, (d, B)      # the host-side layout is the library's
        assert 1 <= chunks <= 16 and (chunks - 1) * per < (2 * B + 31) // 32 <= chunks * per
        engine.contra_check_shape(d, B)
    for d, B in ((0, 8), (2, 8), (6, 8), (258, 8), (260, 8), (-4, 8), (64, 0), (64, -1), (64, top + 1)):
        assert lib.rc_contra_check_shape(d, B) == -4, (d, B)      # RC_ERR_UNSUPPORTED
        msg = lib.rc_last_error_string()
        assert msg.startswith(b"rc_contra_check_shape:") and b"outside the envelope" in msg
        assert ("emb_size=%d batch=%d" % (d, B)).encode() in msg
        assert lib.rc_contra_workspace_bytes(d, B) == 0
        with pytest.raises(ValueError, match="envelope"):
            engine.contra_check_shape(d, B)


def test_layout_splits_the_sweep_from_batch_17():
    from rechorus_amd import engine
    B = engine.contra_first_split_batch()
    assert B == 17      # N = 34: two 32-row column blocks, one per chunk
    assert engine.contra_layout(64, B)[0] == 2 and engine.contra_layout(64, B - 1)[0] == 1
    assert engine.contra_layout(64, 4096)[:2] == (8, 32) and engine.contra_layout(64, 16384)[0] == 2


def test_entry_points_refuse_bad_calls_without_a_gpu():
    import ctypes as C
    from rechorus_amd import _lib
    lib = _lib.load()
    p, q = C.c_void_p(256), C.c_void_p(260)
    big = 1 << 30

    def fwd(va=p, d=64, B=8, t=0.2, ws=p, ws_bytes=big, loss=p):
        return lib.rc_contra_loss_fwd(va, p, None, B, d, t, ws, ws_bytes, loss, None)

    def bwd(d=64, B=8, t=0.2, ws_bytes=big, ga=p):
        return lib.rc_contra_loss_bwd(p, None, B, d, t, p, ws_bytes, ga, p, None)
    for call, name in ((fwd, b"rc_contra_loss_fwd:"), (bwd, b"rc_contra_loss_bwd:")):
        assert call(d=30) == -4 and lib.rc_last_error_string().startswith(name)
        assert call(B=0) == -4 and b"outside the envelope" in lib.rc_last_error_string()
        assert call(ws_bytes=16) == -1 and b"workspace of 16 bytes" in lib.rc_last_error_string()
        assert call(t=0.0) == -1 and b"temperature" in lib.rc_last_error_string()
    assert fwd(va=None) == -1 and b"null pointer" in lib.rc_last_error_string()
    assert fwd(va=q) == -1 and b"16-byte aligned" in lib.rc_last_error_string()
    assert fwd(ws=q) == -1 and b"256-byte aligned" in lib.rc_last_error_string()
    assert bwd(ga=None) == -1 and b"null pointer" in lib.rc_last_error_string()
    assert lib.rc_seq_embed_fwdpos_fwd(None, p, p, p, 4, 5, 8, p, None) == -1 and b"rc_seq_embed_fwdpos_fwd: null pointer" in lib.rc_last_error_string()
    assert lib.rc_seq_embed_fwdpos_fwd(p, p, p, p, 4, 0, 8, p, None) == -1 and b"bad shape" in lib.rc_last_error_string()
    assert lib.rc_seq_pos_grad_fwdpos(p, p, 4, 5, 8, 0, p, None) == -1 and b"rc_seq_pos_grad_fwdpos: bad arguments" in lib.rc_last_error_string()
    assert lib.rc_seq_pos_grad_fwdpos(None, p, 4, 5, 8, 6, p, None) == -1 and b"null pointer" in lib.rc_last_error_string()


def test_engine_wrappers_raise_without_touching_the_gpu():
    import torch
    from rechorus_amd import engine, nn as hnn
    z = torch.zeros
    with pytest.raises(ValueError, match="envelope"):
        engine.contra_loss_fwd(z(3, 6), z(3, 6), None, 0.2)
    with pytest.raises(ValueError, match="alike"):
        engine.contra_loss_fwd(z(3, 8), z(4, 8), None, 0.2)
    with pytest.raises(ValueError, match="labels"):
        engine.contra_loss_fwd(z(3, 8), z(3, 8), z(2, dtype=torch.int64), 0.2)
    with pytest.raises(RuntimeError, match="GPU only"):
        hnn.contra_loss(z(3, 8), z(3, 8), None, 0.2)
    with pytest.raises(ValueError, match="position table"):
        engine.seq_embed_fwdpos(z(9, 8), z(4, 8), z(2, 5, dtype=torch.int64), z(2, dtype=torch.int64))
