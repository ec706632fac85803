"""CPU: the float64 restatement of SetRank's attention block (tests/setrank_np.py) against the block composed from torch's own
modules in float64 and, through the stored figures, against the reference's own `MAB`; rc_setmab_check_shape at the envelope's edges;
the bindings; SetRank's construction refusals, its state_dict keys (the reference's) and its init stream; the numpy model against
the reference's goldens."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
for p in (HERE, PLUGIN):
    if p not in sys.path:
        sys.path.insert(0, p)
import setrank_np as snp  # noqa: E402


@pytest.mark.parametrize("prob_id", [(5, 20, 7, 32, 2, 64, 1, 1, 1), (3, 17, 20, 16, 1, 16, 0, 0, 2), (4, 1, 1, 64, 4, 128, 0, 1, 3),
                                     (2, 20, 40, 64, 16, 128, 1, 1, 4), (3, 9, 33, 32, 4, 48, 0, 1, 5)])
def test_numpy_block_equals_torchs_modules_in_float64(prob_id):
    prob, H = snp.random_mab(*prob_id), prob_id[4]
    mab = snp.TorchMAB(prob[3], H, torch.float64)
    dev = snp.deviation(snp.run_module(mab, mab.params, prob, torch.float64), prob, H)
    assert dev["Y"] < 1e-13
    for k in snp.GRAD_NAMES:
        assert dev[k] < 1e-12, k


def test_a_shared_source_is_the_same_rows_for_every_list_and_its_gradient_their_sum():
    Qs, Ks, pad, W, dY = snp.random_mab(4, 5, 9, 16, 2, 32, 1, 1, 11)
    rep = np.repeat(Qs[None], 4, axis=0)
    assert (snp.mab_forward(Qs, Ks, pad, W, 2) == snp.mab_forward(rep, Ks, pad, W, 2)).all()
    a, b = snp.mab_backward(dY, Qs, Ks, pad, W, 2), snp.mab_backward(dY, rep, Ks, pad, W, 2)
    assert a["dQs"].shape == (5, 16) and np.allclose(a["dQs"], b["dQs"].sum(0), rtol=0, atol=1e-13)
    for k in snp.GRAD_NAMES[1:]:
        assert (a[k] == b[k]).all(), k


def test_every_problem_has_the_references_stored_deviations_and_is_conditioned():
    """the figures tests/golden/make_golden_setrank.py took from the reference's own MAB (SetRank.py:29-56): in float64 it IS the
    restatement to round-off; in float32 it deviates by less than 1e-4; the softmax is peaked and the mask matters"""
    devs = load_golden("setrank_mab_dev")
    for p in snp.MAB_PROBLEMS + snp.SELF_PROBLEMS:
        key = snp.mab_key(*p)
        for name in ("Y",) + snp.GRAD_NAMES:
            assert 0 <= float(devs[f"{key}/f64/{name}"]) < 1e-12, (key, name)
            assert 0 <= float(devs[f"{key}/{name}"]) < 1e-4, (key, name)
        pad = snp.problem(p)[2]
        if p[2] > 2:
            assert float(devs[key + "/maxp"]) > 2.0, key                   # more than twice the uniform probability
        if pad is not None and pad.sum() > 0:
            assert float(devs[key + "/mask"]) > 100 * snp.stored_bound(devs, key + "/Y")[0], key
    assert abs(float(devs["blind/drawn"]) - 1.0) < 0.025 and 3.2 <= float(devs["blind/scaled"]) <= 7.0
    grid = lambda shared: {p[2 if shared else 1] for p in snp.MAB_PROBLEMS if p[0] == 65 and p[3:8] == (64, 4, 128, shared, shared)}
    assert grid(1) == grid(0) == {1, 2, 15, 16, 17, 40, 48}
    assert {p[1:3] for p in snp.MAB_PROBLEMS if p[6:8] == (0, 1)} == {(17, 33), (33, 17), (1, 1)}
    assert len(snp.SHAPES) == len(snp.prm_np.SHAPES)      # the envelope admits every shape of the list encoder's grid at 17 / 20 rows
    assert {(p[0], p[6]) for p in snp.MAB_PROBLEMS if p[3:6] == (128, 4, 256)} == {(3, 0), (3, 1), (257, 0), (257, 1)}


# ---- the library's host side ------------------------------------------------------------------------------------------------------------
def _engine():
    from rechorus_amd import _lib, engine
    try:
        _lib.load()
    except _lib.RechorusHipMissing:
        pytest.skip("librechorus_hip.so is not built")
    return _lib, engine


def test_bindings_exist_and_the_header_declares_them():
    _lib, engine = _engine()
    names = {"rc_setmab_check_shape", "rc_setmab_fwd", "rc_setmab_bwd", "rc_setmab_bwd_workspace_bytes"}
    text = open(os.path.join(ROOT, "include", "rechorus_hip.h")).read()
    assert set(re.findall(r"\b(rc_setmab_\w+)\s*\(", text)) == names
    for name in names:
        assert callable(getattr(_lib.load(), name))
    for name in ("setmab_check_shape", "setmab_fwd", "setmab_bwd", "SetMabWorkspace"):
        assert hasattr(engine, name)
    from rechorus_amd import nn as hnn
    for name in ("set_attention_block", "set_attention_block_eval", "induced_set_block", "induced_set_block_eval"):
        assert callable(getattr(hnn, name))


def test_check_shape_at_the_edges_of_the_envelope():
    _lib, engine = _engine()
    lib = _lib.load()
    for nq, nk, d, H, dff, text in ((0, 20, 64, 4, 128, "outside the envelope"), (20, 0, 64, 4, 128, "outside the envelope"),
                                    (65, 20, 64, 4, 128, "outside the envelope"), (20, 65, 64, 4, 128, "outside the envelope"),
                                    (20, 40, 24, 2, 128, "outside the envelope"), (20, 40, 64, 3, 128, "outside the envelope"),
                                    (20, 40, 64, 32, 128, "outside the envelope"), (20, 40, 64, 4, 120, "outside the envelope"),
                                    (20, 40, 64, 4, 272, "outside the envelope"), (20, 40, 144, 4, 128, "outside the envelope"),
                                    (49, 49, 64, 4, 128, "bytes of LDS"), (64, 64, 64, 4, 128, "172544 bytes of LDS"),
                                    (20, 33, 128, 4, 256, "bytes of LDS"), (33, 20, 128, 4, 256, "bytes of LDS")):
        with pytest.raises(ValueError, match=text):
            engine.setmab_check_shape(nq, nk, d, H, dff)
        assert lib.rc_setmab_bwd_workspace_bytes(8, nq, nk, d, H, dff) == 0
        assert text == "outside the envelope" or not snp.admitted(nq, nk, d, dff)
    for n in range(1, 65):      # the induced block's two shapes, at every list length up to 64 and every width up to 64
        for d in (16, 32, 48, 64):
            engine.setmab_check_shape(snp.M, n, d, 4, 128)
            engine.setmab_check_shape(n, snp.M, d, 4, 128)
    for nq, nk, d, H, dff in ((48, 48, 64, 4, 128), (64, 48, 64, 4, 128), (48, 64, 64, 4, 128), (1, 1, 16, 1, 16), (32, 32, 128, 4, 256),
                              (64, 64, 32, 2, 128), (20, 48, 96, 4, 128), (20, 32, 128, 32, 128)):
        engine.setmab_check_shape(nq, nk, d, H, dff)
        assert snp.admitted(nq, nk, d, dff)
    # the workspace: the twelve gradients and a [nq, d] share per workgroup, at most 256 of them -- it stops growing with the lists
    P = 4 * 64 * 64 + 2 * 64 * 128 + 9 * 64 + 128 + 20 * 64
    per = (P + 63) // 64 * 64 * 4
    assert lib.rc_setmab_bwd_workspace_bytes(3, 20, 40, 64, 4, 128) == 3 * per
    assert lib.rc_setmab_bwd_workspace_bytes(256, 20, 40, 64, 4, 128) == lib.rc_setmab_bwd_workspace_bytes(1 << 20, 20, 40, 64, 4, 128) == 256 * per
    assert lib.rc_setmab_bwd_workspace_bytes(0, 20, 40, 64, 4, 128) == 0


# ---- SetRank ----------------------------------------------------------------------------------------------------------------------------
def _args(**over):
    a = dict(device=torch.device("cpu"), model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, loss_n="BPR", emb_size=16,
             train_max_pos_item=3, train_max_neg_item=4, test_max_pos_item=3, test_max_neg_item=4, ranker_name="BPRMF",
             ranker_config_file="BPRMF.yaml", ranker_model_file="ranker.pt", tuneranker=0, n_blocks=2, num_heads=2, num_hidden_unit=32,
             history_max=5, setrank_type="IMSAB")
    a.update(over)
    return SimpleNamespace(**a)


@pytest.fixture()
def ranker_dir(tmp_path, monkeypatch):
    """./model/BPRMFImpression/ with a checkpoint of this repository's BPRMFImpression and its yaml (emb_size 8)"""
    import yaml
    from models.general.BPRMF import BPRMFImpression
    corpus = SimpleNamespace(n_users=11, n_items=23)
    folder = tmp_path / "model" / "BPRMFImpression"
    folder.mkdir(parents=True)
    torch.manual_seed(5)
    ranker = BPRMFImpression(_args(emb_size=8), corpus)
    torch.save(ranker.state_dict(), str(folder / "ranker.pt"))
    (folder / "BPRMF.yaml").write_text(yaml.safe_dump({"emb_size": 8, "history_max": 77}))
    monkeypatch.chdir(tmp_path)
    return corpus, {k: v.clone() for k, v in ranker.state_dict().items()}


def _build(cls_name, corpus, **over):
    _engine()
    from models.reranker import SetRank
    return getattr(SetRank, cls_name)(_args(**over), corpus)


MAB_KEYS = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "linear1.weight", "linear1.bias",
            "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


def _reference_keys(kind, blocks=2):
    """the reference's state_dict keys in its order: a module's own parameters (I) come before its children's"""
    enc = []
    for l in range(blocks):
        if kind == "IMSAB":
            enc.append("encoder.%d.I" % l)
        enc += ["encoder.%d.%s.%s" % (l, mab, k) for mab in (("MAB1", "MAB2") if kind == "IMSAB" else ("MAB1",)) for k in MAB_KEYS]
    return ["i_embeddings.weight", "ordinal_position_embedding.weight", "rFF0.weight", "rFF0.bias"] + enc + ["rFF1.weight", "rFF1.bias"]


@pytest.mark.parametrize("kind", ["IMSAB", "MSAB"])
def test_state_dict_keys_are_the_references_and_the_ranker_is_the_checkpoint(kind, ranker_dir):
    corpus, saved = ranker_dir
    torch.manual_seed(9)
    m = _build("SetRankGeneral", corpus, setrank_type=kind)
    keys = [k for k in m.state_dict().keys() if not k.startswith("ranker.")]
    assert keys == _reference_keys(kind)
    for k, v in saved.items():      # frozen, and the trained one: the head's init stream did not stay in it
        assert torch.equal(m.state_dict()["ranker." + k], v), k
    assert not any(p.requires_grad for p in m.ranker.parameters()) and not m.ranker.training
    # the position is added AFTER rFF0: its table has the hidden width, and rFF0 reads [i_emb | u_v | i_v] alone
    assert tuple(m.ordinal_position_embedding.weight.shape) == (7, 32) and tuple(m.rFF0.weight.shape) == (32, 16 + 2 * 8)
    assert m.encoder[0].MAB1.linear1.out_features == 128
    if kind == "IMSAB":
        assert tuple(m.encoder[1].I.shape) == (20, 32)
    assert {k for k, p in m.named_parameters() if p.requires_grad} == set(_reference_keys(kind))
    other = {k: torch.randn_like(v) for k, v in m.state_dict().items()}      # a checkpoint with the reference's keys loads
    m.load_state_dict(other)
    assert torch.equal(m.encoder[1].MAB1.attn.in_proj_weight, other["encoder.1.MAB1.attn.in_proj_weight"])
    with pytest.raises(RuntimeError):      # the holders hold parameters and are never called
        m.encoder[0](torch.zeros(1, 7, 32))


def test_init_stream_is_the_references(ranker_dir):
    """init_weights (normal 0, 0.01) reaches out_proj, linear1 / linear2, rFF0 / rFF1 and the embeddings; in_proj_weight is a bare
    Parameter and keeps its Xavier draw, in_proj_bias its zeros, the LayerNorms their ones and zeros; I is drawn normal(0, 0.01)
    inside the block's constructor and init_weights leaves it alone"""
    corpus, _ = ranker_dir
    torch.manual_seed(9)
    m = _build("SetRankGeneral", corpus)
    sd = m.state_dict()
    for k in _reference_keys("IMSAB"):
        v = sd[k]
        if "norm" in k:
            assert bool((v == (1.0 if k.endswith("weight") else 0.0)).all()), k
        elif k.endswith("in_proj_bias"):
            assert bool((v == 0).all()), k
        elif k.endswith("in_proj_weight"):
            bound = float(np.sqrt(6.0 / (32 + 96)))
            assert 0.8 * bound < float(v.abs().max()) <= bound, k
        else:
            assert float(v.abs().max()) < 0.06 and (v.numel() < 64 or 0.005 < float(v.std()) < 0.02), k
    torch.manual_seed(9)
    again = _build("SetRankGeneral", corpus).state_dict()
    assert all(torch.equal(sd[k], again[k]) for k in sd)


@pytest.mark.parametrize("over,text", [
    (dict(dropout=0.1), "--dropout 0.1 is not supported"),
    (dict(tuneranker=1), "--tuneranker 1 is not supported"),
    (dict(test_max_neg_item=5), "equal to the training widths"),
    (dict(test_max_pos_item=2), "equal to the training widths"),
    (dict(setrank_type="imsab"), "--setrank_type must be MSAB or IMSAB"),
    (dict(setrank_type="ISAB"), "--setrank_type must be MSAB or IMSAB"),
    (dict(num_hidden_unit=24), "outside the envelope"),
    (dict(num_heads=3), "outside the envelope"),
    (dict(setrank_type="MSAB", num_heads=3), "outside the envelope"),
    (dict(train_max_pos_item=40, train_max_neg_item=40, test_max_pos_item=40, test_max_neg_item=40), "outside the envelope"),
    (dict(num_hidden_unit=128, train_max_pos_item=20, train_max_neg_item=20, test_max_pos_item=20, test_max_neg_item=20), "bytes of LDS"),
    (dict(setrank_type="MSAB", num_hidden_unit=128, train_max_pos_item=20, train_max_neg_item=20, test_max_pos_item=20,
          test_max_neg_item=20), "bytes of LDS"),
])
def test_construction_refusals(over, text, ranker_dir):
    corpus, _ = ranker_dir
    _engine()
    from models.reranker.SetRank import SetRankGeneral
    with pytest.raises(ValueError, match=text):
        SetRankGeneral(_args(**over), corpus)


def test_main_finds_the_classes_by_either_spelling_and_the_flags_are_the_references():
    import argparse
    import main
    from models.reranker import SetRank
    assert main.find_class("model", ("SetRankGeneral", "")) is SetRank.SetRankGeneral
    assert main.find_class("model", ("SetRankSequential", "")) is SetRank.SetRankSequential
    assert main.find_class("model", ("SetRank", "General")) is SetRank.SetRankGeneral
    assert main.find_class("model", ("SetRank", "Sequential")) is SetRank.SetRankSequential
    a, _ = SetRank.SetRankGeneral.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
    assert (a.emb_size, a.n_blocks, a.num_heads, a.num_hidden_unit, a.setrank_type) == (64, 4, 4, 64, "IMSAB")
    assert SetRank.SetRankSequential.reader == "ImpressionSeqReader" and SetRank.SetRankGeneral.runner == "ImpressionRunner"


# ---- the reference's goldens ------------------------------------------------------------------------------------------------------------
MODEL_CASES = [c for c in golden_cases("setrank_") if c != "setrank_mab_dev"]


def test_the_golden_cases_have_the_properties_the_tests_rely_on():
    assert len(MODEL_CASES) == 4
    combos, singles, heads, widths = set(), 0, set(), set()
    for case in MODEL_CASES:
        g = load_golden(case)
        m = snp.meta(g)
        combos.add((m["seq"], str(g["setrank_type"])))
        heads.add(m["H"]), widths.add(m["hidden"])
        assert os.path.getsize(os.path.join(HERE, "golden", case + ".npz")) <= 600 * 1024
        for i in (1, 2, 3):
            valid = ~g["b%d/padding_mask" % i]
            assert valid.any(1).all()                                  # every list has a valid key
            singles += int(i == 3 and (valid.sum(1) == 1).any())
            if i < 3:      # the training batches: a negative in every list (the reference's BPR is NaN without one)
                assert valid[:, m["P"]:].any(1).all() and valid[:, :m["P"]].any(1).all()
        assert g["maxp"].shape == (m["blocks"], 2) and (g["maxp"][:, :len(snp.mab_names(g))] > 2.0).all(), case
        last = "encoder.%d.%s.norm2.bias" % (m["blocks"] - 1, snp.mab_names(g)[-1])
        assert np.isfinite(g["loss"]) and set(str(k) for k in g["zero_grad_keys"]) == {"rFF1.bias", last}
        scaled = dict(zip((str(k) for k in g["scale_keys"]), g["scale_vals"]))
        if str(g["setrank_type"]) == "IMSAB":      # the init's I is blind: the cases run on I x 100, recorded after the init stream
            assert all(scaled["encoder.%d.I" % l] == 100.0 for l in range(m["blocks"]))
    assert combos == {(0, "IMSAB"), (0, "MSAB"), (1, "IMSAB"), (1, "MSAB")} and singles == 4
    assert heads - {4} and 32 in widths


@pytest.mark.parametrize("case", MODEL_CASES)
def test_numpy_model_equals_the_reference_golden(case):
    g = load_golden(case)
    P0 = snp.scale_state({k[3:]: v for k, v in g.items() if k.startswith("I0/")}, g)
    for i, pre in ((1, ""), (3, "F/")):
        if i == 3 and snp.meta(g)["seq"]:
            continue      # (the sequential ranker's vectors are stored for the first batch only)
        valid = ~g["b%d/padding_mask" % i]
        xs, pred = snp.model_forward(g, i, P0)
        for l, x in enumerate(xs):
            want, got = snp.stored(g, pre, "X%d" % l, x[valid])
            assert snp.rel_err(got, want) <= snp.bound_for(g, pre + "X%d" % l)[0], (case, i, l)
        assert snp.rel_err(pred[valid], g[pre + "pred"][valid]) <= snp.bound_for(g, pre + "pred")[0], (case, i)


@pytest.mark.parametrize("case", MODEL_CASES)
def test_the_port_draws_the_references_init_stream(case, tmp_path, monkeypatch):
    """the port's class built on the CPU over the golden's ranker fixture: the reference's state_dict keys in its order, every head
    parameter bit for bit the reference's draw (asserted inside golden_model), the ranker the checkpoint"""
    _engine()
    g = load_golden(case)
    monkeypatch.chdir(tmp_path)
    model, P0 = snp.golden_model(g, torch.device("cpu"), tmp_path)
    assert type(model).__name__ == ("SetRankSequential" if snp.meta(g)["seq"] else "SetRankGeneral")
    assert model.setrank_type == str(g["setrank_type"]) and sorted(P0) == sorted(str(k) for k in g["state_keys"])
