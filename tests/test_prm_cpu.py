"""CPU: the float64 restatement of the list encoder block (tests/prm_np.py) against torch's own nn.TransformerEncoderLayer in float64;
the re-ranker bases' collate_batch additions with a stub ranker (padding mask, rank positions); PRM's construction refusals, its
state_dict keys (the reference's) and its init stream."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
for p in (HERE, PLUGIN):
    if p not in sys.path:
        sys.path.insert(0, p)
import prm_np as pnp  # noqa: E402


@pytest.mark.parametrize("prob_id", [(5, 7, 32, 2, 64, 1), (3, 17, 16, 1, 16, 2), (4, 1, 64, 4, 128, 3), (2, 40, 64, 16, 128, 4)])
def test_numpy_block_equals_torchs_module_in_float64(prob_id):
    X, pad, W, dY = pnp.random_block(*prob_id)
    H = prob_id[3]
    Y64, G64 = pnp.torch_block(X, pad, W, H, dY, torch.float64)
    assert pnp.rel_err(pnp.block_forward(X, pad, W, H), Y64) < 1e-13
    got = pnp.block_backward(dY, X, pad, W, H)
    for k in pnp.GRAD_NAMES:
        assert pnp.rel_err(got[k], G64[k]) < 1e-12, k


def test_every_layer_problem_has_a_stored_deviation_and_a_peaked_softmax():
    devs = load_golden("prm_layer_dev")
    for p in pnp.LAYER_PROBLEMS:
        key = pnp.layer_key(*p)
        for name in ("Y",) + pnp.GRAD_NAMES:
            assert 0 <= float(devs[f"{key}/{name}"]) < 1e-4, (key, name)
        if p[1] > 2:
            assert float(devs[key + "/maxp"]) > 2.0, key      # more than twice the uniform probability
    lengths = {p[1] for p in pnp.LAYER_PROBLEMS if p[2:5] == (64, 4, 128) and p[0] == 65}
    assert lengths == {1, 2, 15, 16, 17, 40, 64}
    assert {p[2:5] for p in pnp.LAYER_PROBLEMS if p[1] == 17 and p[0] == 257} == set(pnp.SHAPES)


def test_masks_cover_the_four_patterns():
    rng = np.random.default_rng(0)
    for n in (2, 9, 40):
        one, two, full = (pnp.make_mask(rng, k, n) for k in ("one", "two", "all"))
        assert one.sum() == n - 1 and full.sum() == 0 and two[0] == 0
        npos = (n + 1) // 2
        for seg in (two[:npos], two[npos:]):      # [valid | pad] in both segments
            assert (np.diff(seg.astype(int)) >= 0).all()
        for _ in range(20):
            assert pnp.make_mask(rng, "random", n).sum() < n


# ---- the re-ranker bases ---------------------------------------------------------------------------------------------------------------
class _StubRanker(torch.nn.Module):
    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, feed_dict):
        return dict(self.out)


def _stub_model(P, N, out):
    from models.BaseRerankerModel import RerankModel
    m = RerankModel.__new__(RerankModel)
    torch.nn.Module.__init__(m)
    m.device, m.ranker_name = torch.device("cpu"), "Stub"
    m.train_max_pos_item, m.train_max_neg_item = P, N
    m.ranker = _StubRanker(out)
    return m


def test_collate_additions_with_a_stub_ranker():
    rng = np.random.default_rng(3)
    B, P, N, d = 9, 3, 4, 8
    scores = torch.from_numpy(rng.standard_normal((B, P + N)).astype(np.float32))
    u_v, i_v = torch.randn(B, P + N, d), torch.randn(B, P + N, d)
    pos = torch.tensor([3, 1, 2, 1, 3, 2, 1, 3, 2])
    neg = torch.tensor([4, 0, 1, 4, 2, 3, 1, 0, 4])      # a single valid slot (list 1), all valid (list 0), padding inside the positives
    m = _stub_model(P, N, {"prediction": scores, "u_v": u_v, "i_v": i_v})
    feed = m.add_ranker_outputs({"pos_num": pos.clone(), "neg_num": neg.clone(), "item_id": torch.zeros(B, P + N, dtype=torch.long)}, B)
    col = torch.arange(P + N)[None, :]
    valid = (col < pos[:, None]) | ((col >= P) & (col < P + neg[:, None]))
    assert feed["batch_size"] == B and torch.equal(feed["padding_mask"], ~valid)
    assert torch.equal(feed["u_v"], u_v) and torch.equal(feed["i_v"], i_v)
    assert torch.equal(feed["scores"][valid], scores[valid]) and bool(torch.isinf(feed["scores"][~valid]).all())
    position = feed["position"].numpy()
    for b in range(B):
        assert sorted(position[b]) == list(range(P + N))                       # a permutation: the padded slots take the free ranks
        v = valid[b].numpy()
        want = (-scores[b].numpy()[v]).argsort().argsort()                     # the rank among the valid slots
        assert (position[b][v] == want).all() and (position[b][~v] >= v.sum()).all()
    assert valid[1].sum() == 1 and valid[0].all() and not valid[2, 2]


def test_a_ranker_without_vectors_is_refused():
    m = _stub_model(2, 2, {"prediction": torch.zeros(1, 4)})
    with pytest.raises(ValueError, match="does not return u_v / i_v"):
        m.add_ranker_outputs({"pos_num": torch.tensor([1]), "neg_num": torch.tensor([1])}, 1)


# ---- PRM --------------------------------------------------------------------------------------------------------------------------------
def _args(**over):
    a = dict(device=torch.device("cpu"), model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, loss_n="BPR", emb_size=16,
             train_max_pos_item=3, train_max_neg_item=4, test_max_pos_item=3, test_max_neg_item=4, ranker_name="BPRMF",
             ranker_config_file="BPRMF.yaml", ranker_model_file="ranker.pt", tuneranker=0, n_blocks=2, num_heads=2, num_hidden_unit=32,
             history_max=5)
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
    from rechorus_amd import _lib
    from models.reranker import PRM
    try:
        return getattr(PRM, cls_name)(_args(**over), corpus)
    except _lib.RechorusHipMissing:
        pytest.skip("librechorus_hip.so is not built")


REFERENCE_KEYS = (["i_embeddings.weight", "ordinal_position_embedding.weight", "rFF0.weight", "rFF0.bias"]
                  + ["encoder.%d.%s" % (l, k) for l in range(2) for k in
                     ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                      "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
                      "norm2.bias")] + ["rFF1.weight", "rFF1.bias"])


def test_state_dict_keys_are_the_references_and_the_ranker_is_the_checkpoint(ranker_dir):
    corpus, saved = ranker_dir
    torch.manual_seed(9)
    m = _build("PRMGeneral", corpus)
    keys = list(m.state_dict().keys())
    assert sorted(keys) == sorted(["ranker.u_embeddings.weight", "ranker.i_embeddings.weight"] + REFERENCE_KEYS)
    for k, v in saved.items():      # frozen, and the trained one: the head's init stream did not stay in it
        assert torch.equal(m.state_dict()["ranker." + k], v), k
    assert not any(p.requires_grad for p in m.ranker.parameters()) and not m.ranker.training
    assert m.ranker_emb_size == 8 and m.ranker.return_vectors is True
    assert tuple(m.ordinal_position_embedding.weight.shape) == (7, 16 + 2 * 8) and tuple(m.rFF0.weight.shape) == (32, 32)
    assert m.encoder[0].linear1.out_features == 128
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    assert trainable == set(REFERENCE_KEYS)
    # a checkpoint with the reference's keys loads
    other = {k: torch.randn_like(v) for k, v in m.state_dict().items()}
    m.load_state_dict(other)
    assert torch.equal(m.encoder[1].self_attn.in_proj_weight, other["encoder.1.self_attn.in_proj_weight"])
    m.train()
    assert m.training and not m.ranker.training


def test_init_stream_is_the_references(ranker_dir):
    """init_weights (normal 0, 0.01) reaches out_proj, linear1 / linear2, rFF0 / rFF1 and the embeddings; in_proj_weight is a bare
    Parameter and keeps its Xavier draw, in_proj_bias its zeros, the LayerNorms their ones and zeros"""
    corpus, _ = ranker_dir
    torch.manual_seed(9)
    m = _build("PRMGeneral", corpus)
    sd = m.state_dict()
    for k in REFERENCE_KEYS:
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
    # the same seed gives the same head whatever checkpoint the ranker holds
    torch.manual_seed(9)
    again = _build("PRMGeneral", corpus).state_dict()
    assert all(torch.equal(sd[k], again[k]) for k in sd)


@pytest.mark.parametrize("over,text", [
    (dict(dropout=0.1), "--dropout 0.1 is not supported"),
    (dict(tuneranker=1), "--tuneranker 1 is not supported"),
    (dict(test_max_neg_item=5), "equal to the training widths"),
    (dict(test_max_pos_item=2), "equal to the training widths"),
    (dict(num_hidden_unit=24), "outside the envelope"),
    (dict(num_heads=3), "outside the envelope"),
    (dict(train_max_pos_item=40, train_max_neg_item=40, test_max_pos_item=40, test_max_neg_item=40), "outside the envelope"),
    (dict(num_hidden_unit=128, train_max_pos_item=20, train_max_neg_item=20, test_max_pos_item=20, test_max_neg_item=20), "bytes of LDS"),
])
def test_construction_refusals(over, text, ranker_dir):
    corpus, _ = ranker_dir
    from rechorus_amd import _lib
    from models.reranker.PRM import PRMGeneral
    try:
        with pytest.raises(ValueError, match=text):
            PRMGeneral(_args(**over), corpus)
    except _lib.RechorusHipMissing:
        pytest.skip("librechorus_hip.so is not built")


def test_sequential_base_takes_history_max_from_the_flags_not_the_yaml(tmp_path, monkeypatch):
    import yaml
    from models.sequential.SASRec import SASRecImpression
    corpus = SimpleNamespace(n_users=11, n_items=23)
    folder = tmp_path / "model" / "SASRecImpression"
    folder.mkdir(parents=True)
    ra = _args(emb_size=16, num_layers=1, num_heads=2, history_max=5)
    assert SASRecImpression.return_vectors is False
    torch.save(SASRecImpression(ra, corpus).state_dict(), str(folder / "ranker.pt"))
    (folder / "SASRec.yaml").write_text(yaml.safe_dump({"emb_size": 16, "num_layers": 1, "num_heads": 2, "history_max": 77}))
    monkeypatch.chdir(tmp_path)
    m = _build("PRMSequential", corpus, ranker_name="SASRec", ranker_config_file="SASRec.yaml", emb_size=32, num_heads=4, num_hidden_unit=64,
               n_blocks=1)
    assert m.history_max == 5 and m.ranker.max_his == 5 and m.ranker.emb_size == 16 and m.ranker.num_heads == 2
    assert m.ranker.return_vectors is True and type(m).reader == "ImpressionSeqReader"
    assert tuple(m.ordinal_position_embedding.weight.shape) == (7, 32 + 2 * 16)


def test_main_finds_the_classes_by_either_spelling():
    import main
    from models.reranker import PRM
    assert main.find_class("model", ("PRMGeneral", "")) is PRM.PRMGeneral
    assert main.find_class("model", ("PRMSequential", "")) is PRM.PRMSequential
    assert main.find_class("model", ("PRM", "General")) is PRM.PRMGeneral
    for name in (("PRMNothing", ""), ("PRM", "Nothing")):
        with pytest.raises(ValueError, match="unknown model"):
            main.find_class("model", name)


# ---- the reference's goldens ------------------------------------------------------------------------------------------------------------
from conftest import golden_cases  # noqa: E402

MODEL_CASES = [c for c in golden_cases("prm_") if c != "prm_layer_dev"]


def test_the_golden_cases_have_the_properties_the_tests_rely_on():
    assert len(MODEL_CASES) == 4
    singles = fulls = inside = 0
    for case in MODEL_CASES:
        g = load_golden(case)
        m = pnp.meta(g)
        for i in (1, 2, 3):
            valid = ~g["b%d/padding_mask" % i]
            assert valid.any(1).all()                                  # every list has a valid key
            singles += int((valid.sum(1) == 1).any() and valid.shape[1] > 1)
            fulls += int(valid.all(1).any())
            inside += int((~valid[:, :m["P"]]).any() and valid[:, m["P"]:].any())
            if i < 3:      # the training batches: a negative in every list (the reference's BPR is NaN without one)
                assert valid[:, m["P"]:].any(1).all() and valid[:, :m["P"]].any(1).all()
        for l, x in enumerate(g["maxp"]):
            assert x == 0 or x > 2.0, (case, l)                        # more than twice the uniform probability
        assert np.isfinite(g["loss"]) and set(str(k) for k in g["zero_grad_keys"]) == {"rFF1.bias", "encoder.%d.norm2.bias" % (m["blocks"] - 1)}
    assert singles >= 1 and fulls >= 4 and inside >= 1


@pytest.mark.parametrize("case", MODEL_CASES)
def test_numpy_model_equals_the_reference_golden(case):
    g = load_golden(case)
    P0 = pnp.scale_state({k[3:]: v for k, v in g.items() if k.startswith("I0/")}, g)
    for i, pre in ((1, ""), (3, "F/")):
        if i == 3 and pnp.meta(g)["seq"]:
            continue      # (the sequential ranker's vectors are stored for the first batch only)
        valid = ~g["b%d/padding_mask" % i]
        xs, pred = pnp.model_forward(g, i, P0)
        for l, x in enumerate(xs):
            want, got = pnp.stored(g, pre, "X%d" % l, x[valid])
            assert pnp.rel_err(got, want) <= pnp.bound_for(g, pre + "X%d" % l)[0], (case, i, l)
        assert pnp.rel_err(pred[valid], g[pre + "pred"][valid]) <= pnp.bound_for(g, pre + "pred")[0], (case, i)


@pytest.mark.parametrize("case", MODEL_CASES)
def test_collate_additions_equal_the_reference_golden_with_a_stub_ranker(case):
    g = load_golden(case)
    m = pnp.meta(g)
    u_v, i_v = pnp.ranker_vectors(g, 1)
    raw = np.where(np.isinf(g["b1/scores"]), 0.0, g["b1/scores"]).astype(np.float32)      # (what the mask hides is never looked at)
    model = _stub_model(m["P"], m["N"], {"prediction": torch.from_numpy(raw), "u_v": torch.from_numpy(u_v), "i_v": torch.from_numpy(i_v)})
    fd = model.add_ranker_outputs({k: torch.from_numpy(g["b1/" + k]) for k in ("user_id", "item_id", "pos_num", "neg_num")}, m["B"])
    valid = ~g["b1/padding_mask"]
    assert (fd["padding_mask"].numpy() == ~valid).all() and fd["batch_size"] == m["B"]
    assert (fd["scores"].numpy()[valid] == g["b1/scores"][valid]).all() and np.isinf(fd["scores"].numpy()[~valid]).all()
    position = fd["position"].numpy()
    assert (position[valid] == g["b1/position"][valid]).all()
    for b in range(m["B"]):
        assert sorted(position[b]) == list(range(m["P"] + m["N"]))
        assert sorted(g["b1/position"][b]) == list(range(m["P"] + m["N"]))


def _feed_dicts(g, i, seq):
    """batch i of a golden taken apart again into what Dataset._get_feed_dict hands to collate_batch: ragged lists, no padding"""
    m, pre = pnp.meta(g), "b%d/" % i
    feeds = []
    for b in range(m["B"]):
        p, k = int(g[pre + "pos_num"][b]), int(g[pre + "neg_num"][b])
        fd = {"user_id": int(g[pre + "user_id"][b]), "pos_items": g[pre + "item_id"][b, :p].copy(),
              "neg_items": g[pre + "item_id"][b, m["P"]:m["P"] + k].copy(), "pos_num": p, "neg_num": k}
        if seq:
            n, nn_ = int(g[pre + "lengths"][b]), int(g[pre + "neg_lengths"][b])
            fd.update(history_items=g[pre + "history_items"][b, :n].copy(), neg_history_items=g[pre + "neg_history_items"][b, :nn_].copy(),
                      history_times=g[pre + "history_times"][b, :n].copy(), neg_history_times=g[pre + "neg_history_times"][b, :nn_].copy(),
                      lengths=n, neg_lengths=nn_)
        feeds.append(fd)
    return feeds


def _stub_dataset(g, i, ranker_name="Stub", lightgcn=False):
    """the Dataset of the base the golden's class sits on, around a stub ranker that returns batch i's stored prediction and vectors
    and carries the fixture's item table where the sequential base looks for it"""
    from models.BaseRerankerModel import RerankModel, RerankSeqModel
    m = pnp.meta(g)
    base = RerankSeqModel if m["seq"] else RerankModel
    u_v, i_v = pnp.ranker_vectors(g, i)
    raw = np.where(np.isinf(g["b%d/scores" % i]), 0.0, g["b%d/scores" % i]).astype(np.float32)      # (what the mask hides is never looked at)
    model = base.__new__(base)
    torch.nn.Module.__init__(model)
    model.device, model.ranker_name = torch.device("cpu"), ranker_name
    model.train_max_pos_item, model.train_max_neg_item = m["P"], m["N"]
    model.ranker = _StubRanker({"prediction": torch.from_numpy(raw), "u_v": torch.from_numpy(u_v), "i_v": torch.from_numpy(i_v)})
    table = torch.from_numpy(g["R/i_embeddings.weight"])
    if lightgcn:      # LightGCNImpression keeps its tables in encoder.embedding_dict (reference BaseRerankerModel.py:126-127)
        model.ranker.encoder = SimpleNamespace(embedding_dict={"item_emb": table})
    else:
        model.ranker.i_embeddings = torch.nn.Embedding.from_pretrained(table)
    ds = base.Dataset.__new__(base.Dataset)
    ds.model, ds.corpus, ds.phase, ds.pos_len, ds.neg_len = model, SimpleNamespace(n_users=m["n_users"], n_items=m["n_items"]), "train", m["P"], m["N"]
    return ds


@pytest.mark.parametrize("case", MODEL_CASES)
def test_dataset_collate_batch_of_both_bases_equals_the_reference_golden(case):
    """RerankModel.Dataset.collate_batch (cases a, b, c) and RerankSeqModel.Dataset.collate_batch (case d) on the golden's own lists:
    the padded item lists, everything the ranker's run adds and, for the sequential base, his_v"""
    g = load_golden(case)
    m = pnp.meta(g)
    for i in ((1, 3) if not m["seq"] else (1,)):      # (the sequential ranker's vectors are stored for the first batch only)
        pre = "b%d/" % i
        fd = _stub_dataset(g, i).collate_batch(_feed_dicts(g, i, m["seq"]))
        valid = ~g[pre + "padding_mask"]
        assert fd["batch_size"] == m["B"] and fd["phase"] == "train"
        for k in ("user_id", "item_id", "pos_num", "neg_num") + (("history_items", "neg_history_items", "lengths") if m["seq"] else ()):
            assert fd[k].dtype == torch.int64 and (fd[k].numpy() == g[pre + k]).all(), (case, i, k)
        assert "pos_items" not in fd and (fd["padding_mask"].numpy() == ~valid).all()
        assert (fd["scores"].numpy()[valid] == g[pre + "scores"][valid]).all() and np.isinf(fd["scores"].numpy()[~valid]).all()
        position = fd["position"].numpy()
        assert (position[valid] == g[pre + "position"][valid]).all()
        for b in range(m["B"]):
            assert sorted(position[b]) == list(range(m["P"] + m["N"]))
        if i == 1:
            for k in ("u_v", "i_v") + (("his_v",) if m["seq"] else ()):
                want, got = pnp.stored(g, pre, k, fd[k].numpy())
                assert got.tobytes() == want.tobytes(), (case, k)
        assert ("his_v" in fd) == bool(m["seq"])
    if m["seq"]:
        assert g["b1/his_v"].shape == g["b1/history_items"].shape + (m["emb"],) and (g["b1/lengths"] < g["b1/history_items"].shape[1]).any()
        # a LightGCN ranker's item vectors come from its encoder's table, not from an i_embeddings module
        fd = _stub_dataset(g, 1, ranker_name="LightGCN", lightgcn=True).collate_batch(_feed_dicts(g, 1, True))
        assert fd["his_v"].numpy().tobytes() == g["b1/his_v"].tobytes()
