"""CPU: SLRC+'s host side -- the float64 restatement (tests/slrc_np.py) against the reference's own numbers
(tests/golden/slrc_*.npz, kg_reader.json, slrc_kg_dataset.npz, written by tests/golden/make_golden_slrc.py), KGReader, the model
file's class lookup, flags, state_dict keys and shape check, the Dataset's relational intervals, the pipeline's dataset kind, and
the C entry points' declarations and refusals.  No kernel runs.

Tolerances: the goldens are float32 results of the reference, the restatement is float64: conftest.assert_close at its default
1e-5 (relative to the entry plus 1e-5 of the tensor's largest entry).  One quantity has a floor, with the reason: the gradient of
user_bias is sum_c d loss / d pred[b, c], exactly 0 in exact arithmetic (the loss does not change when all scores of a tuple shift
together), so the reference's value is its own round-off; it is held below 1e-5 of the item_bias gradient's largest entry."""
import argparse
import ctypes as C
import json
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT, assert_close, assert_update_close, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import slrc_np  # noqa: E402
from slrc_data import make_kg_dataset  # noqa: E402
from slrc_np import PARAMS, STATE_KEYS  # noqa: E402

PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)

CASES = golden_cases("slrc_d")
KG_SEED, KG_TIME_SCALAR = 5, 100000      # tests/golden/make_golden_slrc.py's


def _args(**kw):
    a = dict(device="cpu", model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=64, history_max=20, time_scalar=8640000)
    a.update(kw)
    return SimpleNamespace(**a)


def _corpus(n_users=5, n_items=6, n_rel=2):
    return SimpleNamespace(n_users=n_users, n_items=n_items, item_relations=["r_%d" % k for k in range(n_rel)], triplet_set=set())


def test_golden_cases_exist_and_hold_the_hand_set_slots():
    assert tuple(CASES) == tuple(sorted(slrc_np.GOLDEN_CASES))
    shapes = set()
    for c in CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", c + ".npz")) < 512 << 10
        g = load_golden(c)
        n_users, n_items, d, R, B, K, seed, redraw = (int(x) for x in g["meta"])
        shapes.add((str(g["opt"]), d, R, B, K, float(g["hyper"][0]), float(g["hyper"][1])))
        iid, iv = g["iid"], g["intervals"]
        assert iid.shape == (B, 1 + K) and g["uid"].shape == (B,) and iv.shape == (B, 1 + K, R) and iv.dtype == np.float32
        assert iv[0, 0, 0] == 0.0 and (iv == -1).any() and ((iv > 0).any() or B == 1)   # an interval of exactly 0; masked and live entries
        if B > 1:
            assert len(np.unique(g["uid"])) < B and len(np.unique(iid)) < iid.size   # ids repeat
            assert (iv[B - 1] == -1).all()                                           # a tuple without any interval
            x = {0: g["betas0"], 3: g["sigmas0"]}
            kinds = {int(k): (int(i), int(r)) for i, r, k in g["special"]}
            assert sorted(kinds) == [0, 1, 2, 3, 4, 5]
            for base in (0, 3):                                                      # below 1e-10, exactly 10, above 10
                lo, mid, hi = (x[base][kinds[base + j]] + np.float32(1) for j in range(3))
                assert lo < 1e-10 and mid == 10.0 and hi > 10.0
                for j in range(3):
                    item, r = kinds[base + j]
                    assert ((iid == item) & (iv[:, :, r] >= 0)).any()                # the entry takes part in a score
        if K >= 2:
            assert iid[0, 1] == iid[0, 0] and iid[0, 2] == iid[0, 1]
        for k in PARAMS:
            assert np.isfinite(g["G" + k]).all() and np.isfinite(g[k + "1"]).all()
    assert shapes == {("SGD", 16, 1, 1, 1, 0.1, 1e-5), ("SGD", 32, 3, 160, 4, 0.5, 0.0), ("Adam", 64, 3, 77, 99, 5e-4, 1e-5),
                      ("Adagrad", 128, 8, 33, 9, 0.01, 1e-4)}


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference(case):
    g = load_golden(case)
    P = {k: g[k + "0"] for k in PARAMS}
    uid, iid, iv = g["uid"], g["iid"], g["intervals"]
    pred = slrc_np.scores(P, uid, iid, iv)
    assert_close(g["pred"], pred, what=case + " pred")
    loss_vec, gpred = slrc_np.bpr(pred)
    assert_close(float(g["loss"]), loss_vec.mean(), what=case + " loss")
    grads = slrc_np.dense_grads(P, uid, iid, iv, gpred)
    floor = 1e-5 * np.abs(grads["item_bias"]).max()
    for k in PARAMS:
        assert_close(g["G" + k], grads[k], what=f"{case} G{k}", abs_floor=floor if k == "user_bias" else 0.0)
    assert np.abs(g["Guser_bias"]).max() <= floor and np.abs(grads["user_bias"]).max() <= 1e-12
    # torch.optim's step is dense: weight decay reaches every row (the two bias tables take none)
    lr, l2 = (float(x) for x in g["hyper"])
    opt = str(g["opt"])
    for k in PARAMS:
        W0 = g[k + "0"].reshape(-1, 1) if k == "global_alpha" else g[k + "0"]
        # from the reference's own fp32 gradient: the step arithmetic is what is pinned here (the gradients were pinned above)
        W1, _, _ = slrc_np.optimizer_rows(W0, g["G" + k].reshape(W0.shape), np.arange(W0.shape[0]), opt, lr, 0.0 if "bias" in k else l2)
        assert_update_close(g[k + "1"].reshape(W0.shape), W0, W1, what=f"{case} {k} update", rtol=2e-5,
                            extra_atol=0.0 if opt == "SGD" else 1e-3 * lr, strict=True)


def test_restated_gradients_agree_with_autograd_in_float64():
    import torch
    rng = np.random.default_rng(7)
    n_users, n_items, d, R, B, Cn = 5, 9, 6, 3, 8, 5
    P = {"U": rng.normal(0, 0.5, (n_users, d)), "I": rng.normal(0, 0.5, (n_items, d)), "user_bias": rng.normal(0, 0.5, (n_users, 1)),
         "item_bias": rng.normal(0, 0.5, (n_items, 1)), "global_alpha": np.array(0.3)}
    for k in slrc_np.HAWKES:
        P[k] = rng.normal(0, 0.4, (n_items, R))
    P["betas"][0, 0], P["betas"][1, 1], P["sigmas"][2, 0], P["sigmas"][3, 2] = -2.0, 9.5, -3.0, 12.0
    uid, iid = rng.integers(0, n_users, B), rng.integers(0, n_items, (B, Cn))
    iid[0, 1] = iid[0, 0]
    iid[1, :4] = [0, 1, 2, 3]
    iv = np.where(rng.random((B, Cn, R)) < 0.3, -1.0, rng.uniform(0, 3, (B, Cn, R)))
    iv[1] = 0.5
    T = {k: torch.tensor(P[k], requires_grad=True) for k in PARAMS}
    t_iv = torch.tensor(iv)
    mask = (t_iv >= 0).double()
    dt = t_iv * mask
    alphas = T["global_alpha"] + T["alphas"][iid]
    pis, mus = T["pis"][iid] + 0.5, T["mus"][iid] + 1
    betas, sigmas = (T["betas"][iid] + 1).clamp(min=1e-10, max=10), (T["sigmas"][iid] + 1).clamp(min=1e-10, max=10)
    e = torch.distributions.exponential.Exponential(betas, validate_args=False).log_prob(dt).exp()
    n = torch.distributions.normal.Normal(mus, sigmas).log_prob(dt).exp()
    pred = ((T["U"][uid][:, None, :] * T["I"][iid]).sum(-1) + T["user_bias"][uid] + T["item_bias"][iid].squeeze(-1)
            + (alphas * (pis * e + (1 - pis) * n) * mask).sum(-1))
    mine = slrc_np.scores(P, uid, iid, iv)
    assert np.abs(mine - pred.detach().numpy()).max() <= 1e-12
    w = rng.normal(0, 1, (B, Cn))                       # an arbitrary loss: the BPR loss leaves user_bias without a gradient
    (pred * torch.tensor(w)).sum().backward()
    G = slrc_np.dense_grads(P, uid, iid, iv, w)
    for k in PARAMS:
        assert np.abs(G[k] - T[k].grad.numpy()).max() <= 1e-11, k
    ugrad, ubgrad, hgrad, gagrad = slrc_np.front_grads(P, uid, iid, iv, w)
    assert hgrad.shape == (B * Cn, 5 * R) and abs(gagrad.sum() - G["global_alpha"]) <= 1e-11 and ubgrad.shape == (B,)
    for j, k in enumerate(slrc_np.HAWKES):
        acc = np.zeros_like(P[k])
        np.add.at(acc, iid.reshape(-1), hgrad[:, j * R:(j + 1) * R])
        assert np.abs(acc - G[k]).max() <= 1e-11, k


# ---- KGReader and the Dataset against the recorded reference -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kg_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("slrc_kg"))
    make_kg_dataset(root, "synth_kg", seed=KG_SEED)
    return root


def _reader(kg_root, include_attr):
    from helpers.KGReader import KGReader
    a, _ = KGReader.parse_data_args(argparse.ArgumentParser()).parse_known_args(
        ["--path", kg_root + "/", "--dataset", "synth_kg", "--include_attr", str(include_attr)])
    return KGReader(a)


def _plain(x):
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x.item() if isinstance(x, np.generic) else x


@pytest.mark.parametrize("include_attr", [0, 1])
def test_kg_reader_equals_the_recorded_reference(include_attr, kg_root):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "kg_reader.json")))["include_attr_%d" % include_attr]
    corpus = _reader(kg_root, include_attr)
    assert corpus.include_attr == include_attr
    assert corpus.item_relations == want["item_relations"] == ["r_complement", "r_substitute"]
    assert corpus.attr_relations == want["attr_relations"] == (["i_category"] if include_attr else [])
    assert corpus.relations == want["relations"]
    assert (int(corpus.n_relations), int(corpus.n_entities), corpus.n_users, corpus.n_items) == (
        want["n_relations"], want["n_entities"], want["n_users"], want["n_items"])
    assert list(corpus.relation_df.columns) == ["head", "relation", "tail"]
    assert _plain(corpus.relation_df.values.tolist()) == want["relation_df"]          # emission order included
    assert sorted(_plain(list(t)) for t in corpus.triplet_set) == want["triplet_set"]
    assert list(corpus.item_meta_df.columns) == want["item_meta_columns"]
    assert _plain(corpus.item_meta_df.values.tolist()) == want["item_meta_rows"]      # the list columns are lists
    if include_attr:
        assert _plain(list(corpus.attr_max)) == want["attr_max"]
        assert {str(k): _plain(v) for k, v in corpus.share_attr_dict.items()} == want["share_attr_dict"]
        assert any(t[1] == 3 and t[2] >= corpus.n_items for t in corpus.triplet_set)
    else:
        assert not hasattr(corpus, "share_attr_dict")
    assert {t[1] for t in corpus.triplet_set} >= {1, 2}


def test_dataset_relational_intervals_equal_the_recorded_reference(kg_root):
    from models.sequential.SLRCPlus import SLRCPlus
    g = load_golden("slrc_kg_dataset")
    corpus = _reader(kg_root, 0)
    model = SimpleNamespace(test_all=0, buffer=0, history_max=int(g["history_max"]), num_neg=3, relation_num=3,
                            time_scalar=int(g["time_scalar"]))
    train = SLRCPlus.Dataset(model, corpus, "train")
    assert len(train) == g["train_intervals"].shape[0]
    train.data["neg_items"] = g["train_neg_items"]
    feeds = [train[k] for k in range(len(train))]
    assert sorted(feeds[0]) == ["history_items", "history_times", "item_id", "lengths", "relational_interval", "user_id"]
    got = np.stack([f["relational_interval"] for f in feeds])
    assert got.dtype == np.float32 and got.shape == (len(train), 4, 3)
    assert np.array_equal(np.stack([f["item_id"] for f in feeds]), g["train_item_id"])
    assert np.array_equal(got, g["train_intervals"])                                  # bit for bit: float64 division, then the cast
    for r in range(3):                                                                # every relation occurs, and so does "none"
        assert (got[:, :, r] >= 0).any() and (got[:, :, r] == -1).any()
    dev = SLRCPlus.Dataset(model, corpus, "dev")
    n = g["dev_intervals"].shape[0]
    feeds = [dev[k] for k in range(n)]
    assert np.array_equal(np.stack([f["item_id"] for f in feeds]), g["dev_item_id"])
    assert np.array_equal(np.stack([f["relational_interval"] for f in feeds]), g["dev_intervals"])
    # --test_all: one interval row per catalogue item
    model.test_all = 1
    f = SLRCPlus.Dataset(model, corpus, "test")[0]
    assert f["relational_interval"].shape == (corpus.n_items, 3)
    batch = dev.collate_batch(feeds[:3])
    assert tuple(batch["relational_interval"].shape) == (3, g["dev_item_id"].shape[1], 3)


# ---- the model file ----------------------------------------------------------------------------------------------------------------

def test_class_lookup_flags_and_log_args():
    import main
    cls = main.find_class("model", ("SLRCPlus", ""))
    assert cls.__name__ == "SLRCPlus" and cls.reader == "KGReader" and cls.runner == "BaseRunner"
    assert cls.extra_log_args == ["emb_size"]
    assert cls.candidate_permutation_equivariant is True
    assert hasattr(cls, "hip_train_step") and hasattr(cls, "hip_rowwise_supported") and not hasattr(cls, "full_catalogue_vectors")
    d, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
    assert (d.emb_size, d.time_scalar, d.history_max, d.num_neg, d.test_all) == (64, 8640000, 20, 1, 0)
    reader = main.find_class("helper", cls.reader)
    assert reader.__name__ == "KGReader"
    r, _ = reader.parse_data_args(argparse.ArgumentParser()).parse_known_args([])
    assert r.include_attr == 0


def _added_flags(add):
    p = argparse.ArgumentParser()
    before = {s for a in p._actions for s in a.option_strings}
    p = add(p)
    return sorted({s for a in p._actions for s in a.option_strings} - before)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_and_flags_equal_the_recorded_reference(case):
    from helpers.KGReader import KGReader
    from models.sequential.SLRCPlus import SLRCPlus
    g = load_golden(case)
    n_users, n_items, d, R = (int(x) for x in g["meta"][:4])
    m = SLRCPlus(_args(emb_size=d), _corpus(n_users, n_items, R - 1))
    assert m.relation_num == R
    assert sorted(m.state_dict().keys()) == sorted(g["state_keys"].tolist()) == sorted(STATE_KEYS.values())
    for k in PARAMS:
        assert tuple(m.state_dict()[STATE_KEYS[k]].shape) == g[k + "0"].shape, k
    assert m.global_alpha.dim() == 0 and float(m.global_alpha.detach()) == 0.0
    assert 0.005 < float(m.i_embeddings.weight.detach().std()) < 0.02          # BaseModel.init_weights: N(0, 0.01)
    # a state_dict in the reference's layout loads, and the reverse: the recorded tensors under the recorded keys
    import torch
    m.load_state_dict({STATE_KEYS[k]: torch.from_numpy(g[k + "1"]) for k in PARAMS})
    assert np.array_equal(m.state_dict()["betas.weight"].numpy(), g["betas1"])
    # weight decay: 'bias' parameters take none, everything else -- global_alpha included -- does
    decay, no_decay = m.customize_parameters()
    assert no_decay["weight_decay"] == 0 and {id(p) for p in no_decay["params"]} == {id(m.user_bias.weight), id(m.item_bias.weight)}
    assert any(p is m.global_alpha for p in decay["params"]) and len(decay["params"]) == 8
    assert _added_flags(SLRCPlus.parse_model_args) == g["model_flags"].tolist()
    assert {"--emb_size", "--time_scalar", "--history_max"} <= set(g["model_flags"].tolist())
    assert _added_flags(KGReader.parse_data_args) == g["reader_flags"].tolist() and "--include_attr" in g["reader_flags"].tolist()


def test_unsupported_shapes_are_refused_at_construction_with_the_flag_named():
    from models.sequential.SLRCPlus import SLRCPlus
    with pytest.raises(ValueError, match=r"--emb_size 48.*16, 32, 64, 128"):
        SLRCPlus(_args(emb_size=48), _corpus())
    with pytest.raises(ValueError, match=r"8 item relations.*R=9 outside 1\.\.8"):
        SLRCPlus(_args(emb_size=16), _corpus(n_rel=8))
    m = SLRCPlus(_args(emb_size=16), _corpus(n_rel=7))
    assert m.hip_rowwise_supported() and m.relation_num == 8


def test_dataset_kind_is_none():
    from models.sequential.SLRCPlus import SLRCPlus
    from rechorus_amd import pipeline
    assert pipeline.dataset_kind(object.__new__(SLRCPlus.Dataset)) is None      # the DataLoader path: the intervals are built on the host


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_lib_signatures_and_header_agree_on_every_slrc_symbol():
    from rechorus_amd import _lib
    header = open(os.path.join(ROOT, "include", "rechorus_hip.h")).read()
    protos = dict((m.group(2), (m.group(1), m.group(3))) for m in
                  re.finditer(r"^(enum rc_status|size_t) (rc_slrc_\w+)\(([^;]*)\);", header, re.M | re.S))
    want = {"rc_slrc_check_shape", "rc_slrc_fwd_bwd_layout", "rc_slrc_scores", "rc_slrc_fwd_bwd", "rc_slrc_excitation_bwd",
            "rc_slrc_item_update_workspace_bytes", "rc_slrc_item_update", "rc_slrc_user_bias_update"}
    assert set(protos) == want == {k for k in _lib.SIGNATURES if k.startswith("rc_slrc_")}
    lib = _lib.load()
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert hasattr(lib, name), name
        assert (restype is C.c_size_t) == (ret == "size_t"), name
        kinds = []
        for p in (q.strip() for q in params.split(",")):
            if "*" in p or p.startswith("rc_stream_t"):
                kinds.append("rc_opt_hyper" in p and "hyper" or "ptr")
            else:
                kinds.append({"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "size_t": C.c_size_t}[p.rsplit(" ", 1)[0]])
        got = ["hyper" if t is _lib._hp else ("ptr" if t is C.c_void_p else t) for t in argtypes]
        assert got == kinds, name


def test_entry_points_refuse_bad_calls_without_a_gpu():
    from rechorus_amd import _lib
    lib = _lib.load()
    p, q = C.c_void_p(256), C.c_void_p(512)      # non-null, aligned; never dereferenced
    INVALID = -1
    err = lambda: lib.rc_last_error_string()
    assert lib.rc_slrc_check_shape(64, 100, 3) == 0 and lib.rc_slrc_check_shape(16, 1, 1) == 0 and lib.rc_slrc_check_shape(128, 1, 8) == 0
    assert lib.rc_slrc_check_shape(48, 100, 3) == INVALID and b"d=48" in err() and err().startswith(b"rc_slrc_check_shape:")
    assert lib.rc_slrc_check_shape(64, 0, 3) == INVALID and b"C >= 1" in err()
    assert lib.rc_slrc_check_shape(64, 5, 0) == INVALID and b"R=0 outside 1..8" in err()
    assert lib.rc_slrc_check_shape(64, 5, 9) == INVALID and b"R=9 outside 1..8" in err()

    def scores(U=p, pred=p, d=64, Cn=1, R=3):
        return lib.rc_slrc_scores(U, *([p] * 12), 4, Cn, d, R, pred, None)
    assert scores(U=None) == INVALID and err().startswith(b"rc_slrc_scores: null pointer")
    assert scores(pred=None) == INVALID and b"null pointer" in err()
    assert scores(d=48) == INVALID and b"d=48" in err()
    assert scores(Cn=0) == INVALID and b"C >= 1" in err()
    assert scores(R=9) == INVALID and b"R=9" in err()

    def fwd_bwd(U=p, gagrad=p, d=64, Cn=2, R=3):
        return lib.rc_slrc_fwd_bwd(U, *([p] * 12), 4, Cn, d, R, 0.25, None, p, p, p, p, p, gagrad, None)
    assert fwd_bwd(U=None) == INVALID and err().startswith(b"rc_slrc_fwd_bwd: null pointer")
    assert fwd_bwd(gagrad=None) == INVALID and b"null pointer" in err()
    assert fwd_bwd(d=48) == INVALID and b"d=48" in err()
    assert fwd_bwd(Cn=1) == INVALID and b"C >= 2" in err()
    assert fwd_bwd(R=0) == INVALID and b"R=0" in err()
    assert lib.rc_slrc_excitation_bwd(*([p] * 9), 4, 5, 3, p, p, None, None) == INVALID and b"null pointer" in err()
    assert lib.rc_slrc_excitation_bwd(*([p] * 9), 4, 5, 9, p, p, p, None) == INVALID and b"R=9" in err()

    h = C.byref(_lib.OptHyper(opt=_lib.RC_OPT_SGD, lr=0.1))
    adam = C.byref(_lib.OptHyper(opt=_lib.RC_OPT_ADAM, lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, step=1))
    seven = lambda *xs: (C.c_void_p * 7)(*xs)
    tables = seven(*(256 * k for k in range(2, 9)))

    def upd(W=tables, U=p, d=64, R=3, dense=None, heads=p, hyper=h, ws_bytes=0):
        return lib.rc_slrc_item_update(W, None, None, d, R, p, p, 100, p, p, U, p, 4, hyper, dense, heads, heads, p, ws_bytes, None)
    # everything that inspects only the arguments comes before the workspace-size check: ws_bytes = 0, so a lost check would end
    # in RC_ERR_WORKSPACE, not in a launch on the made-up pointers
    assert upd(dense=seven(256, 512, 768, None, 1280, 1536, 1792)) == INVALID and b"all seven dense gradients or none (got 6)" in err()
    assert upd(U=None) == INVALID and err().startswith(b"rc_slrc_item_update: null pointer")
    assert upd(heads=None) == INVALID and b"head list" in err()
    assert upd(W=None) == INVALID and b"no output" in err()
    assert upd(W=seven(512, 768, None, 1280, 1536, 1792, 2048)) == INVALID and b"table 2 of seven is null" in err()
    assert upd(d=48) == INVALID and b"d=48" in err()
    assert upd(R=9) == INVALID and b"R=9" in err()
    assert upd(U=C.c_void_p(768)) == INVALID and b"distinct" in err()
    assert upd(hyper=None) == INVALID and b"hyper-parameters missing" in err()
    assert upd(hyper=adam) == INVALID and b"Adam needs m and v" in err()
    assert upd() == -2 and b"workspace 0 <" in err()
    assert upd(dense=tables, W=None) == -2 and b"workspace 0 <" in err()
    sizes = [lib.rc_slrc_item_update_workspace_bytes(n, 64) for n in (0, 1, 32, 33, 100, 1000, 8320, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] == sizes[1] and sizes[-1] > sizes[1]             # monotone in n_occ
    assert sizes[4] >= 256 + 4 * (100 // 33 + 1)

    def ubias(W=p, keys=p, hyper=h, dense=None):
        return lib.rc_slrc_user_bias_update(W, None, None, keys, p, 10, p, hyper, dense, None)
    assert ubias(keys=None) == INVALID and err().startswith(b"rc_slrc_user_bias_update: null pointer")
    assert ubias(W=None) == INVALID and b"no output" in err()
    assert ubias(hyper=None) == INVALID and b"hyper-parameters missing" in err()
    assert ubias(hyper=adam) == INVALID and b"Adam needs m and v" in err()


def test_fwd_bwd_layout_envelope():
    """the register path's envelope as the dispatcher reports it (host logic): C <= 400 / 200 / 100 / 50 at d = 16 / 32 / 64 / 128,
    streaming beyond; d = 64 with C = 100, the benchmark shape, holds 25 rows per lane-group in registers"""
    from rechorus_amd import engine
    assert engine.slrc_fwd_bwd_layout(64, 100, 3) == 25
    for d, top in ((16, 400), (32, 200), (64, 100), (128, 50)):
        assert engine.slrc_fwd_bwd_layout(d, top, 1) is not None and engine.slrc_fwd_bwd_layout(d, top + 1, 1) is None
        assert engine.slrc_fwd_bwd_layout(d, 2, 8) is not None and engine.slrc_fwd_bwd_layout(d, 1, 8) is None
        for Cn in range(2, top + 1):
            cpl = engine.slrc_fwd_bwd_layout(d, Cn, 3)
            assert cpl in (1, 2, 4, 8, 13, 25) and cpl * (256 // d) >= Cn
    assert engine.slrc_fwd_bwd_layout(48, 10, 3) is None and engine.slrc_fwd_bwd_layout(64, 10, 9) is None


def test_slrc_kernels_use_no_float_atomics():
    src = open(os.path.join(ROOT, "rechorus_amd", "csrc", "slrc.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    atomics = re.findall(r"atomic\w*\s*\([^;]*;", code)
    assert len(atomics) == 1 and "a.n_long, 1u" in atomics[0]        # the one integer ticket of the long-row list
    assert not re.search(r"__hip_atomic|__atomic_fetch", code)
