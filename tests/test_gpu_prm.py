"""GPU: the list encoder block on the HIP engine (rc_listenc_block_fwd / _bwd) against the float64 restatement (tests/prm_np.py) on
the grid of list lengths, shapes and batch sizes of prm_np.LAYER_PROBLEMS: every n in {1, 2, 15, 16, 17, 40, 64} at (d, H, d_ff) =
(64, 4, 128) with 65 lists, every shape at n = 17 with 3 and 257 lists (the backward launches at most 256 workgroups, one list per
pass: with 257 lists one workgroup walks a second list), and one list alone.  The four mask kinds (random, one valid slot, all
valid, [valid | pad | valid | pad]) take turns over the lists of every problem; dY is non-zero on padded slots.  The forward is
compared on every slot, dX and all twelve weight and bias gradients each against its own reference.

Tolerances: the project's rule, nothing new -- each comparison is held to the larger of 2e-5 and 4 x the stored deviation of torch's
own fp32 nn.TransformerEncoderLayer from float64 for that tensor (tests/golden/prm_layer_dev.npz, written by
tests/golden/make_golden_prm.py; the problems are regenerated from their seeds), as largest |difference| / largest |reference entry|.
No bound is computed at test time.  Each comparison prints its bound and the error it saw (PRM_TOL lines, run with -s;
tools/prm_tolerance_report.py folds that output into profiles/prm_tolerances.txt).

The model classes: the four goldens of tests/golden/make_golden_prm.py (the reference's own PRM on CPU) -- init stream, collated batch
(ranks on valid slots; a padded slot's rank is the sort's choice among ties, so block outputs and predictions are compared on valid
slots), every block's output, prediction, loss, every gradient, two optimizer steps; both classes through main.run.  Gradients,
updated parameters and block outputs above 2,048 elements are stored as every fifth element (flat; prm_np.keep / prm_np.stored, as the
DCNv2 goldens do above their limit): of i_embeddings, in_proj, out_proj, linear1 and linear2 in cases a, c and d the model tests see a
fifth; the block grid above compares every element of every gradient.  The two largest goldens are 0.5 and 0.6 MB.

The golden cases are conditioned so that the reference's own fp32 run meets the two-step update check against its own float64 run
with twice its deviation (asserted by the generator; its header says what decides that: the candidates' vectors must outweigh what
the rows of a list share, and the learning rates are a tenth of the usual ones).  The key-bias third of every in_proj_bias has a
gradient that is exactly zero in exact arithmetic: like the zero_grad_keys it is held by the size of its move only."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import assert_update_close, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
PLUGIN = os.path.join(os.path.dirname(HERE), "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)
import prm_np as pnp  # noqa: E402
from prm_np import GRAD_NAMES, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEVS = load_golden("prm_layer_dev")


def _check(got, want, what, bound, why):
    if torch.is_tensor(got):
        got = got.detach().cpu().numpy()
    err = rel_err(np.asarray(got).reshape(np.shape(want)), want)
    print(f"PRM_TOL {what}: {err:.3e} (allowed {bound:.3g}: {why})")
    assert err <= bound, f"{what}: largest error / largest entry {err:.3e} > {bound:g}"


@functools.lru_cache(maxsize=None)
def _reference(prob_id):
    """(problem, Y, gradients) in float64, computed once per problem and shared (never written to)"""
    prob = pnp.random_block(*prob_id)
    X, pad, W, dY = prob
    return prob, pnp.block_forward(X, pad, W, prob_id[3]), pnp.block_backward(dY, X, pad, W, prob_id[3])


def _run_block(prob, H, cuda, workspace=None):
    from rechorus_amd import engine
    X, pad, W, dY = prob
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (X, pad, *W, dY)]
    Y = engine.listenc_block_fwd(t[0], t[1], t[2:14], H)
    dX, grads = engine.listenc_block_bwd(t[14], t[0], t[1], t[2:14], H, workspace=workspace)
    return t, Y, [dX] + list(grads)


def _check_block(prob_id, cuda, workspace=None):
    B, n, d, H, dff, _ = prob_id
    key, what = pnp.layer_key(*prob_id), f"B={B} n={n} d={d} H={H} d_ff={dff}"
    prob, Y64, G64 = _reference(prob_id)
    _, Y, grads = _run_block(prob, H, cuda, workspace)
    _check(Y, Y64, what + " Y", *pnp.stored_bound(DEVS, key + "/Y"))                 # every slot, padded ones too
    for name, got in zip(GRAD_NAMES, grads):
        _check(got, G64[name], f"{what} {name}", *pnp.stored_bound(DEVS, f"{key}/{name}"))
    return prob, Y, grads


def _problems(pick):
    found = [p for p in pnp.LAYER_PROBLEMS if pick(p)]
    assert found
    return found


@pytest.mark.parametrize("n", pnp.LENGTHS)
def test_block_at_every_list_length(n, cuda):
    (p,) = _problems(lambda p: p[:5] == (65, n, 64, 4, 128))
    prob, _, grads = _check_block(p, cuda)
    kinds = {pnp.MASKS[(b + p[5]) % 4] for b in range(65)}
    assert kinds == set(pnp.MASKS)
    if n == 1:
        # one key: the softmax is identically 1 and no gradient reaches q or k -- exact zeros, in the reference as well
        d = 64
        assert (grads[1][:2 * d] == 0).all() and (grads[2][:2 * d] == 0).all()
        assert (_reference(p)[2]["dWin"][:2 * d] == 0).all()
        assert not (grads[1][2 * d:] == 0).all()
    else:
        assert prob[1].sum() > 0 and (prob[1].sum(1) == n - 1).any() and (prob[1].sum(1) == 0).any()
        assert np.abs(prob[3][prob[1] == 1]).min() > 0                       # dY on padded slots


@pytest.mark.parametrize("d,H,dff", pnp.SHAPES)
def test_block_at_every_shape_with_few_lists_and_with_more_lists_than_workgroups(d, H, dff, cuda):
    from rechorus_amd import engine
    ws = engine.ListEncWorkspace()
    probs = _problems(lambda p: p[1:5] == (17, d, H, dff) and p[0] in (3, 257))
    assert [p[0] for p in probs] == [3, 257]
    for p in probs:
        _check_block(p, cuda, ws)


def test_one_list_alone(cuda):
    _check_block(_problems(lambda p: p[0] == 1)[0], cuda)


def test_reruns_are_bit_identical_and_a_reused_workspace_changes_nothing(cuda):
    from rechorus_amd import engine
    big = _problems(lambda p: p[:5] == (257, 17, 64, 4, 128))[0]
    for p in (big, _problems(lambda p: p[:5] == (3, 17, 32, 2, 128))[0], _problems(lambda p: p[:5] == (65, 40, 64, 4, 128))[0]):
        prob = _reference(p)[0]
        runs = []
        for _ in range(2):
            t, Y, grads = _run_block(prob, p[3], cuda)
            runs.append([x.cpu().numpy().copy() for x in [Y] + grads])
            for a, b in zip(t, (prob[0], prob[1], *prob[2], prob[3])):      # the inputs stay as they were
                assert a.cpu().numpy().tobytes() == b.tobytes(), p
        for a, b in zip(*runs):
            assert a.tobytes() == b.tobytes(), p
    # a workspace that served a larger problem of the same shape first (257 lists, then 3): the results equal those of a fresh
    # workspace bit for bit
    used = engine.ListEncWorkspace()
    _run_block(_reference(big)[0], 4, cuda, used)
    small = _problems(lambda p: p[:5] == (3, 17, 64, 4, 128))[0]
    _, _, fresh = _run_block(_reference(small)[0], 4, cuda, engine.ListEncWorkspace())
    for _ in range(2):
        _, _, again = _run_block(_reference(small)[0], 4, cuda, used)
        for a, b in zip(fresh, again):
            assert torch.equal(a, b)
    assert len(used._bufs) == 2


@pytest.mark.parametrize("d,H,dff", [(64, 4, 128), (32, 2, 128)])
def test_a_lists_rows_do_not_depend_on_what_else_its_workgroup_walks(d, H, dff, cuda):
    """700 lists on 256 workgroups (up to three lists each) against the same lists in four batches of 175 (one list per workgroup):
    Y and dX bit for bit -- nothing of a list outlives it in the workgroup's LDS or registers -- and the weight gradients, whose sums
    only change their order, to the cap"""
    B, n = 700, 40
    prob = pnp.random_block(B, n, d, H, dff, seed=77)
    _, Y, grads = _run_block(prob, H, cuda)
    parts = [_run_block((prob[0][s:s + 175], prob[1][s:s + 175], prob[2], prob[3][s:s + 175]), H, cuda)[1:] for s in range(0, B, 175)]
    assert torch.equal(Y, torch.cat([y for y, _ in parts])) and torch.equal(grads[0], torch.cat([g[0] for _, g in parts]))
    for k, name in enumerate(GRAD_NAMES[1:], 1):
        want = sum(g[k].double() for _, g in parts).cpu().numpy()
        _check(grads[k], want, f"700 lists against 4 x 175, d={d} {name}", pnp.TOL, "the cap")


def test_autograd_node_and_evaluation_form(cuda):
    from rechorus_amd import nn as hnn
    p = _problems(lambda p: p[:5] == (3, 17, 32, 2, 128))[0]
    prob, Y64, G64 = _reference(p)
    X, pad, W, dY = (prob[0], prob[1], prob[2], prob[3])
    x = torch.from_numpy(X).to(cuda).requires_grad_(True)
    w = [torch.from_numpy(a).to(cuda).requires_grad_(True) for a in W]
    mask = torch.from_numpy(pad.astype(bool)).to(cuda)
    y = hnn.list_encoder_block(x, mask, w, p[3])
    y.backward(torch.from_numpy(dY).to(cuda))
    key = pnp.layer_key(*p)
    _check(y, Y64, "node Y", *pnp.stored_bound(DEVS, key + "/Y"))
    for name, t in zip(GRAD_NAMES, [x] + w):
        _check(t.grad, G64[name], "node " + name, *pnp.stored_bound(DEVS, f"{key}/{name}"))
    with pytest.raises(RuntimeError, match="no backward"):
        hnn.list_encoder_block_eval(x, mask, w, p[3])
    with torch.no_grad():
        ev = hnn.list_encoder_block_eval(x, mask, w, p[3])
    assert not ev.requires_grad and torch.equal(ev, y.detach())


def test_shapes_outside_the_envelope_are_refused_with_the_reason(cuda):
    from rechorus_amd import _lib, engine
    for n, d, H, dff, text in ((0, 64, 4, 128, "outside the envelope"), (65, 64, 4, 128, "outside the envelope"),
                               (40, 24, 2, 128, "outside the envelope"), (40, 64, 3, 128, "outside the envelope"),
                               (40, 64, 32, 128, "outside the envelope"), (40, 64, 4, 120, "outside the envelope"),
                               (40, 64, 4, 272, "outside the envelope"), (64, 128, 4, 256, "bytes of LDS")):
        with pytest.raises(ValueError, match=text):
            engine.listenc_check_shape(n, d, H, dff)
        assert _lib.load().rc_listenc_block_bwd_workspace_bytes(8, n, d, H, dff) == 0
    engine.listenc_check_shape(64, 64, 4, 128)
    engine.listenc_check_shape(32, 128, 4, 256)
    X = torch.zeros(2, 40, 24, device=cuda)
    with pytest.raises(ValueError, match="outside the envelope"):
        engine.listenc_block_fwd(X, torch.zeros(2, 40, dtype=torch.uint8, device=cuda),
                                 [torch.zeros(s, device=cuda) for s in ((72, 24), (72,), (24, 24), (24,), (24,), (24,), (16, 24), (16,),
                                                                        (24, 16), (24,), (24,), (24,))], 2)


# ---- the model classes against the reference's goldens --------------------------------------------------------------------------------
MODEL_CASES = [c for c in golden_cases("prm_") if c != "prm_layer_dev"]


def _collated(model, g, i, cuda):
    """batch i through the port's collate additions, held to the golden's: mask, masked scores, ranks, the ranker's vectors"""
    m = pnp.meta(g)
    fd = model.add_ranker_outputs(pnp.raw_batch(g, i, cuda), m["B"])
    pre, valid = "b%d/" % i, ~g["b%d/padding_mask" % i]
    assert (fd["padding_mask"].cpu().numpy() == ~valid).all()
    position = fd["position"].cpu().numpy()
    assert (position[valid] == g[pre + "position"][valid]).all()
    for b in range(m["B"]):
        assert sorted(position[b]) == list(range(m["P"] + m["N"]))
    scores = fd["scores"].cpu().numpy()
    assert np.isinf(scores[~valid]).all()
    _check(scores[valid], g[pre + "scores"][valid], f"batch {i} scores", pnp.TOL, "the cap")
    for k in ("u_v", "i_v"):
        if pre + k in g:
            want, got = pnp.stored(g, pre, k, fd[k].cpu().numpy())
            _check(got, want, f"batch {i} {k}", pnp.TOL, "the cap")
    return fd, valid


@pytest.mark.parametrize("case", MODEL_CASES)
def test_model_matches_the_reference_golden(case, cuda, tmp_path, monkeypatch):
    from helpers.ImpressionRunner import ImpressionRunner
    g = load_golden(case)
    m = pnp.meta(g)
    monkeypatch.chdir(tmp_path)
    model, _ = pnp.golden_model(g, cuda, tmp_path)      # asserts the init stream and the ranker's weights
    model.train()
    assert len(MODEL_CASES) == 4 and all(float(x) > 2.0 for x in g["maxp"] if x > 0)
    fd3, valid3 = _collated(model, g, 3, cuda)              # the forward-only batch: holds the list with a single valid slot
    assert m["B"] == 1 or (valid3.sum(1) == 1).any()
    with torch.no_grad():
        xs = model.encode(fd3)[1:]
        pred3 = model(fd3)["prediction"].cpu().numpy()
    for l, x in enumerate(xs):
        want, got = pnp.stored(g, "F/", "X%d" % l, x.cpu().numpy()[valid3])      # (a padded slot's rank is the sort's choice)
        _check(got, want, f"{case} forward-only X{l}", *pnp.bound_for(g, "F/X%d" % l))
    _check(pred3[valid3], g["F/pred"][valid3], case + " forward-only pred", *pnp.bound_for(g, "F/pred"))
    fd, valid = _collated(model, g, 1, cuda)
    assert valid[0].all() and (m["B"] < 3 or not valid[2, m["P"] - 1])      # all valid; padding inside the positives
    for l, x in enumerate(model.encode(fd)[1:]):
        want, got = pnp.stored(g, "", "X%d" % l, x.detach().cpu().numpy()[valid])
        _check(got, want, f"{case} X{l}", *pnp.bound_for(g, "X%d" % l))
    out = model(fd)
    loss = model.loss(out, ImpressionRunner._labels(fd, m["P"] + m["N"], m["P"], cuda))
    loss.backward()
    torch.cuda.synchronize()
    _check(out["prediction"].detach().cpu().numpy()[valid], g["pred"][valid], case + " pred", *pnp.bound_for(g, "pred"))
    _check(np.array([loss.item()]), np.array([float(g["loss"])]), case + " loss", *pnp.bound_for(g, "loss"))
    zero, floor = set(str(k) for k in g["zero_grad_keys"]), pnp.grad_floor(g)
    grads = {k: p.grad for k, p in model.named_parameters() if p.requires_grad}
    assert all(v is not None for v in grads.values()) and sorted(grads) == sorted(k[2:] for k in g if k.startswith("G/"))
    for k, got in grads.items():
        want, got = pnp.stored(g, "G/", k, got.cpu().numpy())
        if k in zero:
            assert float(np.abs(got).max()) <= 1e-5 * 1e6 * floor, (case, k)
            continue
        bound, why = pnp.bound_for(g, "G/" + k)
        err = rel_err(got, want, floor)
        print(f"PRM_TOL {case} grad {k}: {err:.3e} (allowed {bound:.3g}: {why})")
        assert err <= bound, f"{case} grad {k}: {err:.3e} > {bound:g}"
    assert all(p.grad is None for p in model.ranker.parameters())


@pytest.mark.parametrize("case", MODEL_CASES)
def test_two_optimizer_steps_match_the_reference_golden(case, cuda, tmp_path, monkeypatch):
    import argparse
    from helpers.BaseRunner import BaseRunner
    from helpers.ImpressionRunner import ImpressionRunner
    g = load_golden(case)
    m = pnp.meta(g)
    opt = [k[:-6] for k in g if k.endswith("_hyper")][0]
    lr, l2 = (float(x) for x in g[opt + "_hyper"])
    monkeypatch.chdir(tmp_path)
    model, P0 = pnp.golden_model(g, cuda, tmp_path)
    model.train()
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.optimizer, a.lr, a.l2, a.train, a.log_file = opt, lr, l2, 1, str(tmp_path / "log.txt")
    model.optimizer = BaseRunner(a)._build_optimizer(model)
    losses = []
    for i in (1, 2):
        fd = model.add_ranker_outputs(pnp.raw_batch(g, i, cuda), m["B"])
        model.optimizer.zero_grad()
        ls = model.loss(model(fd), ImpressionRunner._labels(fd, m["P"] + m["N"], m["P"], cuda))
        ls.backward()
        model.optimizer.step()
        losses.append(ls.item())
    torch.cuda.synchronize()
    print(f"PRM_LOSSES {case} {opt}: {losses} (reference {g[opt + '_losses'].tolist()})")
    np.testing.assert_allclose(losses, g[opt + "_losses"], rtol=pnp.TOL)
    zero, adaptive = set(str(k) for k in g["zero_grad_keys"]), opt in ("Adam", "Adagrad")
    for k, v in model.state_dict().items():
        if k.startswith("ranker."):
            assert v.cpu().numpy().tobytes() == P0[k].tobytes(), k      # frozen
            continue
        want, got = pnp.stored(g, opt + "/", k, v.cpu().numpy())
        start = pnp.stored(g, opt + "/", k, P0[k])[1]
        if k in zero:
            # the gradient is round-off around an exact zero: Adam / Adagrad normalise it to a step of about lr in a direction the
            # round-off decides, in the reference as well -- only the size of the move is held
            assert float(np.abs(got - start).max()) <= (2.5 * lr if adaptive else 1e-5) + 1e-7, (case, k)
            continue
        exclude = None
        if k.endswith("in_proj_bias"):
            # the key bias shifts every score of a query row alike and the softmax does not see it: its gradient (the middle third) is
            # exactly zero in exact arithmetic and round-off in every precision, like the zero_grad_keys -- only the size of the move
            d = got.shape[0] // 3
            exclude = np.zeros(got.shape, dtype=bool)
            exclude[d:2 * d] = True
            assert float(np.abs(got - start)[exclude].max()) <= (2.5 * lr if adaptive else 1e-5) + 1e-7, (case, k)
        assert_update_close(got, start, want, what=f"{case} {opt} {k}", extra_atol=1e-3 * lr if adaptive else 0.0,
                            outlier_atol=2 * lr if adaptive else 0.0, exclude=exclude)


# ---- the model classes through the CLI ------------------------------------------------------------------------------------------------
COMMON = ["--lr", "3e-3", "--l2", "0", "--loss_n", "BPR", "--dataset", "imp", "--epoch", "1", "--batch_size", "64", "--num_workers", "0",
          "--metric", "NDCG,HR", "--topk", "1,2,3,5", "--main_metric", "NDCG@2", "--save_final_results", "0",
          "--train_max_pos_item", "3", "--train_max_neg_item", "6", "--test_max_pos_item", "3", "--test_max_neg_item", "6"]


@pytest.mark.parametrize("cls,ranker,ranker_flags,flags", [
    ("PRMGeneral", "BPRMF", ["--emb_size", "32"], ["--emb_size", "16", "--num_hidden_unit", "32", "--num_heads", "2", "--n_blocks", "2"]),
    ("PRMSequential", "SASRec", ["--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--history_max", "5"],
     ["--emb_size", "32", "--num_hidden_unit", "64", "--num_heads", "4", "--n_blocks", "1", "--history_max", "5"])])
def test_cli_reranks_the_lists_of_a_ranker_trained_here(cls, ranker, ranker_flags, flags, tmp_path, cuda, monkeypatch):
    """a <ranker>Impression checkpoint written by this repository's own CLI, its yaml beside it, then one epoch of the re-ranker:
    the loss is finite, every block went through the fused node, and the logged test metrics equal those recomputed from predict"""
    import main
    import yaml
    from helpers.ImpressionRunner import ImpressionRunner
    from rechorus_amd import nn as hnn
    from synth_data import make_impression_dataset
    make_impression_dataset(str(tmp_path), "imp", n_users=120, n_items=80, n_imp=8, seed=5)
    monkeypatch.chdir(tmp_path)
    folder = tmp_path / "model" / (ranker + "Impression")
    main.run(["--model_name", ranker, "--model_mode", "Impression", "--path", str(tmp_path) + "/", "--regenerate", "1",
              "--log_file", str(tmp_path / "log" / "ranker.txt"), "--model_path", str(folder / "ranker.pt")] + ranker_flags + COMMON)
    config = {k.lstrip("-"): int(v) for k, v in zip(ranker_flags[::2], ranker_flags[1::2])}
    config["history_max"] = 99      # never taken from the yaml
    (folder / (ranker + ".yaml")).write_text(yaml.safe_dump(config))
    seen, fused, evaluate, train_node, eval_node = [], [], ImpressionRunner.evaluate, hnn.list_encoder_block, hnn.list_encoder_block_eval
    monkeypatch.setattr(ImpressionRunner, "evaluate", lambda self, data, topks, metrics, *a, **k: seen.append(
        (self, data, topks, metrics, evaluate(self, data, topks, metrics, *a, **k))) or seen[-1][-1])
    monkeypatch.setattr(hnn, "list_encoder_block", lambda *a, **k: fused.append("train") or train_node(*a, **k))
    monkeypatch.setattr(hnn, "list_encoder_block_eval", lambda *a, **k: fused.append("eval") or eval_node(*a, **k))
    log = str(tmp_path / "log" / "rerank.txt")
    res = main.run(["--model_name", cls, "--ranker_name", ranker, "--ranker_config_file", ranker + ".yaml", "--ranker_model_file",
                    "ranker.pt", "--path", str(tmp_path) + "/", "--regenerate", "0", "--log_file", log,
                    "--model_path", str(tmp_path / "model" / cls / "m.pt")] + flags + COMMON)
    import re
    found = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", open(log).read())
    assert found and np.isfinite(float(found.group(1))), open(log).read()[-2000:]
    assert "train" in fused and "eval" in fused and "NDCG@2" in res["test"]
    runner, data, topks, metrics, logged = seen[-1]
    model = data.model
    assert data.phase == "test" and type(model).__name__ == cls and not any(p.requires_grad for p in model.ranker.parameters())
    saved = torch.load(str(folder / "ranker.pt"), map_location="cpu")
    for k, v in model.ranker.state_dict().items():      # the trained ranker, not the head's init stream
        assert torch.equal(v.cpu(), saved[k]), k
    pred = runner.predict(data)
    mp, mn = model.test_max_pos_item, model.test_max_neg_item
    pos, neg = np.asarray(data.data["pos_num"]), np.asarray(data.data["neg_num"])
    col = np.arange(pred.shape[1])[None, :]
    keep = (col < np.minimum(pos, mp)[:, None]) | ((col >= mp) & (col < mp + np.minimum(neg, mn)[:, None]))
    again = ImpressionRunner.evaluate_method(np.where(keep, pred, -np.inf), topks, metrics, 0, neg, mp, pos)
    assert sorted(again) == sorted(logged)
    for k in logged:
        assert abs(float(again[k]) - float(logged[k])) <= 1e-6, (k, again[k], logged[k])
