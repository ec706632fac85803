"""GPU: the set attention block on the HIP engine (rc_setmab_fwd / _bwd) against the float64 restatement (tests/setrank_np.py) on the
grid of setrank_np.MAB_PROBLEMS: one shared [20, d] query source under a mask at (nq, nk) = (20, n) and per-list queries without a mask
at (n, 20) for every n in {1, 2, 15, 16, 17, 40, 48} at (d, H, d_ff) = (64, 4, 128) with 65 lists; per-list queries under a mask at
(17, 33), (33, 17) and (1, 1); every shape of prm_np.SHAPES the envelope admits at (20, 17) shared and (17, 20) with 3 and 257 lists
(the backward launches at most 256 workgroups: with 257 lists one workgroup walks a second list); one list alone.  The four mask kinds
(random, one valid key, all valid, [valid | pad | valid | pad]) take turns over the lists of every masked problem; dY is non-zero
everywhere.  Y, dQs, dKs and all twelve weight and bias gradients are each compared against their own reference.

Tolerances: the project's rule, nothing new -- each comparison is held to the larger of 2e-5 and 4 x the stored deviation of the
reference's own fp32 `MAB` from float64 for that tensor (tests/golden/setrank_mab_dev.npz, written by
tests/golden/make_golden_setrank.py from models/reranker/SetRank.py:29-56; the problems are regenerated from their seeds), as largest
|difference| / largest |reference entry|.  No bound is computed at test time.  Each comparison prints its bound and the error it saw
(SETRANK_TOL lines, run with -s; profiles/setrank_tolerances.txt is that output of one run, folded).

The generator asserts the conditioning: every problem with a list of more than two valid keys has its least peaked list's largest
probability above 2 x uniform, and every problem with padding moves Y by more than 100 x its bound when the mask is ignored."""
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
import setrank_np as snp  # noqa: E402
from setrank_np import GRAD_NAMES, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEVS = load_golden("setrank_mab_dev")


def _check(got, want, what, bound, why):
    if torch.is_tensor(got):
        got = got.detach().cpu().numpy()
    err = rel_err(np.asarray(got).reshape(np.shape(want)), want)
    print(f"SETRANK_TOL {what}: {err:.3e} (allowed {bound:.3g}: {why})")
    assert err <= bound, f"{what}: largest error / largest entry {err:.3e} > {bound:g}"


@functools.lru_cache(maxsize=None)
def _reference(prob_id):
    """(problem, Y, gradients) in float64, computed once per problem and shared (never written to)"""
    prob = snp.problem(prob_id)
    Qs, Ks, pad, W, dY = prob
    return prob, snp.mab_forward(Qs, Ks, pad, W, prob_id[4]), snp.mab_backward(dY, Qs, Ks, pad, W, prob_id[4])


def _to(cuda, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _run_mab(prob, H, cuda, workspace=None):
    from rechorus_amd import engine
    Qs, Ks, pad, W, dY = prob
    q, k, m, dy, w = _to(cuda, Qs), _to(cuda, Ks), _to(cuda, pad), _to(cuda, dY), [_to(cuda, a) for a in W]
    shared = q.dim() == 2
    Y = engine.setmab_fwd(q, k, m, w, H, shared)
    dQs, dKs, grads = engine.setmab_bwd(dy, q, k, m, w, H, shared, workspace=workspace)
    return (q, k, m, *w, dy), Y, [dQs, dKs] + list(grads)


def _what(p):
    B, nq, nk, d, H, dff, shared, masked, _ = p
    return f"B={B} nq={nq} nk={nk} d={d} H={H} d_ff={dff} {'shared' if shared else 'per-list'} {'masked' if masked else 'unmasked'}"


def _check_mab(prob_id, cuda, workspace=None):
    key, what = snp.mab_key(*prob_id), _what(prob_id)
    prob, Y64, G64 = _reference(prob_id)
    _, Y, grads = _run_mab(prob, prob_id[4], cuda, workspace)
    _check(Y, Y64, what + " Y", *snp.stored_bound(DEVS, key + "/Y"))
    for name, got in zip(GRAD_NAMES, grads):
        _check(got, G64[name], f"{what} {name}", *snp.stored_bound(DEVS, f"{key}/{name}"))
    return prob, Y, grads


def _problems(pick):
    found = [p for p in snp.MAB_PROBLEMS if pick(p)]
    assert found
    return found


@pytest.mark.parametrize("n", snp.LENGTHS)
def test_shared_queries_under_the_mask_at_every_key_count(n, cuda):
    (p,) = _problems(lambda p: p[:8] == (65, snp.M, n, 64, 4, 128, 1, 1))
    prob, _, grads = _check_mab(p, cuda)
    assert {snp.MASKS[(b + p[8]) % 4] for b in range(65)} == set(snp.MASKS)
    assert np.abs(prob[4]).min() > 0
    if n == 1:
        # one valid key: the softmax is identically 1 and no gradient reaches q or k -- exact zeros, in the reference as well
        d = 64
        assert (grads[2][:2 * d] == 0).all() and (grads[3][:2 * d] == 0).all()
        assert (_reference(p)[2]["dWin"][:2 * d] == 0).all() and (_reference(p)[2]["dbin"][:2 * d] == 0).all()
        assert not (grads[2][2 * d:] == 0).all()
    else:
        pad = prob[2]
        assert pad.sum() > 0 and (pad.sum(1) == n - 1).any() and (pad.sum(1) == 0).any()
        assert (grads[1][torch.from_numpy(pad.astype(bool))] == 0).all()            # a masked key's row gets no gradient


@pytest.mark.parametrize("n", snp.LENGTHS)
def test_per_list_queries_without_a_mask_at_every_query_count(n, cuda):
    (p,) = _problems(lambda p: p[:8] == (65, n, snp.M, 64, 4, 128, 0, 0))
    prob, _, _ = _check_mab(p, cuda)
    assert prob[2] is None and np.abs(prob[4]).min() > 0


@pytest.mark.parametrize("nq,nk", [(17, 33), (33, 17), (1, 1)])
def test_per_list_queries_under_the_mask(nq, nk, cuda):
    (p,) = _problems(lambda p: p[:8] == (65, nq, nk, 64, 4, 128, 0, 1))
    _, _, grads = _check_mab(p, cuda)
    if nk == 1:
        assert (grads[2][:128] == 0).all() and (grads[3][:128] == 0).all()


@pytest.mark.parametrize("d,H,dff", snp.SHAPES)
def test_every_admitted_shape_with_few_lists_and_with_more_lists_than_workgroups(d, H, dff, cuda):
    from rechorus_amd import engine
    ws = engine.SetMabWorkspace()
    probs = _problems(lambda p: p[3:6] == (d, H, dff) and p[0] in (3, 257))
    assert sorted((p[0], p[6]) for p in probs) == [(3, 0), (3, 1), (257, 0), (257, 1)]
    for p in probs:
        _check_mab(p, cuda, ws)


def test_every_shape_of_the_list_encoder_grid_is_admitted_or_refused_by_the_lds_rule():
    from rechorus_amd import engine
    for d, H, dff in snp.prm_np.SHAPES:
        if (d, H, dff) in snp.SHAPES:
            engine.setmab_check_shape(snp.M, 17, d, H, dff)
            engine.setmab_check_shape(17, snp.M, d, H, dff)
        else:
            with pytest.raises(ValueError, match="bytes of LDS"):
                engine.setmab_check_shape(snp.M, 17, d, H, dff)


@pytest.mark.parametrize("shared", [1, 0])
def test_one_list_alone(shared, cuda):
    _check_mab(_problems(lambda p: p[0] == 1 and p[6] == shared)[0], cuda)


@pytest.mark.parametrize("p", snp.SELF_PROBLEMS, ids=lambda p: snp.mab_key(*p))
def test_queries_that_are_the_keys_agree_with_the_list_encoder_kernels(p, cuda):
    """per-list Qs equal to Ks under the mask: the same block as engine.listenc_block_fwd / _bwd computes, within the same bounds;
    dQs + dKs stands for dX"""
    from rechorus_amd import engine
    key, what = snp.mab_key(*p), _what(p) + " Qs = Ks"
    prob, Y64, G64 = _reference(p)
    assert prob[0].tobytes() == prob[1].tobytes()
    t, Y, grads = _run_mab(prob, p[4], cuda)
    x, pad, w, dy = t[1], t[2], list(t[3:15]), t[15]
    Yl = engine.listenc_block_fwd(x, pad, w, p[4])
    dX, gl = engine.listenc_block_bwd(dy, x, pad, w, p[4])
    _check(Y, Y64, what + " Y", *snp.stored_bound(DEVS, key + "/Y"))
    _check(Yl, Y64, what + " Y of listenc", *snp.stored_bound(DEVS, key + "/Y"))
    dX64 = G64["dQs"] + G64["dKs"]
    bound = max(snp.stored_bound(DEVS, key + "/dQs"), snp.stored_bound(DEVS, key + "/dKs"))
    _check(grads[0] + grads[1], dX64, what + " dQs + dKs", *bound)
    _check(dX, dX64, what + " dX of listenc", *bound)
    for name, a, b in zip(GRAD_NAMES[2:], grads[2:], gl):
        _check(a, G64[name], f"{what} {name}", *snp.stored_bound(DEVS, f"{key}/{name}"))
        _check(b, G64[name], f"{what} {name} of listenc", *snp.stored_bound(DEVS, f"{key}/{name}"))


def test_reruns_are_bit_identical_and_a_reused_workspace_changes_nothing(cuda):
    from rechorus_amd import engine
    big = _problems(lambda p: p[:8] == (257, snp.M, 17, 64, 4, 128, 1, 1))[0]
    for p in (big, _problems(lambda p: p[:8] == (257, 17, snp.M, 32, 2, 128, 0, 0))[0],
              _problems(lambda p: p[:8] == (65, snp.M, 40, 64, 4, 128, 1, 1))[0]):
        prob = _reference(p)[0]
        runs = []
        for _ in range(2):
            t, Y, grads = _run_mab(prob, p[4], cuda)
            runs.append([x.cpu().numpy().copy() for x in [Y] + grads])
            for a, b in zip(t, (prob[0], prob[1], prob[2], *prob[3], prob[4])):      # the inputs stay as they were
                assert (a is None and b is None) or a.cpu().numpy().tobytes() == b.tobytes(), p
        for a, b in zip(*runs):
            assert a.tobytes() == b.tobytes(), p
    # a workspace that served a larger problem of the same shape first (257 lists, then 3): the results equal those of a fresh
    # workspace bit for bit
    used = engine.SetMabWorkspace()
    _run_mab(_reference(big)[0], 4, cuda, used)
    small = _problems(lambda p: p[:8] == (3, snp.M, 17, 64, 4, 128, 1, 1))[0]
    _, _, fresh = _run_mab(_reference(small)[0], 4, cuda, engine.SetMabWorkspace())
    for _ in range(2):
        _, _, again = _run_mab(_reference(small)[0], 4, cuda, used)
        for a, b in zip(fresh, again):
            assert torch.equal(a, b)
    assert len(used._bufs) == 2


def test_a_lists_rows_do_not_depend_on_what_else_its_workgroup_walks(cuda):
    """700 lists on 256 workgroups (up to three lists each) against the same lists in four batches of 175 (one list per workgroup), with
    a shared query source: Y and dKs bit for bit -- nothing of a list outlives it in the workgroup's LDS or registers, and the shared
    projection computed once is the one computed per batch -- and the summed gradients, whose order changes, to the cap"""
    B, n = 700, 40
    Qs, Ks, pad, W, dY = snp.random_mab(B, snp.M, n, 64, 4, 128, 1, 1, seed=78)
    _, Y, grads = _run_mab((Qs, Ks, pad, W, dY), 4, cuda)
    parts = [_run_mab((Qs, Ks[s:s + 175], pad[s:s + 175], W, dY[s:s + 175]), 4, cuda)[1:] for s in range(0, B, 175)]
    assert torch.equal(Y, torch.cat([y for y, _ in parts])) and torch.equal(grads[1], torch.cat([g[1] for _, g in parts]))
    for k, name in enumerate(GRAD_NAMES):
        if name != "dKs":
            want = sum(g[k].double() for _, g in parts).cpu().numpy()
            _check(grads[k], want, f"700 lists against 4 x 175 {name}", snp.TOL, "the cap")


def test_autograd_nodes_the_induced_block_and_the_evaluation_forms(cuda):
    """nn.set_attention_block as a node (shared source: I's gradient is the sum over the lists), nn.induced_set_block as the chain of
    two of them (x's two gradients added by autograd), and the evaluation forms"""
    from rechorus_amd import nn as hnn
    p = _problems(lambda p: p[:8] == (3, snp.M, 17, 32, 2, 128, 1, 1))[0]
    prob, Y64, G64 = _reference(p)
    Qs, Ks, pad, W, dY = prob
    leaf = lambda a: torch.from_numpy(a).to(cuda).requires_grad_(True)
    q, k, w = leaf(Qs), leaf(Ks), [leaf(a) for a in W]
    mask = torch.from_numpy(pad.astype(bool)).to(cuda)
    y = hnn.set_attention_block(q, k, mask, w, p[4], shared_q=True)
    y.backward(torch.from_numpy(dY).to(cuda))
    key = snp.mab_key(*p)
    _check(y, Y64, "node Y", *snp.stored_bound(DEVS, key + "/Y"))
    for name, t in zip(GRAD_NAMES, [q, k] + w):
        _check(t.grad, G64[name], "node " + name, *snp.stored_bound(DEVS, f"{key}/{name}"))
    with pytest.raises(RuntimeError, match="no backward"):
        hnn.set_attention_block_eval(q, k, mask, w, p[4], shared_q=True)
    with torch.no_grad():
        ev = hnn.set_attention_block_eval(q, k, mask, w, p[4], shared_q=True)
    assert not ev.requires_grad and torch.equal(ev, y.detach())
    # the induced block is the two nodes chained: h passes between them as an ordinary tensor and autograd adds x's two gradients (MAB2's
    # queries, MAB1's keys).  Against the engine's own calls on the same inputs that is bit for bit, so no bound is needed: each block
    # is held to float64 above.  The second block's weights are the twelve of the per-list problem of the same shape.
    from rechorus_amd import engine
    p2 = _problems(lambda r: r[:8] == (3, 17, snp.M, 32, 2, 128, 0, 0))[0]
    W2, dX = _reference(p2)[0][3], torch.from_numpy(_reference(p2)[0][4]).to(cuda)
    for t in [q, k] + w:
        t.grad = None
    w2 = [leaf(a) for a in W2]
    out = hnn.induced_set_block(k, mask, q, w, w2, p[4])
    out.backward(dX)
    with torch.no_grad():
        m8, wd, w2d = mask.to(torch.uint8), [t.detach() for t in w], [t.detach() for t in w2]
        h = engine.setmab_fwd(q.detach(), k.detach(), m8, wd, p[4], True)
        assert torch.equal(out, engine.setmab_fwd(k.detach(), h, None, w2d, p[4]))
        dx2, dh, g2 = engine.setmab_bwd(dX, k.detach(), h, None, w2d, p[4])
        dI, dx1, g1 = engine.setmab_bwd(dh, q.detach(), k.detach(), m8, wd, p[4], True)
        assert torch.equal(k.grad, dx2 + dx1) and torch.equal(q.grad, dI)
        for a, b, ga, gb in zip(w, w2, g1, g2):
            assert torch.equal(a.grad, ga) and torch.equal(b.grad, gb)
        assert torch.equal(hnn.induced_set_block_eval(k, mask, q, w, w2, p[4]), out.detach())
    assert float(dx1.abs().max()) > 0 and float(dx2.abs().max()) > 0


def test_shapes_outside_the_envelope_are_refused_with_the_reason(cuda):
    from rechorus_amd import engine
    Ks = torch.zeros(2, 40, 24, device=cuda)
    with pytest.raises(ValueError, match="outside the envelope"):
        engine.setmab_fwd(torch.zeros(20, 24, device=cuda), Ks, None,
                          [torch.zeros(s, device=cuda) for s in ((72, 24), (72,), (24, 24), (24,), (24,), (24,), (16, 24), (16,),
                                                                 (24, 16), (24,), (24,), (24,))], 2, shared_q=True)
    with pytest.raises(ValueError, match="Qs must be"):
        engine.setmab_fwd(torch.zeros(2, 20, 24, device=cuda), Ks, None, [], 2, shared_q=True)


# ---- the model classes against the reference's goldens --------------------------------------------------------------------------------
# The four goldens of tests/golden/make_golden_setrank.py (the reference's own SetRankGeneral / SetRankSequential on CPU, IMSAB and
# MSAB): init stream, collated batch (ranks on valid slots; a padded slot's rank is the sort's choice among ties, so block outputs and
# predictions are compared on valid slots), every block's output, prediction, loss, every gradient, two optimizer steps; all four
# class / type combinations through main.run.  The cases run on I x 100 (at its init the induced attention is blind) and on rescaled
# in_proj / out_proj / rFF0 / rFF1, each factor stored in the golden and applied here by setrank_np.scale_state.  Tensors above 2,048
# elements are stored as every fifth element (prm_np.keep / stored).
MODEL_CASES = [c for c in golden_cases("setrank_") if c != "setrank_mab_dev"]


def _collated(model, g, i, cuda):
    """batch i through the port's collate additions, held to the golden's: mask, masked scores, ranks, the ranker's vectors"""
    m = snp.meta(g)
    fd = model.add_ranker_outputs(snp.raw_batch(g, i, cuda), m["B"])
    pre, valid = "b%d/" % i, ~g["b%d/padding_mask" % i]
    assert (fd["padding_mask"].cpu().numpy() == ~valid).all()
    assert (fd["position"].cpu().numpy()[valid] == g[pre + "position"][valid]).all()
    for k in ("u_v", "i_v"):
        if pre + k in g:
            want, got = snp.stored(g, pre, k, fd[k].cpu().numpy())
            _check(got, want, f"batch {i} {k}", snp.TOL, "the cap")
    return fd, valid


@pytest.mark.parametrize("case", MODEL_CASES)
def test_model_matches_the_reference_golden(case, cuda, tmp_path, monkeypatch):
    from helpers.ImpressionRunner import ImpressionRunner
    g = load_golden(case)
    m = snp.meta(g)
    monkeypatch.chdir(tmp_path)
    model, _ = snp.golden_model(g, cuda, tmp_path)      # asserts the init stream and the ranker's weights
    model.train()
    assert len(MODEL_CASES) == 4 and (g["maxp"][:, :len(snp.mab_names(g))] > 2.0).all()
    fd3, valid3 = _collated(model, g, 3, cuda)              # the forward-only batch: holds the list with a single valid slot
    assert (valid3.sum(1) == 1).any()
    with torch.no_grad():
        xs = model.encode(fd3)[1:]
        pred3 = model(fd3)["prediction"].cpu().numpy()
    for l, x in enumerate(xs):
        want, got = snp.stored(g, "F/", "X%d" % l, x.cpu().numpy()[valid3])      # (a padded slot's rank is the sort's choice)
        _check(got, want, f"{case} forward-only X{l}", *snp.bound_for(g, "F/X%d" % l))
    _check(pred3[valid3], g["F/pred"][valid3], case + " forward-only pred", *snp.bound_for(g, "F/pred"))
    fd, valid = _collated(model, g, 1, cuda)
    for l, x in enumerate(model.encode(fd)[1:]):
        want, got = snp.stored(g, "", "X%d" % l, x.detach().cpu().numpy()[valid])
        _check(got, want, f"{case} X{l}", *snp.bound_for(g, "X%d" % l))
    out = model(fd)
    loss = model.loss(out, ImpressionRunner._labels(fd, m["P"] + m["N"], m["P"], cuda))
    loss.backward()
    torch.cuda.synchronize()
    _check(out["prediction"].detach().cpu().numpy()[valid], g["pred"][valid], case + " pred", *snp.bound_for(g, "pred"))
    _check(np.array([loss.item()]), np.array([float(g["loss"])]), case + " loss", *snp.bound_for(g, "loss"))
    zero, floor = set(str(k) for k in g["zero_grad_keys"]), snp.grad_floor(g)
    grads = {k: p.grad for k, p in model.named_parameters() if p.requires_grad}
    assert all(v is not None for v in grads.values()) and sorted(grads) == sorted(k[2:] for k in g if k.startswith("G/"))
    for k, got in grads.items():
        want, got = snp.stored(g, "G/", k, got.cpu().numpy())
        if k in zero:
            assert float(np.abs(got).max()) <= 1e-5 * 1e6 * floor, (case, k)
            continue
        bound, why = snp.bound_for(g, "G/" + k)
        err = rel_err(got, want, floor)
        print(f"SETRANK_TOL {case} grad {k}: {err:.3e} (allowed {bound:.3g}: {why})")
        assert err <= bound, f"{case} grad {k}: {err:.3e} > {bound:g}"
    assert all(p.grad is None for p in model.ranker.parameters())


@pytest.mark.parametrize("case", MODEL_CASES)
def test_two_optimizer_steps_match_the_reference_golden(case, cuda, tmp_path, monkeypatch):
    import argparse
    from helpers.BaseRunner import BaseRunner
    from helpers.ImpressionRunner import ImpressionRunner
    g = load_golden(case)
    m = snp.meta(g)
    opt = [k[:-6] for k in g if k.endswith("_hyper")][0]
    lr, l2 = (float(x) for x in g[opt + "_hyper"])
    monkeypatch.chdir(tmp_path)
    model, P0 = snp.golden_model(g, cuda, tmp_path)
    model.train()
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.optimizer, a.lr, a.l2, a.train, a.log_file = opt, lr, l2, 1, str(tmp_path / "log.txt")
    model.optimizer = BaseRunner(a)._build_optimizer(model)
    losses = []
    for i in (1, 2):
        fd = model.add_ranker_outputs(snp.raw_batch(g, i, cuda), m["B"])
        model.optimizer.zero_grad()
        ls = model.loss(model(fd), ImpressionRunner._labels(fd, m["P"] + m["N"], m["P"], cuda))
        ls.backward()
        model.optimizer.step()
        losses.append(ls.item())
    torch.cuda.synchronize()
    print(f"SETRANK_LOSSES {case} {opt}: {losses} (reference {g[opt + '_losses'].tolist()})")
    np.testing.assert_allclose(losses, g[opt + "_losses"], rtol=snp.TOL)
    zero, adaptive = set(str(k) for k in g["zero_grad_keys"]), opt in ("Adam", "Adagrad")
    for k, v in model.state_dict().items():
        if k.startswith("ranker."):
            assert v.cpu().numpy().tobytes() == P0[k].tobytes(), k      # frozen
            continue
        want, got = snp.stored(g, opt + "/", k, v.cpu().numpy())
        start = snp.stored(g, opt + "/", k, P0[k])[1]
        # a gradient that is round-off around an exact zero (the zero_grad_keys; the key-bias third of every in_proj_bias): Adam /
        # Adagrad normalise it to a step of about lr in a direction the round-off decides, in the reference as well -- only the size
        # of the move is held
        moved = (2.5 * lr if adaptive else 1e-5) + 1e-7
        if k in zero:
            assert float(np.abs(got - start).max()) <= moved, (case, k)
            continue
        exclude = snp.key_bias(k, got.shape)
        if exclude is not None:
            assert float(np.abs(got - start)[exclude].max()) <= moved, (case, k)
        assert_update_close(got, start, want, what=f"{case} {opt} {k}", extra_atol=1e-3 * lr if adaptive else 0.0,
                            outlier_atol=2 * lr if adaptive else 0.0, exclude=exclude)


# ---- the model classes through the CLI ------------------------------------------------------------------------------------------------
COMMON = ["--lr", "3e-3", "--l2", "0", "--loss_n", "BPR", "--dataset", "imp", "--epoch", "1", "--batch_size", "64", "--num_workers", "0",
          "--metric", "NDCG,HR", "--topk", "1,2,3,5", "--main_metric", "NDCG@2", "--save_final_results", "0",
          "--train_max_pos_item", "3", "--train_max_neg_item", "6", "--test_max_pos_item", "3", "--test_max_neg_item", "6"]
GENERAL = ("BPRMF", ["--emb_size", "32"], ["--emb_size", "16", "--num_hidden_unit", "32", "--num_heads", "2", "--n_blocks", "2"])
SEQUENTIAL = ("SASRec", ["--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--history_max", "5"],
              ["--emb_size", "32", "--num_hidden_unit", "64", "--num_heads", "4", "--n_blocks", "1", "--history_max", "5"])


@pytest.mark.parametrize("cls,setup", [("SetRankGeneral", GENERAL), ("SetRankSequential", SEQUENTIAL)])
def test_cli_reranks_the_lists_of_a_ranker_trained_here_with_both_block_types(cls, setup, tmp_path, cuda, monkeypatch):
    """a <ranker>Impression checkpoint written by this repository's own CLI, its yaml beside it, then one epoch of the re-ranker with
    each --setrank_type: the loss is finite, every block went through its fused nodes in training and in evaluation, and the logged
    test metrics equal those recomputed from predict"""
    import re
    import main
    import yaml
    from helpers.ImpressionRunner import ImpressionRunner
    from rechorus_amd import nn as hnn
    from synth_data import make_impression_dataset
    ranker, ranker_flags, flags = setup
    make_impression_dataset(str(tmp_path), "imp", n_users=120, n_items=80, n_imp=8, seed=5)
    monkeypatch.chdir(tmp_path)
    folder = tmp_path / "model" / (ranker + "Impression")
    main.run(["--model_name", ranker, "--model_mode", "Impression", "--path", str(tmp_path) + "/", "--regenerate", "1",
              "--log_file", str(tmp_path / "log" / "ranker.txt"), "--model_path", str(folder / "ranker.pt")] + ranker_flags + COMMON)
    config = {k.lstrip("-"): int(v) for k, v in zip(ranker_flags[::2], ranker_flags[1::2])}
    config["history_max"] = 99      # never taken from the yaml
    (folder / (ranker + ".yaml")).write_text(yaml.safe_dump(config))
    seen, fused, evaluate = [], [], ImpressionRunner.evaluate
    monkeypatch.setattr(ImpressionRunner, "evaluate", lambda self, data, topks, metrics, *a, **k: seen.append(
        (self, data, topks, metrics, evaluate(self, data, topks, metrics, *a, **k))) or seen[-1][-1])
    for name in ("list_encoder_block", "list_encoder_block_eval", "induced_set_block", "induced_set_block_eval"):
        monkeypatch.setattr(hnn, name, lambda *a, _f=getattr(hnn, name), _n=name, **k: fused.append(_n) or _f(*a, **k))
    for kind, nodes in (("IMSAB", {"induced_set_block", "induced_set_block_eval"}), ("MSAB", {"list_encoder_block", "list_encoder_block_eval"})):
        del fused[:]
        log = str(tmp_path / "log" / (kind + ".txt"))
        res = main.run(["--model_name", cls, "--ranker_name", ranker, "--ranker_config_file", ranker + ".yaml", "--ranker_model_file",
                        "ranker.pt", "--setrank_type", kind, "--path", str(tmp_path) + "/", "--regenerate", "0", "--log_file", log,
                        "--model_path", str(tmp_path / "model" / cls / (kind + ".pt"))] + flags + COMMON)
        found = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", open(log).read())
        assert found and np.isfinite(float(found.group(1))), open(log).read()[-2000:]
        assert set(fused) == nodes and "NDCG@2" in res["test"], (kind, set(fused))
        runner, data, topks, metrics, logged = seen[-1]
        model = data.model
        assert data.phase == "test" and type(model).__name__ == cls and model.setrank_type == kind
        assert not any(p.requires_grad for p in model.ranker.parameters())
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
