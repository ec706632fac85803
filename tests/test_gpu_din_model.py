"""GPU: DINCTR / DINTopK against the goldens written FROM THE REFERENCE (tests/golden/make_golden_din.py): the attention unit's
output and weights, prediction, loss, every gradient, and the parameters and BatchNorm buffers after two optimizer steps.

Tolerances: each comparison gets 10 x the reference's own fp32 error on that quantity (the golden's dev/*: the reference in fp32
against the same modules in float64), relative to the largest magnitude of the compared array (gradients: at least 1e-6 of the largest
entry of any gradient, the generator's floor), capped at the project's 2e-5.  Named exceptions:
  * a quantity whose dev/* is itself above 2e-5 gets 10 x dev: the reference's own fp32 run is outside the cap on it (BatchNorm's
    weight gradient, the loss over 3 rows);
  * single-element gradients (the attention's b_out, the tower's output bias) are ONE signed sum over all instances that nearly or
    exactly cancels (exactly under the pairwise BPR loss), so their relative error is set by the cancellation, not by the kernel:
    they get 10 x the largest dev/* any golden records for a single-element gradient;
  * `zero_grad_keys` (the bias of a Linear in front of BatchNorm1d) have an exactly-zero gradient in exact arithmetic: round-off in
    every precision, no dev/*; they are bounded absolutely by 1e-5 of the largest gradient entry;
  * the case with numeric fields has no dev/* (the reference's .float() calls stop its double run): it takes the largest dev/* the
    other cases record for the same key, or, for keys they do not have, for the same module;
  * parameters after two optimizer steps: conftest.assert_update_close as for every model here (the step amplifies round-off of g
    where |g| ~ eps for Adam / Adagrad).
Every error and its bound are printed."""
import numpy as np
import pytest
import torch

from conftest import assert_update_close, load_golden
import din_model_cases as DC

pytestmark = pytest.mark.gpu
CAP = 2e-5


def rel(got, want, floor=0.0):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), floor, 1e-30))


def bound(dev):
    return 10 * dev if dev > CAP else min(CAP, 10 * dev)


def recorded_devs():
    """(per key, per module, single-element gradients): the largest dev/* over the cases that have them"""
    by_key, by_module, scalar = {}, {}, 0.0
    for name in DC.CASES:
        g = load_golden(name)
        for k in g:
            if not k.startswith("dev/"):
                continue
            v = float(g[k])
            by_key[k] = max(by_key.get(k, 0.0), v)
            if k.startswith("dev/G/"):
                mod = "dev/G/" + k[6:].split(".")[0]
                by_module[mod] = max(by_module.get(mod, 0.0), v)
                if g["G/" + k[6:]].size == 1:
                    scalar = max(scalar, v)
    return by_key, by_module, scalar


def dev_of(g, key, recorded):
    by_key, by_module, scalar = recorded
    if key.startswith("G/") and g[key].size == 1:
        return max(scalar, CAP)      # (above the cap: bound() does not clip it)
    if "dev/" + key in g:
        return float(g["dev/" + key])
    if "dev/" + key in by_key:
        return by_key["dev/" + key]
    return by_module["dev/G/" + key[2:].split(".")[0]]


@pytest.mark.parametrize("name", DC.CASES)
def test_model_matches_the_reference_golden(name, cuda):
    g = load_golden(name)
    fallback = recorded_devs()
    model, args, corpus = DC.build(g)
    model = DC.scale_to_p0(model, g).to(cuda)
    model.train()
    seen = {}
    plain = type(model).attention

    def spy(current, history, lengths, n_cand):
        seen["out"], seen["w"] = plain(model, current, history, lengths, n_cand)
        return seen["out"], seen["w"]
    model.attention = spy
    out = model(DC.feed(g, 1, cuda))
    del model.attention
    pred = out["prediction"]
    loss = model.loss(out)
    loss.backward()
    torch.cuda.synchronize()
    checks = [("att_out", seen["out"].detach().cpu().numpy(), g["att_out"]), ("att_w", seen["w"].cpu().numpy(), g["att_w"]),
              ("pred", pred.detach().cpu().numpy().reshape(g["pred"].shape), g["pred"]), ("loss", np.array([loss.item()]), np.array([g["loss"]]))]
    for key, got, want in checks:
        err, tol = rel(got, want), bound(dev_of(g, key, fallback))
        print(f"din model {name} {key}: error {err:.3e} bound {tol:.3e}")
        assert err <= tol, (name, key, err, tol)
    grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
    assert sorted(grads) == sorted(k[2:] for k in g if k.startswith("G/"))
    gmax = max(float(np.abs(g["G/" + k]).max()) for k in grads)
    zero = set(str(k) for k in g["zero_grad_keys"])
    for k, got in grads.items():
        if k in zero:
            assert float(np.abs(got).max()) <= 1e-5 * gmax, (name, k)
            continue
        err, tol = rel(got, g["G/" + k], 1e-6 * gmax), bound(dev_of(g, "G/" + k, fallback))
        print(f"din model {name} G/{k}: error {err:.3e} bound {tol:.3e}")
        assert err <= tol, (name, k, err, tol)


@pytest.mark.parametrize("name", DC.CASES)
def test_two_optimizer_steps_match_the_reference_golden(name, cuda, tmp_path):
    import argparse
    from helpers.BaseRunner import BaseRunner
    g = load_golden(name)
    opt = [k[:-6] for k in g if k.endswith("_hyper")][0]
    lr, l2 = (float(x) for x in g[opt + "_hyper"])
    model, _, _ = DC.build(g)
    model = DC.scale_to_p0(model, g).to(cuda)
    model.train()
    P0 = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.optimizer, a.lr, a.l2, a.train, a.log_file = opt, lr, l2, 1, str(tmp_path / "log.txt")
    model.optimizer = BaseRunner(a)._build_optimizer(model)
    losses = []
    for n in (1, 2):
        model.optimizer.zero_grad()
        ls = model.loss(model(DC.feed(g, n, cuda)))
        ls.backward()
        model.optimizer.step()
        losses.append(ls.item())
    torch.cuda.synchronize()
    np.testing.assert_allclose(losses, g[opt + "_losses"], rtol=2e-5)
    zero = set(str(k) for k in g["zero_grad_keys"])
    for k, v in model.state_dict().items():
        want = g["%s/%s" % (opt, k)]
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(want) == 2
            continue
        got = v.cpu().numpy()
        if k in zero:
            # the gradient is round-off around an exact zero (see the module docstring): Adam / Adagrad normalise it to a step of
            # about lr in a direction the round-off decides, in the reference as well -- only the size of the move is held
            assert float(np.abs(got - P0[k]).max()) <= 2.5 * lr + 1e-5, (name, k)
            continue
        if k.endswith(".bn.running_mean"):
            # Dice's BatchNorm reads the output of the BatchNorm in front of it, whose batch mean is its bias: 0 at the first step,
            # so the running mean starts from the round-off of a zero mean of unit-scale values -- held absolutely at 1e-5
            assert float(np.abs(got - want).max()) <= 1e-5, (name, k, float(np.abs(got - want).max()))
            continue
        extra = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
        if opt in ("Adam", "Adagrad") and k.endswith(".running_mean") and k[:-len("running_mean")] + "weight" in P0 and \
                "dnn_mlp_layers.mlp.%d.bias" % (int(k.split(".")[2]) - 1) in zero:
            # the batch mean of the second step contains the bias in front, which the first step moved by about lr in a direction
            # round-off decided (above); it enters the running mean with BatchNorm's momentum 0.1
            extra = 0.1 * 2.5 * lr
        assert_update_close(got, P0[k], want, what=f"{name} {opt} {k}", extra_atol=extra)


def test_forward_concatenates_no_tensor_of_history_rows(cuda, monkeypatch):
    """nothing of N * L (or B * L) rows goes through torch.cat / torch.stack: the history comes from ONE gather, the attention is
    one node"""
    g = load_golden("din_topk_d16_a64x64x64_l10_k4_b7_hs")
    model, _, _ = DC.build(g)
    model = DC.scale_to_p0(model, g).to(cuda)
    B, C, L = int(g["meta"][4]), int(g["meta"][5]), int(g["meta"][3])
    real_cat, real_stack = torch.cat, torch.stack
    rows = []

    def cat(tensors, *a, **k):
        out = real_cat(tensors, *a, **k)
        rows.append(out.numel() // out.shape[-1] if out.dim() > 1 else 1)
        return out

    def stack(tensors, *a, **k):
        raise AssertionError("torch.stack in DIN's forward")
    monkeypatch.setattr(torch, "cat", cat)
    monkeypatch.setattr(torch, "stack", stack)
    model(DC.feed(g, 1, cuda))
    monkeypatch.undo()
    assert rows and max(rows) <= B * C < B * L, rows


@pytest.mark.parametrize("mode", ["CTR", "TopK"])
def test_cli_trains_one_epoch_with_dropout_and_reloads_its_checkpoint(mode, tmp_path, cuda):
    import re
    import din_data
    import main
    root = str(tmp_path / "data")
    names = din_data.write(root, n_users=60, n_items=50, per_user=12)
    log, ckpt = str(tmp_path / "run.txt"), str(tmp_path / "din.pt")
    task = (["--model_mode", "CTR", "--loss_n", "BCE", "--metric", "AUC,ACC"] if mode == "CTR"
            else ["--model_mode", "TopK", "--num_neg", "2", "--topk", "5,10"])
    argv = ["--model_name", "DIN", "--emb_size", "16", "--att_layers", "[32,16]", "--dnn_layers", "[32]", "--history_max", "5",
            "--add_historical_situations", "1", "--dropout", "0.5", "--lr", "5e-3", "--l2", "0", "--path", root + "/",
            "--dataset", names[mode], "--epoch", "1", "--batch_size", "64", "--num_workers", "0", "--regenerate", "1",
            "--include_item_features", "1", "--include_user_features", "1", "--include_situation_features", "1",
            "--log_file", log, "--model_path", ckpt, "--save_final_results", "0"] + task
    res = main.run(argv)
    found = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", open(log).read())
    assert found and np.isfinite(float(found.group(1)))
    assert ("AUC" if mode == "CTR" else "HR@5") in res["test"]
    again = main.run(argv + ["--train", "0", "--load", "1"])        # the checkpoint alone: same metrics in eval mode
    assert again["test"] == res["test"]
