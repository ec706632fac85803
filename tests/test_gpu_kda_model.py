"""GPU: KDA against the goldens written FROM THE REFERENCE (tests/golden/make_golden_kda.py): the aggregation's context, both
predictions, the loss, every gradient, and the state_dict after two optimizer steps; one CLI epoch with the reference's demo flags
on a KGReader dataset.

Tolerances: each comparison gets the larger of 2e-5 and four times the reference's own fp32 error on that quantity (the golden's
dev/*: the reference in fp32 against the same modules in float64), relative to the largest magnitude of the compared array
(gradients: at least 1e-6 of the largest entry of any gradient, the generator's floor).  Parameters after two optimizer steps:
conftest.assert_update_close as for every model here (the step amplifies round-off of g where |g| ~ eps for Adam / Adagrad).
Every error and its bound are printed."""
import re

import numpy as np
import pytest
import torch

from conftest import assert_update_close, load_golden
import kda_model_cases as MC

pytestmark = pytest.mark.gpu
CAP = 2e-5
NAMES = sorted(MC.CASES)


def rel(got, want, floor=0.0):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), floor, 1e-30))


def bound(dev):
    return max(CAP, 4 * float(dev))


@pytest.mark.parametrize("name", NAMES)
def test_model_matches_the_reference_golden(name, cuda):
    g = load_golden(name)
    B = MC.CASES[name][7]
    model, args, corpus = MC.build(name)
    model = MC.scale_to_p0(model, g).to(cuda)
    model.train()
    seen = {}
    plain = type(model).aggregate

    def spy(*a):
        seen["context"] = plain(model, *a)
        return seen["context"]
    model.aggregate = spy
    out = model(MC.feed(g, 1, cuda, B))
    del model.aggregate
    loss = model.loss(out)
    loss.backward()
    torch.cuda.synchronize()
    checks = [("context", seen["context"].detach().cpu().numpy(), g["context"]),
              ("pred", out["prediction"].detach().cpu().numpy(), g["pred"]),
              ("kg_pred", out["kg_prediction"].detach().cpu().numpy(), g["kg_pred"]),
              ("loss", np.array([loss.item()]), np.array([g["loss"]]))]
    for key, got, want in checks:
        err, tol = rel(got, want), bound(g["dev/" + key])
        print(f"kda model {name} {key}: error {err:.3e} bound {tol:.3e}")
        assert err <= tol, (name, key, err, tol)
    grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
    assert sorted(grads) == sorted(k[2:] for k in g if k.startswith("G/"))
    gmax = max(float(np.abs(g["G/" + k]).max()) for k in grads)
    for k, got in grads.items():
        err, tol = rel(got, g["G/" + k], 1e-6 * gmax), bound(g["dev/G/" + k])
        print(f"kda model {name} G/{k}: error {err:.3e} bound {tol:.3e}")
        assert err <= tol, (name, k, err, tol)


@pytest.mark.parametrize("name", NAMES)
def test_two_optimizer_steps_match_the_reference_golden(name, cuda, tmp_path):
    import argparse
    from helpers.BaseRunner import BaseRunner
    g = load_golden(name)
    B = MC.CASES[name][7]
    opt = [k[:-6] for k in g if k.endswith("_hyper")][0]
    lr, l2 = (float(x) for x in g[opt + "_hyper"])
    model, _, _ = MC.build(name)
    model = MC.scale_to_p0(model, g).to(cuda)
    model.train()
    P0 = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.optimizer, a.lr, a.l2, a.train, a.log_file = opt, lr, l2, 1, str(tmp_path / "log.txt")
    model.optimizer = BaseRunner(a)._build_optimizer(model)
    losses = []
    for n in (1, 2):
        model.optimizer.zero_grad()
        ls = model.loss(model(MC.feed(g, n, cuda, B)))
        ls.backward()
        model.optimizer.step()
        losses.append(ls.item())
    torch.cuda.synchronize()
    np.testing.assert_allclose(losses, g[opt + "_losses"], rtol=max(CAP, 4 * float(g["dev/loss"])))
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in g["state_keys"]]
    for k, v in sd.items():
        extra = 1e-3 * lr if opt in ("Adam", "Adagrad") else 0.0
        assert_update_close(v.cpu().numpy(), P0[k], g["%s/%s" % (opt, k)], what=f"{name} {opt} {k}", extra_atol=extra)


def test_cli_trains_one_epoch_with_the_demo_flags_and_reloads_its_checkpoint(tmp_path, cuda):
    import main
    from slrc_data import make_kg_dataset
    root = str(tmp_path / "data")
    make_kg_dataset(root, "synth_kg", n_users=40, n_items=40, per_user=8, seed=5)
    log, ckpt = str(tmp_path / "run.txt"), str(tmp_path / "kda.pt")
    argv = ["--model_name", "KDA", "--emb_size", "64", "--include_attr", "1", "--freq_rand", "0", "--lr", "1e-3", "--l2", "1e-6",
            "--num_heads", "4", "--history_max", "5", "--n_dft", "16", "--num_neg", "2", "--dropout", "0.2", "--path", root + "/",
            "--dataset", "synth_kg", "--epoch", "1", "--batch_size", "64", "--num_workers", "0", "--regenerate", "1", "--topk", "5,10",
            "--log_file", log, "--model_path", ckpt, "--save_final_results", "0"]
    res = main.run(argv)
    found = re.search(r"Epoch 1\s+loss=(-?[0-9.]+|nan|inf)", open(log).read())
    assert found and np.isfinite(float(found.group(1)))
    assert "HR@5" in res["test"]
    again = main.run(argv + ["--train", "0", "--load", "1", "--regenerate", "0"])        # the checkpoint alone: same metrics in eval mode
    assert again["test"] == res["test"]
