"""Golden vectors for BUIR FROM THE REFERENCE ITSELF (models/general/BUIR.py, helpers/BaseRunner.py, the per-batch order of
helpers/BUIRRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_buir.py [--out DIR]

Each buir_*.npz holds
  meta [n_users, n_items, d, B, seed, redraw], hyper [momentum, lr, l2], opt (name)
  UO0, UT0, IO0, IT0, W0, b0      the state every computation below starts from: what BUIR.__init__ leaves after
                                  torch.manual_seed(seed) (redraw = 0), or (redraw = 1) that W0 and b0 with online tables
                                  re-drawn at N(0, 0.5) and targets = online + N(0, 0.1) noise.  With the native init the bias
                                  (std ~ 0.9) swamps W x (table std ~ 0.07): every normalised predictor output is nearly the same
                                  vector and a wrong product would go unnoticed; the re-drawn cases are the ones that see it.
  uid, iid, uid2, iid2            two training batches (ids [B], [B, 1]: no negatives, BUIR.Dataset)
  pred, loss, GUO, GIO, GW, Gb    first batch: training prediction [B, 1], loss, the four gradients
  UO1 .. b2 (six tensors per step), losses   every table plus W and b after each of two iterations in BUIRRunner's order
                                  (zero_grad, forward, loss, backward, optimizer.step(), _update_target())
  eval_uid, eval_iid, eval_pred   eval-mode predictions of a batch with 99 candidates besides the target (model after the two
                                  iterations)
  state_keys
Batches are Zipf-distributed on both sides, so users and items repeat inside a batch.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

STATE = (("UO", "user_online.weight"), ("UT", "user_target.weight"), ("IO", "item_online.weight"), ("IT", "item_target.weight"),
         ("W", "predictor.weight"), ("b", "predictor.bias"))


def make_case(out_dir, name, n_users, n_items, d, B, momentum, opt, lr, l2, seed, redraw):
    torch, _, BaseRunner = make_golden._import_reference()
    from models.general.BUIR import BUIR
    torch.set_num_threads(1)   # one summation order for every rerun
    rng = np.random.default_rng(seed)
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=0, dropout=0, test_all=0,
                           emb_size=d, momentum=momentum)
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items)
    drawn = {}
    if redraw:
        for key, rows in (("UO", n_users), ("IO", n_items)):
            drawn[key] = (0.5 * rng.standard_normal((rows, d))).astype(np.float32)
        for key, src in (("UT", "UO"), ("IT", "IO")):
            drawn[key] = (drawn[src] + 0.1 * rng.standard_normal(drawn[src].shape)).astype(np.float32)

    def snapshot(model, tag, out):
        sd = model.state_dict()
        for key, full in STATE:
            out[key + tag] = sd[full].detach().numpy().copy()

    def build():
        torch.manual_seed(seed)
        model = BUIR(args, corpus)
        with torch.no_grad():
            for key, full in STATE[:4]:
                if key in drawn:
                    model.state_dict()[full].copy_(torch.from_numpy(drawn[key]))
        return model

    out = {"meta": np.array([n_users, n_items, d, B, seed, int(redraw)], dtype=np.int64),
           "hyper": np.array([momentum, lr, l2], dtype=np.float64), "opt": np.array(opt)}
    model = build()
    snapshot(model, "0", out)

    def batch():
        pu = 1.0 / np.arange(1, n_users)
        pu /= pu.sum()
        pi = 1.0 / np.arange(1, n_items)
        pi /= pi.sum()
        uid = rng.choice(np.arange(1, n_users), size=B, p=pu)
        iid = rng.choice(np.arange(1, n_items), size=(B, 1), p=pi)
        return uid.astype(np.int64), iid.astype(np.int64)

    uid, iid = batch()
    uid2, iid2 = batch()
    out.update(uid=uid, iid=iid, uid2=uid2, iid2=iid2)

    def feed(u, i):
        return {"user_id": torch.from_numpy(u), "item_id": torch.from_numpy(i), "batch_size": len(u), "phase": "train"}

    model.zero_grad()
    o = model(feed(uid, iid))
    loss = model.loss(o)
    loss.backward()
    assert model.user_target.weight.grad is None and model.item_target.weight.grad is None
    out["pred"] = o["prediction"].detach().numpy().copy()
    out["loss"] = np.array(loss.item(), dtype=np.float32)
    out["GUO"] = model.user_online.weight.grad.numpy().copy()
    out["GIO"] = model.item_online.weight.grad.numpy().copy()
    out["GW"] = model.predictor.weight.grad.numpy().copy()
    out["Gb"] = model.predictor.bias.grad.numpy().copy()

    m = build()
    runner = BaseRunner(make_golden._runner_args(BaseRunner, opt, lr, l2))
    m.optimizer = runner._build_optimizer(m)
    losses = []
    for step, (u, i) in enumerate(((uid, iid), (uid2, iid2)), 1):
        m.train()
        m.optimizer.zero_grad()
        ls = m.loss(m(feed(u, i)))
        ls.backward()
        m.optimizer.step()
        m._update_target()
        losses.append(ls.item())
        snapshot(m, str(step), out)
    out["losses"] = np.array(losses, dtype=np.float32)

    m.eval()
    eu = rng.integers(1, n_users, size=8).astype(np.int64)
    ei = rng.integers(1, n_items, size=(8, 100)).astype(np.int64)
    with torch.no_grad():
        ep = m({"user_id": torch.from_numpy(eu), "item_id": torch.from_numpy(ei), "batch_size": 8, "phase": "test"})["prediction"]
    out.update(eval_uid=eu, eval_iid=ei, eval_pred=ep.numpy().copy())
    out["state_keys"] = np.array(sorted(m.state_dict().keys()))

    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB")


CASES = [
    # name,                       n_users, n_items,   d,   B, momentum, opt,       lr,   l2,   seed, redraw
    ("buir_d64_adam_b77_native",      120,     100,  64,  77, 0.995,   "Adam",    1e-3, 1e-6, 51, False),  # the demo flags: pins the init stream
    ("buir_d32_sgd_b160",             250,     180,  32, 160, 0.995,   "SGD",     0.5,  0.0,  52, True),   # three tiles of 64 rows
    ("buir_d128_adagrad_b33_m09",      40,      30, 128,  33, 0.9,     "Adagrad", 0.01, 1e-4, 53, True),
    ("buir_d16_sgd_b1",               100,      60,  16,   1, 0.995,   "SGD",     0.1,  1e-5, 54, True),
    ("buir_d64_adam_b2_nol2",         100,      60,  64,   2, 0.995,   "Adam",    1e-3, 0.0,  55, True),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    for c in CASES:
        make_case(a.out, *c)
