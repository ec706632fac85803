"""Golden vectors for DirectAU FROM THE REFERENCE ITSELF (models/general/DirectAU.py, helpers/BaseRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_directau.py [--out DIR]

Each directau_*.npz holds
  meta [n_users, n_items, d, B, seed], hyper [gamma, lr, l2], opt (name)
  U0 / I0                       initial tables (xavier_normal_, DirectAU.py:35-42, after torch.manual_seed(seed))
  uid, iid, uid2, iid2          two training batches (ids [B], [B, 1]: no negatives, DirectAU.Dataset)
  pred, loss, GU, GI            first batch: training prediction [B, 1], loss, both table gradients
  U1, I1, U2, I2, losses        tables after each of two fit() iterations (BaseRunner._build_optimizer, the fit call order)
  eval_uid, eval_iid, eval_pred eval-mode predictions of a batch with 99 candidates besides the target (model after the two
                                iterations)
Batches are Zipf-distributed on both sides, so users and items repeat inside a batch.  B = 1 records what the reference returns
when torch.pdist has no pair: a NaN loss, and gradients that carry the alignment term only.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402


def make_case(out_dir, name, n_users, n_items, d, B, gamma, opt, lr, l2, seed):
    torch, _, BaseRunner = make_golden._import_reference()
    from models.general.DirectAU import DirectAU
    torch.set_num_threads(1)   # one summation order for every rerun
    rng = np.random.default_rng(seed)
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=0, dropout=0, test_all=0,
                           emb_size=d, gamma=gamma)
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items)

    def build():
        torch.manual_seed(seed)
        return DirectAU(args, corpus)

    model = build()
    out = {"meta": np.array([n_users, n_items, d, B, seed], dtype=np.int64), "hyper": np.array([gamma, lr, l2], dtype=np.float64),
           "opt": np.array(opt)}
    out["U0"] = model.u_embeddings.weight.detach().numpy().copy()
    out["I0"] = model.i_embeddings.weight.detach().numpy().copy()

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
    out["pred"] = o["prediction"].detach().numpy().copy()
    out["loss"] = np.array(loss.item(), dtype=np.float32)
    out["GU"] = model.u_embeddings.weight.grad.numpy().copy()
    out["GI"] = model.i_embeddings.weight.grad.numpy().copy()

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
        losses.append(ls.item())
        out["U%d" % step] = m.u_embeddings.weight.detach().numpy().copy()
        out["I%d" % step] = m.i_embeddings.weight.detach().numpy().copy()
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
    # name,                          n_users, n_items,   d,   B, gamma, opt,       lr,   l2,   seed
    ("directau_d64_g03_adam_b77",        300,     200,  64,  77, 0.3,  "Adam",    1e-3, 1e-5, 41),   # the demo flags, B off every tile
    ("directau_d32_g1_sgd_b160",         250,     180,  32, 160, 1.0,  "SGD",     0.5,  0.0,  42),   # five 32-row column blocks
    ("directau_d128_g0_adagrad_b50",     120,      90, 128,  50, 0.0,  "Adagrad", 0.01, 1e-4, 43),   # gamma 0: alignment only
    ("directau_d64_g1_adam_b1",          100,      60,  64,   1, 1.0,  "Adam",    1e-3, 0.0,  44),   # no pair: NaN loss
    ("directau_d32_g03_sgd_b2",          100,      60,  32,   2, 0.3,  "SGD",     0.1,  1e-5, 45),   # one pair
    ("directau_d128_g03_adam_b300",      200,     150, 128, 300, 0.3,  "Adam",    1e-2, 1e-6, 46),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    for c in CASES:
        make_case(a.out, *c)
