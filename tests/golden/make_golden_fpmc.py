"""Golden vectors for FPMC FROM THE REFERENCE ITSELF (models/sequential/FPMC.py, helpers/SeqReader.py's flags, the optimizer
construction of helpers/BaseRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fpmc.py [--out DIR]

Each fpmc_*.npz holds
  meta [n_users, n_items, d, B, K, seed, redraw], hyper [lr, l2], opt (name)
  UI0, IU0, LI0, IL0       the four tables every computation below starts from: what FPMC.__init__ leaves after
                           torch.manual_seed(seed) (redraw = 0: normal(0, 0.01), the demo line), or (redraw = 1) re-drawn at
                           N(0, 0.3): with the native init every score is ~1e-3 and a wrong product hides in the loss
  uid, lid, iid            one training batch: users [B], last items [B], candidates [B, 1 + K] (column 0 the target)
  pred, loss               FPMC.forward's prediction [B, 1 + K] and GeneralModel.loss
  GUI, GIU, GLI, GIL       the four dense gradients of that loss
  UI1, IU1, LI1, IL1       the four tables after one step of the torch.optim optimizer BaseRunner builds (dense semantics: weight
                           decay reaches every row)
  state_keys, model_flags, reader_flags     the state_dict keys and the option strings FPMC.parse_model_args / SeqReader.parse_data_args add
Ids are Zipf-distributed over small tables, so users, last items and candidates repeat inside the batch; a few slots are set by
hand so that a negative equals the positive, a candidate repeats inside a tuple and a last item is among its tuple's candidates.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

TABLES = (("UI", "ui_embeddings.weight"), ("IU", "iu_embeddings.weight"), ("LI", "li_embeddings.weight"), ("IL", "il_embeddings.weight"))


def _flags(add):
    p = argparse.ArgumentParser()
    before = {s for a in p._actions for s in a.option_strings}
    p = add(p)
    return np.array(sorted({s for a in p._actions for s in a.option_strings} - before))


def make_case(out_dir, name, n_users, n_items, d, B, K, opt, lr, l2, seed, redraw):
    torch, _, BaseRunner = make_golden._import_reference()
    from helpers.SeqReader import SeqReader
    from models.sequential.FPMC import FPMC
    torch.set_num_threads(1)   # one summation order for every rerun
    rng = np.random.default_rng(seed)
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=K, dropout=0, test_all=0, emb_size=d,
                           history_max=20)
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items)
    drawn = {key: (0.3 * rng.standard_normal((n_users if key == "UI" else n_items, d))).astype(np.float32)
             for key, _ in TABLES} if redraw else {}

    def build():
        torch.manual_seed(seed)
        model = FPMC(args, corpus)
        with torch.no_grad():
            for key, full in TABLES:
                if key in drawn:
                    model.state_dict()[full].copy_(torch.from_numpy(drawn[key]))
        return model

    def snapshot(model, tag, out):
        sd = model.state_dict()
        for key, full in TABLES:
            out[key + tag] = sd[full].detach().numpy().copy()

    out = {"meta": np.array([n_users, n_items, d, B, K, seed, int(redraw)], dtype=np.int64),
           "hyper": np.array([lr, l2], dtype=np.float64), "opt": np.array(opt)}
    model = build()
    snapshot(model, "0", out)

    def zipf(n, size):
        p = 1.0 / np.arange(1, n)
        return rng.choice(np.arange(1, n), size=size, p=p / p.sum()).astype(np.int64)

    uid, lid, iid = zipf(n_users, B), zipf(n_items, B), zipf(n_items, (B, 1 + K))
    if K >= 2:
        iid[0, 1] = iid[0, 0]          # a negative equals the positive
        iid[0, 2] = iid[0, 1]          # ... and a candidate repeats inside the tuple
    lid[B - 1] = iid[B - 1, K]         # a last item that is one of its tuple's candidates
    out.update(uid=uid, lid=lid, iid=iid)
    feed = {"user_id": torch.from_numpy(uid), "item_id": torch.from_numpy(iid), "last_item_id": torch.from_numpy(lid),
            "batch_size": B, "phase": "train"}

    model.zero_grad()
    o = model(feed)
    loss = model.loss(o)
    loss.backward()
    out["pred"] = o["prediction"].detach().numpy().copy()
    out["loss"] = np.array(loss.item(), dtype=np.float32)
    sd = dict(model.named_parameters())
    for key, full in TABLES:
        out["G" + key] = sd[full].grad.numpy().copy()

    m = build()
    runner = BaseRunner(make_golden._runner_args(BaseRunner, opt, lr, l2))
    m.optimizer = runner._build_optimizer(m)
    m.train()
    m.optimizer.zero_grad()
    m.loss(m(feed)).backward()
    m.optimizer.step()
    snapshot(m, "1", out)

    out["state_keys"] = np.array(sorted(m.state_dict().keys()))
    out["model_flags"] = _flags(FPMC.parse_model_args)
    out["reader_flags"] = _flags(SeqReader.parse_data_args)

    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 << 10, (name, size)
    print("wrote", path, size >> 10, "KiB")


CASES = [
    # name,                     n_users, n_items,  d,   B,  K, opt,       lr,   l2,   seed, redraw
    ("fpmc_d16_sgd_b1_k1",           20,      30,  16,   1,  1, "SGD",     0.1,  1e-5, 61, True),
    ("fpmc_d32_sgd_b160_k4",         64,     300,  32, 160,  4, "SGD",     0.5,  0.0,  62, True),
    ("fpmc_d64_adam_b77_k99",        40,     120,  64,  77, 99, "Adam",    1e-3, 1e-6, 63, False),   # the demo line: pins the init stream
    ("fpmc_d128_adagrad_b33_k9",     30,      60, 128,  33,  9, "Adagrad", 0.01, 1e-4, 64, True),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    for c in CASES:
        make_case(a.out, *c)
