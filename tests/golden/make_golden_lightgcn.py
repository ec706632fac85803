"""Golden vectors for LightGCN FROM THE REFERENCE ITSELF (models/general/LightGCN.py, helpers/BaseRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lightgcn.py

The reference's LGCNEncoder moves its adjacency to the GPU in __init__ (`.cuda()`, LightGCN.py:117); for the duration of the
model's construction torch.Tensor.cuda returns the tensor itself, so everything runs on CPU.  Each lightgcn_*.npz holds
  meta [n_users, n_items, d, L, B, K, seed], hyper [lr, l2], opt (name)
  train_u / train_i             the training interactions (train_clicked_set as pairs)
  indptr / indices / data       the reference's build_adjmat CSR
  U0 / I0                       initial tables (xavier_uniform, LightGCN.py:122-128)
  uid, iid, uid2, iid2          two training batches (ids [B], [B, 1 + K])
  fwd_U / fwd_I                 the propagated tables of the initial model (LGCNEncoder.forward over every id)
  pred, loss, GU, GI            first batch: predictions, loss, both gradients
  U1, I1, U2, I2, losses        tables after each of two fit() iterations (BaseRunner._build_optimizer, the fit call order)
  eval_uid, eval_iid, eval_pred eval-mode predictions of a full-catalogue batch (model after the two iterations)
Graphs: Zipf item popularity, isolated users and items (rows 0 and a few more), an item hub in every case (longer than the default
chunk, so the default plan splits it), of degree >= 1,000 in the d32 case.  The graphs are small so that each fixture stays well
under a megabyte: the tables are stored six times over.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402


def graph(rng, n_users, n_items, per_user, hub_degree):
    """{user: set(items)}: Zipf items, users 1..n_users-1 minus a few isolated ones, item 1 clicked by hub_degree users"""
    pop = 1.0 / np.arange(1, n_items)
    pop /= pop.sum()
    clicked = {}
    isolated_users = set(rng.choice(np.arange(2, n_users), size=5, replace=False).tolist())
    isolated_items = set(range(n_items - 4, n_items))
    for u in range(1, n_users):
        if u in isolated_users:
            continue
        k = int(rng.integers(1, per_user + 1))
        items = set(int(x) for x in rng.choice(np.arange(1, n_items), size=k, p=pop)) - isolated_items
        clicked[u] = items
    hub_users = rng.choice(np.arange(1, n_users), size=hub_degree, replace=False)
    for u in hub_users:
        if int(u) not in isolated_users:
            clicked.setdefault(int(u), set()).add(1)
    return {u: s for u, s in clicked.items() if s}


def make_case(name, n_users, n_items, hub, d, L, B, K, opt, lr, l2, seed):
    torch, _, BaseRunner = make_golden._import_reference()
    from models.general.LightGCN import LightGCN
    rng = np.random.default_rng(seed)
    clicked = graph(rng, n_users, n_items, 12, hub)
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=K, dropout=0, test_all=0,
                           emb_size=d, n_layers=L)
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, train_clicked_set=clicked)

    def build():
        cuda = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self
        try:
            torch.manual_seed(seed)
            return LightGCN(args, corpus)
        finally:
            torch.Tensor.cuda = cuda

    model = build()
    adj = model.norm_adj
    out = {"meta": np.array([n_users, n_items, d, L, B, K, seed], dtype=np.int64), "hyper": np.array([lr, l2], dtype=np.float64),
           "opt": np.array(opt), "indptr": adj.indptr.astype(np.int64), "indices": adj.indices.astype(np.int32),
           "data": adj.data.copy(),
           "train_u": np.array([u for u in sorted(clicked) for _ in sorted(clicked[u])], dtype=np.int64),
           "train_i": np.array([i for u in sorted(clicked) for i in sorted(clicked[u])], dtype=np.int64)}
    emb = model.encoder.embedding_dict
    U0, I0 = emb["user_emb"].detach().numpy().copy(), emb["item_emb"].detach().numpy().copy()
    out.update(U0=U0, I0=I0)

    def batch():
        pi = 1.0 / np.arange(1, n_items)
        pi /= pi.sum()
        uid = rng.integers(1, n_users, size=B)
        iid = rng.choice(np.arange(1, n_items), size=(B, 1 + K), p=pi)
        return uid.astype(np.int64), iid.astype(np.int64)

    uid, iid = batch()
    uid2, iid2 = batch()
    out.update(uid=uid, iid=iid, uid2=uid2, iid2=iid2)

    def feed(u, i):
        return {"user_id": torch.from_numpy(u), "item_id": torch.from_numpy(i), "batch_size": len(u), "phase": "train"}

    with torch.no_grad():
        fu, fi = model.encoder(torch.arange(n_users), torch.arange(n_items))
    out.update(fwd_U=fu.numpy().copy(), fwd_I=fi.numpy().copy())

    model.zero_grad()
    o = model(feed(uid, iid))
    pred = o["prediction"]
    loss = model.loss(o)
    loss.backward()
    out["pred"] = pred.detach().numpy().copy()
    out["loss"] = np.array(loss.item(), dtype=np.float32)
    out["GU"], out["GI"] = emb["user_emb"].grad.numpy().copy(), emb["item_emb"].grad.numpy().copy()

    m = build()
    runner = BaseRunner(make_golden._runner_args(BaseRunner, opt, lr, l2))
    m.optimizer = runner._build_optimizer(m)
    losses = []
    for step, (u, i) in enumerate(((uid, iid), (uid2, iid2)), 1):
        m.train()
        m.optimizer.zero_grad()
        od = m(feed(u, i))
        ls = m.loss(od)
        ls.backward()
        m.optimizer.step()
        losses.append(ls.item())
        e = m.encoder.embedding_dict
        out["U%d" % step], out["I%d" % step] = e["user_emb"].detach().numpy().copy(), e["item_emb"].detach().numpy().copy()
    out["losses"] = np.array(losses, dtype=np.float32)

    m.eval()
    eu = rng.integers(1, n_users, size=8).astype(np.int64)
    ei = np.concatenate([rng.integers(1, n_items, size=(8, 1)), np.tile(np.arange(1, n_items), (8, 1))], axis=1).astype(np.int64)
    with torch.no_grad():
        ep = m({"user_id": torch.from_numpy(eu), "item_id": torch.from_numpy(ei), "batch_size": 8, "phase": "test"})["prediction"]
    out.update(eval_uid=eu, eval_iid=ei, eval_pred=ep.numpy().copy())
    out["state_keys"] = np.array(sorted(m.state_dict().keys()))

    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB")


CASES = [
    # name,                       n_users, n_items, hub, d, L,  B, K, opt,       lr,   l2,   seed
    ("lightgcn_d64_l3_k1_adam",      300,   120,  220,  64, 3, 64, 1, "Adam",    1e-3, 1e-8, 31),   # the demo flags
    ("lightgcn_d32_l1_k4_sgd",      1050,   200, 1000,  32, 1, 48, 4, "SGD",     0.05, 0.0,  32),   # the hub of degree >= 1,000
    ("lightgcn_d128_l4_k9_adam",     140,    70,  110, 128, 4, 32, 9, "Adam",    1e-3, 1e-4, 33),   # weight decay on both tables
    ("lightgcn_d48_l2_k1_adagrad",   380,   150,  280,  48, 2, 40, 1, "Adagrad", 0.01, 0.0,  34),
    ("lightgcn_d64_l0_k1_adam",      300,   120,  220,  64, 0, 40, 1, "Adam",    1e-3, 0.0,  35),   # n_layers 0: MF on the raw tables
]

if __name__ == "__main__":
    for c in CASES:
        make_case(*c)
