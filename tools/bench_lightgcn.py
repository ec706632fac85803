"""LightGCN propagation on the HIP engine vs torch's sparse route, on one GPU; prints ONE JSON line.

    python tools/bench_lightgcn.py [--shapes grocery,amazon_book,zipf_large] [--d 64] [--layers 3] [--iters 20]

For each shape (Grocery 14,681 users / 8,713 items / ~120 K interactions; Amazon-Book 52,643 / 91,599 / 2,984,108; a Zipf graph of
2 M users / 1 M items / 30 M interactions, a 768 MB table past the 256 MB Infinity Cache) it times, with HIP events:
  fwd / bwd         rc_lgcn_propagate_fwd / _bwd (L products + epilogues)
  step_eager        one training step of the LightGCN model file (propagate, BPR scores, loss, backward, dense Adam), eager
  step_replayed     the same step replayed from a hipGraph (rechorus_amd/graph.py)
  torch_fwd         the reference's encoder restated in torch (torch.cat, L torch.sparse.mm, stack, mean) on the same GPU
Per SpMM: edge bytes nnz * (d * 4 + 8) (one gathered row + column id + value per edge), compulsory bytes (CSR once, the [N, d]
input read once and output written once), and the fraction of 8 TB/s those edge bytes reach.  bench.py is not involved.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

SHAPES = {"grocery": (14681, 8713, 120000), "amazon_book": (52643, 91599, 2984108), "zipf_large": (2000000, 1000000, 30000000)}
PEAK_BPS = 8e12


def interactions(n_users, n_items, n_inter, seed=0):
    """n_inter distinct (user, item) pairs: Zipf item popularity, uniform users"""
    rng = np.random.default_rng(seed)
    keys = np.empty(0, dtype=np.int64)
    while keys.size < n_inter:
        m = int((n_inter - keys.size) * 1.3) + 1000
        u = rng.integers(1, n_users, m)
        i = (rng.zipf(1.15, m) - 1) % (n_items - 1) + 1
        keys = np.unique(np.concatenate([keys, u * n_items + i]))
    keys = rng.choice(keys, n_inter, replace=False)
    return keys // n_items, keys % n_items


def timed(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def bench_shape(name, d, L, iters, batch):
    import torch
    from helpers.BaseRunner import BaseRunner
    from models.general.LightGCN import LightGCN
    from rechorus_amd import engine, graph as hgraph
    dev = torch.device("cuda:0")
    n_users, n_items, n_inter = SHAPES[name]
    t0 = time.time()
    u, i = interactions(n_users, n_items, n_inter)
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=d, n_layers=L)
    m = LightGCN(args, SimpleNamespace(n_users=n_users, n_items=n_items, train_clicked_set=(u, i))).to(dev)
    host_s = time.time() - t0
    g = m.encoder.graph()
    U, I = m.encoder.embedding_dict["user_emb"], m.encoder.embedding_dict["item_emb"]
    N, nnz = g.N, g.nnz
    res = {"users": n_users, "items": n_items, "interactions": n_inter, "nnz": nnz, "d": d, "n_layers": L, "chunk": g.chunk,
           "long_rows": int(g.tensors["long_row"].numel()), "max_degree": int(np.diff(g.tensors["indptr"].cpu().numpy()).max()),
           "host_build_s": round(host_s, 2)}
    GU = torch.randn(n_users, d, device=dev) * 1e-3
    GI = torch.randn(n_items, d, device=dev) * 1e-3
    res["fwd_ms"] = timed(lambda: engine.lgcn_propagate_fwd(g, U.detach(), I.detach(), L, out="persistent"), iters)
    res["bwd_ms"] = timed(lambda: engine.lgcn_propagate_bwd(g, GU, GI, L), iters)
    # torch's route of the reference encoder (LightGCN.py:137-151) on the same graph
    t = g.tensors
    rows = torch.repeat_interleave(torch.arange(N, device=dev), torch.diff(t["indptr"]))
    A = torch.sparse_coo_tensor(torch.stack([rows, t["indices"].long()]), t["values"], (N, N)).coalesce()

    def torch_fwd():
        ego = torch.cat([U.detach(), I.detach()], 0)
        embs = [ego]
        for _ in range(L):
            ego = torch.sparse.mm(A, ego)
            embs.append(ego)
        return torch.stack(embs, 1).mean(1)
    res["torch_fwd_ms"] = timed(torch_fwd, iters)
    ref = torch_fwd()
    ours = engine.lgcn_propagate_fwd(g, U.detach(), I.detach(), L)
    res["max_abs_diff_vs_torch"] = "%.3e" % float((ref - ours).abs().max())
    res["max_abs_torch"] = "%.3e" % float(ref.abs().max())
    del ref, ours
    edge_b = nnz * (d * 4 + 8)
    comp_b = (N + 1) * 8 + nnz * 8 + 2 * N * d * 4
    per = res["fwd_ms"] / max(L, 1) * 1e-3
    res.update(spmm_edge_bytes=edge_b, spmm_compulsory_bytes=comp_b, spmm_ms_est=round(per * 1e3, 4),
               spmm_edge_frac_of_8TBps=round(edge_b / per / PEAK_BPS, 3) if L else None,
               speedup_fwd_vs_torch=round(res["torch_fwd_ms"] / res["fwd_ms"], 2))
    # the training step of the model file, eager and replayed
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.train, a.log_file = 1, "/tmp/rc_bench_lightgcn/log.txt"
    a.optimizer, a.lr, a.l2, a.engine = "Adam", 1e-3, 1e-8, "dense"
    m.optimizer = BaseRunner(a)._build_optimizer(m)
    m.train()
    rng = np.random.default_rng(1)
    feed = {"user_id": torch.from_numpy(rng.integers(1, n_users, batch)).to(dev),
            "item_id": torch.from_numpy(rng.integers(1, n_items, (batch, 2))).to(dev), "batch_size": batch, "phase": "train"}

    def eager():
        m.optimizer.zero_grad()
        m.loss(m(feed)).backward()
        m.optimizer.step()
    res["step_eager_ms"] = timed(eager, iters)
    if hgraph.usable():
        step = hgraph.GraphedStep(m)
        res["step_replayed_ms"] = timed(lambda: step.run(feed), iters)
    for k, v in list(res.items()):
        if isinstance(v, float):
            res[k] = round(v, 4)
    del m, A, rows
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="grocery,amazon_book,zipf_large")
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    out = {"bench": "lightgcn", "peak_TBps": PEAK_BPS / 1e12, "shapes": {}}
    for s in a.shapes.split(","):
        out["shapes"][s] = bench_shape(s, a.d, a.layers, a.iters, a.batch)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
