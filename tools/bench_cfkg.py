"""CFKG on the HIP engine: the fused front against the same head in torch ops, and the whole row-wise Adam step against the same
step with dense torch.optim.Adam, on one GPU; prints ONE JSON line (and writes it to --out, default profiles/cfkg_bench.json).

    python tools/bench_cfkg.py [--batches 65536] [--d 64] [--n_rel 4] [--users 1000001 --entities 1000001] [--out FILE]

Every figure is a HIP-event time of warm calls, accumulated over at least --seconds (0.5) per shape and route; the two routes of a
comparison alternate block by block in the same process (tools/bench_fpmc.py's protocol).  Ids are Zipf-like (p ~ 1 / k over the
users for "buy" heads, over the entities otherwise), so hot rows repeat inside a batch.  Per batch size:
  front    front_ms: rc_cfkg_fwd_bwd alone (both launches: the four gradient rows per row, loss_vec, the dense relation gradient);
           fused_ms: the same + rc_reduce_sum (the loss);  torch_ms: the same head in torch ops -- HipEmbedding's gather kernel for
           the [B, 4] heads, tails and relations, the reference's expression, MarginRankingLoss, torch.autograd.grad to the gathered
           rows (per-occurrence gradients);
           rc_cfkg_fwd_bwd's algorithmic bytes (4 rows read + 4 rows written + 5 ids per row) over front_ms as a fraction of
           8 TB/s -- a whole-call figure from HIP events over its two launches, not a kernel-trace time
  step     rowwise_adam_ms: CfkgTrainer.step (Adam, the demo line's lr and l2);  dense_adam_ms: nn.cfkg_scores + the loss in torch
           ops + backward + torch.optim.Adam over both tables
bench.py is not involved.  Not measured here: kernel traces, Grocery metrics.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_fpmc import HBM_PEAK, alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536")
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--n_rel", type=int, default=4)
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--users", type=int, default=1000001)
    ap.add_argument("--entities", type=int, default=1000001)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--parts", default="front,step", help="which measurements to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfkg_bench.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    import torch
    from rechorus_amd import engine, nn as hnn
    if not torch.cuda.is_available():
        raise SystemExit("bench_cfkg.py measures on the GPU only")
    dev = torch.device("cuda:0")
    d, n_rel, margin = a.d, a.n_rel, a.margin
    n_rows = a.users + a.entities
    gen = torch.Generator(device=dev).manual_seed(2)
    E = torch.randn((n_rows, d), device=dev, generator=gen) * 0.1
    R = torch.randn((n_rel, d), device=dev, generator=gen) * 0.1
    out = {"bench": "cfkg", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "d": d, "n_rel": n_rel, "margin": margin,
           "users": a.users, "entities": a.entities, "ids": "zipf", "hbm_peak_tbps": HBM_PEAK / 1e12,
           "rows_per_workgroup": engine.cfkg_fwd_bwd_rows_per_block(d), "front": {}, "step": {},
           "not_measured": ["kernel traces", "Grocery metrics"]}
    rel_diff = lambda x, y: float((x.detach() - y.detach()).abs().max() / y.detach().abs().max().clamp_min(1e-30))

    def zipf(n, size):
        """ids in [1, n) with p(k) ~ 1 / k"""
        u = torch.rand(size, device=dev, generator=gen)
        return torch.exp(u * math.log(n - 1)).long().clamp_(1, n - 1)

    def feed(bs):
        r = torch.randint(0, n_rel, (bs,), device=dev, generator=gen)
        buy = r == 0
        h = torch.where(buy, zipf(a.users, (bs,)), a.users + zipf(a.entities, (bs,)))
        hn = torch.where(buy, zipf(a.users, (bs,)), a.users + zipf(a.entities, (bs,)))
        t, tn = a.users + zipf(a.entities, (bs,)), a.users + zipf(a.entities, (bs,))
        head, tail = torch.stack((h, h, h, hn), 1).contiguous(), torch.stack((t, t, tn, t), 1).contiguous()
        return head, tail, r[:, None].repeat(1, 4).contiguous(), (h, t, hn, tn, r)

    loss_fn = torch.nn.MarginRankingLoss(margin=margin)

    for bs in (int(x) for x in a.batches.split(",")):
        head, tail, rel, cols = feed(bs)
        inv_b = 1.0 / bs
        ones = torch.ones(2 * bs, device=dev)

        def front_only():
            return engine.cfkg_fwd_bwd(E, R, *cols, margin=margin, inv_b=inv_b, want_pred=False)

        def fused():
            _, lv, rows, GR = front_only()
            return engine.reduce_sum(lv, inv_b), rows, GR

        def torch_head():
            hv = engine.gather_rows(E, head).requires_grad_(True)
            tv = engine.gather_rows(E, tail).requires_grad_(True)
            rv = engine.gather_rows(R, rel).requires_grad_(True)
            pred = -((hv + rv - tv) ** 2).sum(-1)
            loss = loss_fn(pred[:, :2].flatten(), pred[:, 2:].flatten(), ones)
            return (loss,) + torch.autograd.grad(loss, (hv, tv, rv))
        if "front" in parts:
            res = {"B": bs, "distinct_rows": int(torch.unique(torch.stack(cols[:4])).numel())}
            res["front_ms"], res["fused_ms"], res["torch_ms"] = alternate([front_only, fused, torch_head], a.seconds, block=3, warmup=2)
            res["speedup"] = res["torch_ms"] / res["fused_ms"]
            f, t = fused(), torch_head()
            # the torch side leaves one gradient row per (b, c): h's is columns 0 + 1 + 2 of the head rows, t''s column 2 of the tails
            res["loss_rel_diff"] = "%.3e" % rel_diff(f[0].reshape(()), t[0])
            res["gh_rel_diff"] = "%.3e" % rel_diff(f[1][:, 0], t[1][:, :3].sum(1))
            res["gtn_rel_diff"] = "%.3e" % rel_diff(f[1][:, 3], t[2][:, 2])
            nbytes = bs * (8 * 4 * d + 5 * 8)
            res["algorithmic_bytes"] = nbytes
            res["fraction_of_hbm_peak"] = nbytes / (res["front_ms"] * 1e-3) / HBM_PEAK
            out["front"][str(bs)] = res

    if "step" in parts:
        lr, l2 = 1e-4, 1e-6
        Er, Rr = E.clone(), R.clone()
        trainer = engine.CfkgTrainer(Er, Rr, margin=margin, opt="Adam", lr=lr, l2=l2)
        Ed, Rd = torch.nn.Parameter(E.clone()), torch.nn.Parameter(R.clone())
        optim = torch.optim.Adam([Ed, Rd], lr=lr, weight_decay=l2)
        for bs in (int(x) for x in a.batches.split(",")):
            head, tail, rel, _ = feed(bs)
            ones = torch.ones(2 * bs, device=dev)

            def dense():
                optim.zero_grad(set_to_none=True)
                pred = hnn.cfkg_scores(Ed, Rd, head, tail, rel)
                loss = loss_fn(pred[:, :2].flatten(), pred[:, 2:].flatten(), ones)
                loss.backward()
                optim.step()
                return loss
            row_ms, dense_ms = alternate([lambda: trainer.step(head, tail, rel), dense], a.seconds, block=3, warmup=2)
            out["step"][str(bs)] = {"B": bs, "rowwise_adam_ms": row_ms, "dense_adam_ms": dense_ms, "dense_over_rowwise": dense_ms / row_ms}

    def rnd(o):
        if isinstance(o, dict):
            return {k: rnd(v) for k, v in o.items()}
        return round(o, 5) if isinstance(o, float) and abs(o) < 1e6 else o
    line = json.dumps(rnd(out))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
