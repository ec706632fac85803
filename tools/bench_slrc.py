"""SLRC+ on the HIP engine: the fused front against the same head in torch ops, the seven-table item update against the existing
row-wise entry point that covers one of its seven tables, and the whole row-wise Adam step, on one GPU; prints ONE JSON line (and
writes it to --out, default profiles/slrc_bench.json).

    python tools/bench_slrc.py [--batches 65536] [--d 64] [--R 3] [--K 99] [--users 1000001 --items 1000001] [--out FILE]

Every figure is a HIP-event time of warm calls, accumulated over at least --seconds (0.5) per shape and route; the two routes of a
comparison alternate block by block in the same process (tools/bench_fpmc.py's protocol).  Per batch size:
  front    fused_ms: rc_slrc_fwd_bwd + rc_reduce_sum (scores, loss, gpred, ugrad, ubgrad, hgrad, gagrad);  torch_ms: the same head in
           torch ops on gathered rows -- five [B, C, R] lookups, the two torch.distributions log_probs, the broadcast product,
           GeneralModel.loss -- and torch.autograd.grad to the gathered rows (the per-occurrence gradients the fused kernel leaves);
           the fused kernel's algorithmic bytes (I rows, intervals, five Hawkes rows in; gpred and hgrad out) over its time as a
           fraction of 8 TB/s
  item     fused_ms: rc_slrc_item_update (SGD, in place: I, item_bias and the five Hawkes tables) on the sorted candidate ids;
           i_only_ms: rc_segmented_update on I alone (coef = gpred, src = U through uid, div = C) with the same head list -- the one
           of the seven tables an existing row-wise entry point covers at this size (rc_small_row_sums stops at 32,768 ids, the
           segmented update starts at d = 16)
  step     rowwise_ms: SlrcTrainer.step (Adam, the demo line's lr and l2)
bench.py is not involved.  Not measured here: kernel traces, Grocery metrics.
"""
import argparse
import json
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
    ap.add_argument("--R", type=int, default=3)
    ap.add_argument("--K", type=int, default=99)
    ap.add_argument("--users", type=int, default=1000001)
    ap.add_argument("--items", type=int, default=1000001)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--parts", default="front,item,step", help="which measurements to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slrc_bench.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    import torch
    from rechorus_amd import engine
    if not torch.cuda.is_available():
        raise SystemExit("bench_slrc.py measures on the GPU only")
    dev = torch.device("cuda:0")
    d, R, Cn = a.d, a.R, a.K + 1
    gen = torch.Generator(device=dev).manual_seed(2)
    rnd_ = lambda *shape, sd=0.1: torch.randn(shape, device=dev, generator=gen) * sd
    P = [rnd_(a.users, d), rnd_(a.items, d), rnd_(a.users, 1), rnd_(a.items, 1), torch.full((1,), 0.1, device=dev)] + \
        [rnd_(a.items, R, sd=0.2) for _ in range(5)]
    U, I, ub, ib, ga, alphas, pis, betas, sigmas, mus = P
    out = {"bench": "slrc", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "d": d, "R": R, "K": a.K, "users": a.users,
           "items": a.items, "hbm_peak_tbps": HBM_PEAK / 1e12, "layout": engine.slrc_fwd_bwd_layout(d, Cn, R), "front": {}, "item": {},
           "step": {}, "not_measured": ["kernel traces", "Grocery metrics"]}
    rel = lambda x, y: float((x.detach() - y.detach()).abs().max() / y.detach().abs().max().clamp_min(1e-30))

    for bs in (int(x) for x in a.batches.split(",")):
        uid = torch.randint(1, a.users, (bs,), device=dev, generator=gen)
        iid = torch.randint(1, a.items, (bs, Cn), device=dev, generator=gen)
        iv = torch.where(torch.rand((bs, Cn, R), device=dev, generator=gen) < 0.7, torch.full((), -1.0, device=dev),
                         torch.rand((bs, Cn, R), device=dev, generator=gen) * 3)
        inv_b = 1.0 / bs

        def fused():
            _, lv, g, ug, ubg, hg, gag = engine.slrc_fwd_bwd(P, uid, iid, iv, inv_b, want_pred=False)
            return engine.reduce_sum(lv, inv_b), g, ug

        def torch_head():
            rows = [U[uid].requires_grad_(True), I[iid].requires_grad_(True), ub[uid].requires_grad_(True), ib[iid].requires_grad_(True)] + \
                   [t[iid].requires_grad_(True) for t in (alphas, pis, betas, sigmas, mus)]
            u, i, b_u, b_i, al, pi, be, si, mu = rows
            mask = (iv >= 0).float()
            dt = iv * mask
            be_c, si_c = (be + 1).clamp(min=1e-10, max=10), (si + 1).clamp(min=1e-10, max=10)
            e = torch.distributions.exponential.Exponential(be_c, validate_args=False).log_prob(dt).exp()
            n = torch.distributions.normal.Normal(mu + 1, si_c, validate_args=False).log_prob(dt).exp()
            exc = ((ga + al) * ((pi + 0.5) * e + (0.5 - pi) * n) * mask).sum(-1)
            pred = (u[:, None, :] * i).sum(-1) + b_u + b_i.squeeze(-1) + exc
            pos, neg = pred[:, 0], pred[:, 1:]
            w = (neg - neg.max()).softmax(dim=1)
            loss = -(((pos[:, None] - neg).sigmoid() * w).sum(dim=1)).clamp(min=1e-8, max=1 - 1e-8).log().mean()
            grads = torch.autograd.grad(loss, rows)
            return loss, None, grads[0]
        if "front" in parts:
            res = {"B": bs}
            res["fused_ms"], res["torch_ms"] = alternate([fused, torch_head], a.seconds, block=3, warmup=2)
            res["speedup"] = res["torch_ms"] / res["fused_ms"]
            f, t = fused(), torch_head()
            # (the torch side carries this difference: against the same head in float64 the fused kernel's ugrad is within 4e-7,
            # torch's fp32 ops within 4e-4 -- DESIGN.md 7j)
            res["loss_rel_diff"], res["ugrad_rel_diff"] = "%.3e" % rel(f[0], t[0]), "%.3e" % rel(f[2], t[2])
            nbytes = bs * (4 * d + Cn * (4 * d + 8 + 4 * R + 5 * 4 * R + 4 + 5 * 4 * R))
            res["algorithmic_bytes"] = nbytes
            res["fraction_of_hbm_peak"] = nbytes / (res["fused_ms"] * 1e-3) / HBM_PEAK
            out["front"][str(bs)] = res
        if "item" in parts:
            _, _, gpred, _, _, hgrad, _ = engine.slrc_fwd_bwd(P, uid, iid, iv, inv_b, want_pred=False)
            keys, perm = engine.sort_ids(iid, a.items)
            _, heads, n_heads = engine.segment_heads(keys, perm, want_single=False)
            h = engine.make_hyper("SGD", lr=1e-9, l2=0.0)     # a tiny step: the tables stay where they are over thousands of calls
            flat = gpred.reshape(-1)
            W = [I, ib, alphas, pis, betas, sigmas, mus]

            def item_fused():
                engine.slrc_item_update(keys, perm, heads, n_heads, gpred, hgrad, U, uid, hyper=h, W=W)

            def item_i_only():
                engine.segmented_update(keys, perm, U, hyper=h, W=I, coef=flat, src_index=uid, div=Cn, heads=heads, n_heads=n_heads)
            res = {"B": bs, "n_occ": bs * Cn, "distinct_rows": int(n_heads.item())}
            res["fused_ms"], res["i_only_ms"] = alternate([item_fused, item_i_only], a.seconds)
            res["seven_tables_over_one"] = res["fused_ms"] / res["i_only_ms"]
            GA = [torch.zeros_like(w) for w in W]
            engine.slrc_item_update(keys, perm, heads, n_heads, gpred, hgrad, U, uid, dense_grad=GA)
            GC = torch.zeros_like(I)
            engine.segmented_update(keys, perm, U, coef=flat, src_index=uid, div=Cn, dense_grad=GC, heads=heads, n_heads=n_heads)
            res["max_rel_diff_I"] = "%.3e" % rel(GA[0], GC)
            del GA, GC
            out["item"][str(bs)] = res

    if "step" in parts:
        trainer = engine.SlrcTrainer(*P, opt="Adam", lr=5e-4, l2=1e-5)
        for bs in (int(x) for x in a.batches.split(",")):
            uid = torch.randint(1, a.users, (bs,), device=dev, generator=gen)
            iid = torch.randint(1, a.items, (bs, Cn), device=dev, generator=gen)
            iv = torch.where(torch.rand((bs, Cn, R), device=dev, generator=gen) < 0.7, torch.full((), -1.0, device=dev),
                             torch.rand((bs, Cn, R), device=dev, generator=gen) * 3)
            (ms,) = alternate([lambda: trainer.step(uid, iid, iv)], a.seconds, block=3, warmup=2)
            out["step"][str(bs)] = {"B": bs, "rowwise_adam_ms": ms}

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
