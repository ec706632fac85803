"""FPMC on the HIP engine: the two new kernels against the composition of existing entry points they replace, and the whole row-wise
step against the same step in torch ops over HipEmbedding lookups, on one GPU; prints ONE JSON line (and writes it to --out).

    python tools/bench_fpmc.py [--batches 256,4096,65536] [--d 64] [--K 99] [--users 1000001 --items 10000001] [--out FILE]

Every figure is a HIP-event time of warm calls, accumulated over at least --seconds (0.5) per shape and route; the two routes of a
comparison alternate block by block in the same process.  Per batch size:
  front    fused_ms: rc_fpmc_fwd_bwd + rc_reduce_sum (scores, loss, gpred, ugrad, lgrad);  composed_ms: rc_gather_dot_fwd x 2, an
           add, rc_bpr_loss_fwd_bwd (+ rc_reduce_sum), rc_weighted_row_sum x 2 -- every candidate row read twice;  the fused
           kernel's algorithmic gather bytes (2 + 2 C) * 4 d * B over its time as a fraction of 8 TB/s
  item     fused_ms: rc_fpmc_item_update (SGD, in place) on the sorted candidate ids;  composed_ms: two rc_segmented_update calls
           (coef = gpred, src = UI / LI through uid / lid, div = C) with the same head list -- the sorted ids walked twice
  step     rowwise_ms: FpmcTrainer.step (Adam);  torch_ms: four HipEmbedding lookups, the two broadcast products, GeneralModel.loss,
           backward and torch.optim.Adam over the same tables (dense semantics, the reference's step)
The verdict per kernel compares the B = 65,536 speed-up with the +-7 % box-to-box spread the README states.  bench.py is not involved.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))

HBM_PEAK = 8.0e12
SPREAD = 0.07


def alternate(fns, seconds, block=5, warmup=3):
    """ms per call of every fn: blocks of `block` calls, the routes taking turns, until each has run for `seconds`"""
    import torch
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    total, calls = [0.0] * len(fns), [0] * len(fns)
    while min(total) < seconds * 1e3:
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(block):
                fn()
            b.record()
            torch.cuda.synchronize()
            total[k] += a.elapsed_time(b)
            calls[k] += block
    return [t / c for t, c in zip(total, calls)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,4096,65536")
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--K", type=int, default=99)
    ap.add_argument("--users", type=int, default=1000001)
    ap.add_argument("--items", type=int, default=10000001)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--parts", default="front,item,step", help="which comparisons to run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    parts = a.parts.split(",")
    import torch
    from rechorus_amd import engine, nn as hnn
    if not torch.cuda.is_available():
        raise SystemExit("bench_fpmc.py measures on the GPU only")
    dev = torch.device("cuda:0")
    d, Cn = a.d, a.K + 1
    gen = torch.Generator(device=dev).manual_seed(2)
    emb = {}
    for name, rows in (("UI", a.users), ("LI", a.items), ("IU", a.items), ("IL", a.items)):
        emb[name] = hnn.HipEmbedding(rows, d).to(dev)
        with torch.no_grad():
            emb[name].weight.copy_(torch.randn((rows, d), device=dev, generator=gen) * 0.1)
    UI, LI, IU, IL = (emb[k].weight.data for k in ("UI", "LI", "IU", "IL"))
    out = {"bench": "fpmc", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "d": d, "K": a.K, "users": a.users,
           "items": a.items, "hbm_peak_tbps": HBM_PEAK / 1e12, "layout": engine.fpmc_fwd_bwd_layout(d, Cn), "front": {}, "item": {},
           "step": {}}
    rel = lambda x, y: "%.3e" % float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))

    for bs in (int(x) for x in a.batches.split(",")):
        uid = torch.randint(1, a.users, (bs,), device=dev, generator=gen)
        lid = torch.randint(1, a.items, (bs,), device=dev, generator=gen)
        iid = torch.randint(1, a.items, (bs, Cn), device=dev, generator=gen)
        inv_b = 1.0 / bs

        # ---- forward + loss + backward to the query rows
        def fused():
            _, lv, g, ug, lg = engine.fpmc_fwd_bwd(UI, LI, IU, IL, uid, lid, iid, inv_b, want_pred=False)
            return engine.reduce_sum(lv, inv_b), g, ug, lg

        def composed():
            pred = engine.gather_dot(UI, IU, uid, iid) + engine.gather_dot(LI, IL, lid, iid)
            loss, _, g = engine.bpr_loss(pred, inv_b)
            return loss, g, engine.weighted_row_sum(IU, iid, g), engine.weighted_row_sum(IL, iid, g)
        if "front" in parts:
            res = {"B": bs}
            res["fused_ms"], res["composed_ms"] = alternate([fused, composed], a.seconds)
            res["speedup"] = res["composed_ms"] / res["fused_ms"]
            res["max_rel_diff"] = max(rel(x, y) for x, y in zip(fused(), composed()))
            nbytes = (2 + 2 * Cn) * 4 * d * bs
            res["gather_bytes"] = nbytes
            res["fraction_of_hbm_peak"] = nbytes / (res["fused_ms"] * 1e-3) / HBM_PEAK
            out["front"][str(bs)] = res
        if "item" not in parts:
            continue

        # ---- item-side update of IU and IL (SGD with a tiny step: the tables stay where they are over thousands of calls)
        gpred = fused()[1]
        keys, perm = engine.sort_ids(iid, a.items)
        _, heads, n_heads = engine.segment_heads(keys, perm, want_single=False)
        h = engine.make_hyper("SGD", lr=1e-9, l2=0.0)
        flat = gpred.reshape(-1)

        def item_fused():
            engine.fpmc_item_update(keys, perm, heads, n_heads, gpred, UI, LI, uid, lid, hyper=h, IU=IU, IL=IL)

        def item_composed():
            engine.segmented_update(keys, perm, UI, hyper=h, W=IU, coef=flat, src_index=uid, div=Cn, heads=heads, n_heads=n_heads)
            engine.segmented_update(keys, perm, LI, hyper=h, W=IL, coef=flat, src_index=lid, div=Cn, heads=heads, n_heads=n_heads)
        res = {"B": bs, "n_occ": bs * Cn, "distinct_rows": int(n_heads.item())}
        res["fused_ms"], res["composed_ms"] = alternate([item_fused, item_composed], a.seconds)
        res["speedup"] = res["composed_ms"] / res["fused_ms"]
        GA, GB = torch.zeros_like(IU), torch.zeros_like(IL)
        engine.fpmc_item_update(keys, perm, heads, n_heads, gpred, UI, LI, uid, lid, dense_grad=(GA, GB))
        GC = torch.zeros_like(IU)
        engine.segmented_update(keys, perm, UI, coef=flat, src_index=uid, div=Cn, dense_grad=GC, heads=heads, n_heads=n_heads)
        res["max_rel_diff"] = rel(GA, GC)
        del GA, GB, GC
        out["item"][str(bs)] = res

    # ---- the whole step (after the kernel comparisons: Adam's state and the dense gradients take 5x the tables' memory)
    params = [emb[k].weight for k in ("UI", "LI", "IU", "IL")]
    trainer = engine.FpmcTrainer(UI, LI, IU, IL, opt="Adam", lr=1e-3, l2=1e-6) if "step" in parts else None
    optim = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-6)
    for bs in (int(x) for x in a.batches.split(",") if "step" in parts):
        uid = torch.randint(1, a.users, (bs,), device=dev, generator=gen)
        lid = torch.randint(1, a.items, (bs,), device=dev, generator=gen)
        iid = torch.randint(1, a.items, (bs, Cn), device=dev, generator=gen)

        def rowwise():
            return trainer.step(uid, lid, iid)

        def torch_step():
            optim.zero_grad()
            iu, il = emb["IU"](iid), emb["IL"](iid)
            pred = (emb["UI"](uid)[:, None, :] * iu).sum(-1) + (emb["LI"](lid)[:, None, :] * il).sum(-1)
            pos, neg = pred[:, 0], pred[:, 1:]
            w = (neg - neg.max()).softmax(dim=1)
            loss = -(((pos[:, None] - neg).sigmoid() * w).sum(dim=1)).clamp(min=1e-8, max=1 - 1e-8).log().mean()
            loss.backward()
            optim.step()
            return loss
        res = {"B": bs}
        res["rowwise_ms"], res["torch_ms"] = alternate([rowwise, torch_step], a.seconds, block=3, warmup=2)
        res["speedup"] = res["torch_ms"] / res["rowwise_ms"]
        out["step"][str(bs)] = res

    top = str(max(int(x) for x in a.batches.split(",")))
    out["verdict"] = {}
    for kind in ("front", "item"):
        if kind not in parts:
            continue
        s = out[kind][top]["speedup"]
        out["verdict"][kind] = ("win" if s > 1 + SPREAD else "loss") + ": %.2fx at B = %s against the composition (bar: more than %.2fx)" % (s, top, 1 + SPREAD)

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
