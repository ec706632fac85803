"""Chorus on the HIP engine: the fused stage-2 front, the category update and the whole row-wise step of both stages, each beside the
same expression in torch ops (dense torch.optim for the steps), on one GPU; prints ONE JSON line (and writes it to --out, default
profiles/chorus_bench.json).

    python tools/bench_chorus.py [--batches 256,4096,65536] [--d 64] [--R 3] [--K 99] [--users 1000001 --items 1000001]
                                 [--cats 1,300] [--out FILE]

Every figure is a HIP-event time of warm calls, accumulated over at least --seconds (0.3) per shape and route; the two routes of a
comparison alternate block by block in the same process (tools/bench_fpmc.py's protocol).  Per batch size and category count:
  front     fused_ms: rc_chorus_fwd_bwd + rc_reduce_sum (scores, loss, gpred, coef, ugrad, ubgrad, kgrad, GRel);  torch_ms: the same
            head in torch ops on gathered rows (z = (1 + S) i + decay Rel, GeneralModel.loss) and torch.autograd.grad to the gathered
            rows and Rel; the fused kernel's algorithmic bytes (I rows once, ids, intervals in; gpred, coef, kgrad out) over its time
            as a fraction of 8 TB/s
  category  fused_ms: rc_chorus_category_update (SGD, in place) on the sorted category ids, the sort and head list not included;
            torch_ms: index_add_ of kgrad into a [n_cat, 3 R] gradient (floating-point atomics) and the SGD axpy
  step2     rowwise_ms: ChorusTrainer.step (Adam, the demo flags);  torch_ms: the head in torch ops on nn.Parameters, backward, and
            dense torch.optim.Adam with the three parameter groups
  step1     rowwise_ms: CfkgTrainer.step on the exchanged feed (Adam);  torch_ms: TransE in torch ops, MarginRankingLoss, backward and
            dense torch.optim.Adam
bench.py is not involved.  Not measured here: kernel traces, Grocery metrics, the GMF head.  A full run takes about seven minutes, most
of it in the torch routes (the dense step with one category costs 6 s per call at B = 65,536).
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

LOG_SQRT_2PI = 0.9189385332046727


def torch_scores(u, i, rel, be, si, mu, ub_u, ib_i, iv, kinds):
    """the stage-2 BPR head on gathered rows: u [B, d], i [B, C, d], rel [R, d], be / si / mu [B, C, R]"""
    import torch
    on = iv >= 0
    dt = torch.where(on, iv, torch.zeros_like(iv))
    beta, sigma, m = (be + 1).clamp(min=1e-10, max=10), (si + 1).clamp(min=1e-10, max=10), mu + 1
    n = lambda x, mean, s: torch.exp(-(x - mean) ** 2 / (2 * s * s) - torch.log(s) - LOG_SQRT_2PI)
    cols = []
    for r, k in enumerate(kinds):
        b, s, mm, x = beta[..., r], sigma[..., r], m[..., r], dt[..., r]
        kappa = torch.exp(torch.log(b) - b * x) if k == 0 else (n(x, 0, b) if k == 1 else n(x, mm, s) - n(x, 0, b))
        cols.append(kappa.clamp(-1, 1))
    decay = torch.stack(cols, dim=2) * on
    z = (1 + decay.sum(-1, keepdim=True)) * i + decay @ rel
    return (u[:, None, :] * z).sum(-1) + ub_u + ib_i.squeeze(-1)


def bpr(pred):
    pos, neg = pred[:, 0], pred[:, 1:]
    w = (neg - neg.max()).softmax(dim=1)
    return -(((pos[:, None] - neg).sigmoid() * w).sum(dim=1)).clamp(min=1e-8, max=1 - 1e-8).log().mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,4096,65536")
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--R", type=int, default=3)
    ap.add_argument("--K", type=int, default=99)
    ap.add_argument("--users", type=int, default=1000001)
    ap.add_argument("--items", type=int, default=1000001)
    ap.add_argument("--cats", default="1,300")
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--parts", default="front,category,step2,step1", help="which measurements to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chorus_bench.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    import torch
    from rechorus_amd import engine
    if not torch.cuda.is_available():
        raise SystemExit("bench_chorus.py measures on the GPU only")
    dev = torch.device("cuda:0")
    d, R, Cn = a.d, a.R, a.K + 1
    kinds = ([0, 1, 2] * 3)[:R]
    gen = torch.Generator(device=dev).manual_seed(2)
    rnd_ = lambda *shape, sd=0.1: torch.randn(shape, device=dev, generator=gen) * sd
    U, I, Rel, w, ub, ib = rnd_(a.users, d), rnd_(a.items, d), rnd_(R, d), rnd_(1, d), rnd_(a.users, 1), rnd_(a.items, 1)
    out = {"bench": "chorus", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "d": d, "R": R, "K": a.K, "kinds": kinds,
           "users": a.users, "items": a.items, "hbm_peak_tbps": HBM_PEAK / 1e12, "tuples_per_workgroup": engine.chorus_front_tuples_per_block(),
           "piece": engine.chorus_category_piece(), "front": {}, "category": {}, "step2": {}, "step1": {}, "runs": 1,
           "not_measured": ["kernel traces", "Grocery metrics", "the GMF head"]}
    rel = lambda x, y: float((x.detach() - y.detach()).abs().max() / y.detach().abs().max().clamp_min(1e-30))
    margin = 1.0

    for n_cat in (int(x) for x in a.cats.split(",")):
        cat = [rnd_(n_cat, R, sd=0.2) for _ in range(3)]      # betas, mus, sigmas
        P = [U, I, Rel, cat[0], cat[1], cat[2], w, ub, ib]
        for bs in (int(x) for x in a.batches.split(",")):
            tag = f"n_cat={n_cat},B={bs}"
            uid = torch.randint(1, a.users, (bs,), device=dev, generator=gen)
            iid = torch.randint(1, a.items, (bs, Cn), device=dev, generator=gen)
            cid = torch.randint(0, n_cat, (bs, Cn), device=dev, generator=gen)
            iv = torch.where(torch.rand((bs, Cn, R), device=dev, generator=gen) < 0.7, torch.full((), -1.0, device=dev),
                             torch.rand((bs, Cn, R), device=dev, generator=gen) * 3)
            inv_b = 1.0 / bs

            def fused():
                o = engine.chorus_fwd_bwd(P, uid, iid, cid, iv, kinds, False, inv_b, want_pred=False)
                return engine.reduce_sum(o["loss_vec"], inv_b), o

            def torch_head():
                rows = [U[uid].requires_grad_(True), I[iid].requires_grad_(True), Rel.clone().requires_grad_(True)] + \
                       [t[cid].requires_grad_(True) for t in (cat[0], cat[2], cat[1])] + \
                       [ub[uid].requires_grad_(True), ib[iid].requires_grad_(True)]
                loss = bpr(torch_scores(*rows, iv, kinds))
                return loss, torch.autograd.grad(loss, rows)
            if "front" in parts:
                res = {"B": bs, "n_cat": n_cat}
                res["fused_ms"], res["torch_ms"] = alternate([fused, torch_head], a.seconds, block=3, warmup=2)
                res["speedup"] = res["torch_ms"] / res["fused_ms"]
                f, t = fused(), torch_head()
                res["loss_rel_diff"], res["ugrad_rel_diff"] = "%.3e" % rel(f[0], t[0]), "%.3e" % rel(f[1]["ugrad"], t[1][0])
                res["GRel_rel_diff"] = "%.3e" % rel(f[1]["GRel"], t[1][2])
                nbytes = bs * (4 * d + 8 + Cn * (4 * d + 8 + 8 + 4 * R + 4 + 4 + 3 * 4 * R))
                res["algorithmic_bytes"] = nbytes
                res["fraction_of_hbm_peak"] = nbytes / (res["fused_ms"] * 1e-3) / HBM_PEAK
                del f, t
                out["front"][tag] = res
            if "category" in parts:
                kgrad = engine.chorus_fwd_bwd(P, uid, iid, cid, iv, kinds, False, inv_b, want_pred=False)["kgrad"]
                keys, perm = engine.sort_ids(cid, n_cat)
                _, heads, n_heads = engine.segment_heads(keys, perm, want_single=False)
                h = engine.make_hyper("SGD", lr=1e-9, l2=0.0)     # a tiny step: the tables stay where they are over thousands of calls
                W = [cat[0], cat[2], cat[1]]
                flat = cid.reshape(-1)
                Wt = torch.cat(W, dim=1)

                def cat_fused():
                    engine.chorus_category_update(keys, perm, heads, n_heads, kgrad, n_cat, hyper=h, W=W)

                def cat_torch():
                    G = torch.zeros((n_cat, 3 * R), device=dev).index_add_(0, flat, kgrad)
                    Wt.add_(G, alpha=-1e-9)
                res = {"B": bs, "n_cat": n_cat, "n_occ": bs * Cn, "pieces": (bs * Cn + out["piece"] - 1) // out["piece"]}
                res["fused_ms"], res["torch_ms"] = alternate([cat_fused, cat_torch], a.seconds)
                res["speedup"] = res["torch_ms"] / res["fused_ms"]
                dense = [torch.zeros_like(t) for t in W]
                engine.chorus_category_update(keys, perm, heads, n_heads, kgrad, n_cat, dense_grad=dense)
                res["max_rel_diff"] = "%.3e" % rel(torch.cat(dense, dim=1), torch.zeros((n_cat, 3 * R), device=dev).index_add_(0, flat, kgrad))
                out["category"][tag] = res
            if "step2" in parts:
                trainer = engine.ChorusTrainer(*P, kinds=kinds, gmf=False, opt="Adam", lr=1e-3, l2=0.0, lr_scale=0.1)
                tp = [torch.nn.Parameter(t.clone()) for t in (U, I, Rel, cat[0], cat[2], cat[1], ub, ib)]
                opt = torch.optim.Adam([{"params": [tp[0], tp[3], tp[4], tp[5]]}, {"params": [tp[1], tp[2]], "lr": 1e-4},
                                        {"params": [tp[6], tp[7]], "weight_decay": 0.0}], lr=1e-3, weight_decay=0.0)

                def torch_step():
                    opt.zero_grad(set_to_none=False)
                    bpr(torch_scores(tp[0][uid], tp[1][iid], tp[2], tp[3][cid], tp[4][cid], tp[5][cid], tp[6][uid], tp[7][iid], iv,
                                     kinds)).backward()
                    opt.step()
                res = {"B": bs, "n_cat": n_cat}
                res["rowwise_adam_ms"], res["torch_dense_adam_ms"] = alternate(
                    [lambda: trainer.step(uid, iid, cid, iv), torch_step], a.seconds, block=2, warmup=2)
                res["speedup"] = res["torch_dense_adam_ms"] / res["rowwise_adam_ms"]
                del trainer, tp, opt
                out["step2"][tag] = res
        del cat, P

    if "step1" in parts:
        for bs in (int(x) for x in a.batches.split(",")):
            h, t, hn, tn = (torch.randint(1, a.items, (bs,), device=dev, generator=gen) for _ in range(4))
            r = torch.randint(1, R, (bs, 1), device=dev, generator=gen).expand(bs, 4).contiguous()
            head_id, tail_id = torch.stack((t, t, tn, t), dim=1), torch.stack((h, h, h, hn), dim=1)      # the reference's feed
            trainer = engine.CfkgTrainer(I.clone(), Rel.clone(), margin=margin, opt="Adam", lr=5e-4, l2=1e-5)
            tp = [torch.nn.Parameter(I.clone()), torch.nn.Parameter(Rel.clone())]
            opt = torch.optim.Adam(tp, lr=5e-4, weight_decay=1e-5)
            lossf = torch.nn.MarginRankingLoss(margin=margin)
            ones = torch.ones(2 * bs, device=dev)

            def rowwise():
                ch, ct = engine.chorus_kg_feed(head_id, tail_id)
                return trainer.step(ch, ct, r)

            def torch_step():
                opt.zero_grad(set_to_none=False)
                pred = -((tp[0][head_id] + tp[1][r] - tp[0][tail_id]) ** 2).sum(-1)
                lossf(pred[:, :2].flatten(), pred[:, 2:].flatten(), ones).backward()
                opt.step()
            res = {"B": bs}
            res["rowwise_adam_ms"], res["torch_dense_adam_ms"] = alternate([rowwise, torch_step], a.seconds, block=2, warmup=2)
            res["speedup"] = res["torch_dense_adam_ms"] / res["rowwise_adam_ms"]
            out["step1"][f"B={bs}"] = res
            del trainer, tp, opt

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
