"""BUIR on the HIP engine vs the same computation written with torch ops over HipEmbedding lookups (what a user's BUIR model file
gets through adopt_embeddings), on one GPU; prints ONE JSON line (and writes it to --out).

    python tools/bench_buir.py [--batches 256,4096,65536] [--d 64] [--users 1000001 --items 10000001] [--out FILE]

Every figure is a HIP-event time of warm calls, accumulated over at least --seconds (0.5) per shape and route; where two routes
are compared they alternate block by block in the same process.
  loss        per batch size: kernels_ms (rc_buir_fwd + rc_buir_bwd alone: loss, prediction, per-occurrence row gradients, dW,
              db), fused_ms / torch_ms (the autograd node / the torch-op route end to end: forward, backward, all four gradients,
              the two table gradients dense), and the kernels' share of peak: algorithmic flops 3 * 2 * (2B) * d^2 over the
              157.3 TF fp32 MFMA peak, algorithmic bytes (four row gathers, two row-gradient writes, the ids, each counted
              once although the backward launch gathers the rows again) over 8 TB/s, and which of the two bounds the kernels
  ema         rc_buir_ema on both table pairs: ms, GB/s on 12 * rows * d bytes against 8 TB/s, and the torch expression
              t * m + o * (1 - m) on the same tables
  step        the whole training step of the model (forward, backward, dense Adam, target update), eager and replayed from a
              hipGraph
bench.py is not involved.
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

HBM_PEAK = 8.0e12
MFMA_F32_PEAK = 157.3e12


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


def torch_loss(U_on, U_t, I_on, I_t, P, uid, iid):
    """BUIR.py:73-110 in torch ops; the tables are HipEmbedding modules"""
    import torch.nn.functional as F
    uo, io = U_on(uid), I_on(iid)
    ut, it = U_t(uid).detach(), I_t(iid).detach()
    pu, pi = P(uo), P(io)
    pred = (pi * uo).sum(-1) + (pu * io).sum(-1)
    l_ui = 2 - 2 * (F.normalize(pu, dim=-1) * F.normalize(it, dim=-1)).sum(-1)
    l_iu = 2 - 2 * (F.normalize(pi, dim=-1) * F.normalize(ut, dim=-1)).sum(-1)
    return (l_ui + l_iu).mean(), pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,4096,65536")
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--users", type=int, default=1000001)
    ap.add_argument("--items", type=int, default=10000001)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from helpers.BUIRRunner import BUIRRunner
    from models.general.BUIR import BUIR
    from rechorus_amd import engine, graph as hgraph, nn as hnn
    dev = torch.device("cuda:0")
    d = a.d
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=0, dropout=0, test_all=0, emb_size=d, momentum=0.995)
    torch.manual_seed(1)
    model = BUIR(args, SimpleNamespace(n_users=a.users, n_items=a.items)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(2)
    with torch.no_grad():      # tables away from the near-zero native init, targets beside their online tables
        for online, target in ((model.user_online, model.user_target), (model.item_online, model.item_target)):
            online.weight.copy_(torch.randn(online.weight.shape, device=dev, generator=gen) * 0.5)
            target.weight.copy_(online.weight + 0.1 * torch.randn(online.weight.shape, device=dev, generator=gen))
    tabs = (model.user_online.weight, model.user_target.weight, model.item_online.weight, model.item_target.weight)
    W, b = model.predictor.weight, model.predictor.bias
    det = [t.detach() for t in (*tabs, W, b)]
    params = (tabs[0], tabs[2], W, b)
    out = {"bench": "buir", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "d": d, "users": a.users,
           "items": a.items, "hbm_peak_tbps": HBM_PEAK / 1e12, "fp32_mfma_peak_tflops": MFMA_F32_PEAK / 1e12, "loss": {}, "step": {}}

    def zero():
        for p in params:
            p.grad = None

    one = torch.ones(1, device=dev)
    for bs in (int(x) for x in a.batches.split(",")):
        uid = torch.randint(1, a.users, (bs,), device=dev, generator=gen)
        iid = torch.randint(1, a.items, (bs,), device=dev, generator=gen)
        ws = engine.BuirWorkspace()
        res = {"B": bs}

        def kernels():
            engine.buir_fwd(*det, uid, iid, workspace=ws)
            engine.buir_bwd(one, *det, uid, iid, workspace=ws)

        def fused():
            zero()
            hnn.buir_loss(*tabs, W, b, uid, iid, workspace=ws)[0].backward()

        def torch_route():
            zero()
            torch_loss(model.user_online, model.user_target, model.item_online, model.item_target, model.predictor, uid, iid)[0].backward()
        res["kernels_ms"], = alternate([kernels], a.seconds)
        res["fused_ms"], res["torch_ms"] = alternate([fused, torch_route], a.seconds)
        fused()
        g_f = [p.grad.clone() for p in params]
        torch_route()
        res["max_rel_diff_vs_torch"] = "%.3e" % max(float((x - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30))
                                                    for x, p in zip(g_f, params))
        zero()
        res["fused_vs_torch_speedup"] = res["torch_ms"] / res["fused_ms"]
        flops = 3 * 2 * (2 * bs) * d * d
        nbytes = (4 + 2) * bs * d * 4 + 2 * 8 * bs      # four row gathers, two row-gradient writes, the ids (each counted once)
        sec = res["kernels_ms"] * 1e-3
        res["fraction_of_mfma_peak"] = flops / sec / MFMA_F32_PEAK
        res["fraction_of_hbm_peak"] = nbytes / sec / HBM_PEAK
        res["bound"] = "memory" if res["fraction_of_hbm_peak"] >= res["fraction_of_mfma_peak"] else "mfma"
        res["fraction_of_peak"] = max(res["fraction_of_hbm_peak"], res["fraction_of_mfma_peak"])
        out["loss"][str(bs)] = res

    # ---- target update
    m = 0.995

    def ema_kernel():      # (through .data, like the torch statement below, which binds a fresh tensor every time)
        engine.ema_update(model.user_target.weight.data, model.user_online.weight.data, model.item_target.weight.data,
                          model.item_online.weight.data, m)

    def ema_torch_rebind():      # the reference's own statement: a fresh tensor bound to .data
        model.user_target.weight.data = model.user_target.weight.data * m + model.user_online.weight.data * (1. - m)
        model.item_target.weight.data = model.item_target.weight.data * m + model.item_online.weight.data * (1. - m)
    k_ms, t_ms = alternate([ema_kernel, ema_torch_rebind], a.seconds, block=3, warmup=2)
    ema_bytes = 12.0 * (a.users + a.items) * d
    out["ema"] = {"kernel_ms": k_ms, "torch_ms": t_ms, "bytes": ema_bytes, "kernel_gbps": ema_bytes / (k_ms * 1e-3) / 1e9,
                  "fraction_of_hbm_peak": ema_bytes / (k_ms * 1e-3) / HBM_PEAK, "kernel_vs_torch_speedup": t_ms / k_ms}

    # ---- the whole step, eager and replayed (dense Adam over every table, as the runner does it)
    ra, _ = BUIRRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    ra.train, ra.log_file, ra.optimizer, ra.lr, ra.l2, ra.graph, ra.engine = 1, "/tmp/bench_buir/log.txt", "Adam", 1e-3, 1e-6, 1, "dense"
    runner = BUIRRunner(ra)
    model.optimizer = runner._build_optimizer(model)
    model.train()
    for bs in (int(x) for x in a.batches.split(",")):
        feed = {"user_id": torch.randint(1, a.users, (bs,), device=dev, generator=gen),
                "item_id": torch.randint(1, a.items, (bs, 1), device=dev, generator=gen), "batch_size": bs, "phase": "train"}

        def eager():
            model.optimizer.zero_grad()
            model.loss(model(feed)).backward()
            model.optimizer.step()
            model._update_target()
        res = {"B": bs}
        res["eager_ms"], = alternate([eager], a.seconds, block=3, warmup=2)
        if hgraph.usable():
            step = hgraph.GraphedStep(model)

            def replayed():
                step.run(feed)
                model._update_target()
            for _ in range(step.WARMUP + 1):
                replayed()
            res["replayed_ms"], = alternate([replayed], a.seconds, block=3, warmup=2)
        out["step"][str(bs)] = res

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
