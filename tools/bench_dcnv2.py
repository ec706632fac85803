"""DCNv2's mixed cross stack on the HIP engine vs the same expression in torch ops on the same GPU in the same process.
Prints ONE JSON line (and writes it to --out).

    python tools/bench_dcnv2.py [--seconds 0.5] [--out FILE]

Shapes: the demo width D = 512 (8 fields x emb_size 64), low_rank 64: B = 1,024 and B = 131,072 with 2 experts and 3 layers, and the
TopK evaluation shape 128 x 100 rows with 1 expert and 4 layers (forward only: evaluation has no backward).
Every figure is a HIP-event time of warm calls, accumulated over at least --seconds per shape and route; the two routes alternate
block by block.  Per shape:
  fwd_*    the forward of the stack under torch.no_grad(): fused_ms (nn.dcnv2_mix_layer_eval per layer) / torch_ms (the reference's
           expression, DCNv2.py:119-141: per expert the gating Linear, three broadcast matmuls on [N, D, 1], two tanh; stack,
           softmax, matmul)
  step_*   forward + backward of the stack with every gradient (x_0, U, V, C, bias per layer, the gate), not for the evaluation shape
  flop_fraction   algorithmic flops -- (4 D r + 2 r^2) per row, layer and expert forward, three times that forward + backward (the
           backward's recomputation is not counted) -- per second over the 157.3 TFLOP/s fp32 MFMA peak
  hbm_fraction    the bytes the node has to move -- X0, Xl read and Xnext written per layer forward; dXnext, X0, Xl read and dXl,
           dX0_part written per layer backward -- per second over 8 TB/s
  max_rel_diff    largest relative difference between the two routes' outputs / gradients
bench.py is not involved."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, MFMA_F32_PEAK = 8.0e12, 157.3e12
SHAPES = [dict(name="B1024", N=1024, D=512, r=64, E=2, L=3, backward=True),
          dict(name="B131072", N=131072, D=512, r=64, E=2, L=3, backward=True),
          dict(name="topk_eval_128x100", N=12800, D=512, r=64, E=1, L=4, backward=False)]


def alternate(fns, seconds, block=3, warmup=2):
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


def torch_stack(x0, layers, gates):
    """cross_net_mix as the reference writes it (DCNv2.py:116-141)"""
    import torch
    x_0 = x0.unsqueeze(2)
    x_l = x_0
    for U, V, C, b in layers:
        outs, gs = [], []
        for e, (wg, bgv) in enumerate(gates):
            gs.append(torch.nn.functional.linear(x_l.squeeze(2), wg, bgv))
            v = torch.tanh(torch.matmul(V[e].T, x_l))
            c = torch.tanh(torch.matmul(C[e], v))
            outs.append((x_0 * (torch.matmul(U[e], c) + b)).squeeze(2))
        moe = torch.matmul(torch.stack(outs, 2), torch.stack(gs, 1).softmax(dim=1))
        x_l = x_l + moe
    return x_l.squeeze(2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from rechorus_amd import engine, nn as hnn
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(2)
    rnd = lambda *s, sd=1.0: (torch.randn(*s, device=dev, generator=gen) * sd).requires_grad_(True)
    out = {"bench": "dcnv2", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "hbm_peak_tbps": HBM_PEAK / 1e12,
           "mfma_f32_peak_tflops": MFMA_F32_PEAK / 1e12, "shapes": []}
    for s in SHAPES:
        N, D, r, E, L = s["N"], s["D"], s["r"], s["E"], s["L"]
        x0 = rnd(N, D, sd=0.5)
        layers = [(rnd(E, D, r, sd=r ** -0.5), rnd(E, D, r, sd=2.0 * D ** -0.5), rnd(E, r, r, sd=1.5 * r ** -0.5), rnd(D, 1, sd=0.3))
                  for _ in range(L)]
        gates = [(rnd(1, D, sd=3.0 * D ** -0.5), rnd(1, sd=0.3)) for _ in range(E)]
        leaves = [x0] + [p for group in layers for p in group] + [p for gt in gates for p in gt]
        dY = torch.randn(N, D, device=dev, generator=gen)
        ws = engine.DCNv2Workspace()

        def fused(train):
            Wg, bg = torch.cat([g[0] for g in gates], 0), torch.cat([g[1] for g in gates], 0)
            x = x0
            for U, V, C, b in layers:
                x = hnn.dcnv2_mix_layer(x0, x, U, V, C, b, Wg, bg, ws) if train else hnn.dcnv2_mix_layer_eval(x0, x, U, V, C, b, Wg, bg)
            return x

        def fwd(route):
            def fn():
                with torch.no_grad():
                    return route()
            return fn

        def step(route):
            def fn():
                for p in leaves:
                    p.grad = None
                route().backward(dY)
                return [p.grad for p in leaves]
            return fn
        rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
        res = {k: s[k] for k in ("name", "N", "D", "r", "E", "L")}
        f_fwd, t_fwd = fwd(lambda: fused(False)), fwd(lambda: torch_stack(x0, layers, gates))
        res["fwd_fused_ms"], res["fwd_torch_ms"] = alternate([f_fwd, t_fwd], a.seconds)
        res["fwd_torch_over_fused"] = res["fwd_torch_ms"] / res["fwd_fused_ms"]
        res["fwd_max_rel_diff"] = "%.3e" % rel(f_fwd(), t_fwd())
        flops = N * L * E * (4 * D * r + 2 * r * r)
        res["fwd_flop_fraction"] = flops / (res["fwd_fused_ms"] * 1e-3) / MFMA_F32_PEAK
        res["fwd_hbm_fraction"] = 3 * 4 * N * D * L / (res["fwd_fused_ms"] * 1e-3) / HBM_PEAK
        if s["backward"]:
            f_step, t_step = step(lambda: fused(True)), step(lambda: torch_stack(x0, layers, gates))
            res["step_fused_ms"], res["step_torch_ms"] = alternate([f_step, t_step], a.seconds)
            res["step_torch_over_fused"] = res["step_torch_ms"] / res["step_fused_ms"]
            gf, gt = [g.clone() for g in f_step()], [g.clone() for g in t_step()]
            res["step_max_rel_diff"] = "%.3e" % max(rel(x, y) for x, y in zip(gf, gt))
            res["step_flop_fraction"] = 3 * flops / (res["step_fused_ms"] * 1e-3) / MFMA_F32_PEAK
            res["step_hbm_fraction"] = 8 * 4 * N * D * L / (res["step_fused_ms"] * 1e-3) / HBM_PEAK
            res["bwd_workspace_bytes"] = int(engine._lib.load().rc_dcnv2_mix_layer_bwd_workspace_bytes(N, D, r, E))
            del gf, gt
        out["shapes"].append(res)
        del x0, layers, gates, leaves, dY, ws
        torch.cuda.empty_cache()

    def rounded(o):
        if isinstance(o, dict):
            return {k: rounded(v) for k, v in o.items()}
        if isinstance(o, list):
            return [rounded(v) for v in o]
        return round(o, 5) if isinstance(o, float) and abs(o) < 1e6 else o
    line = json.dumps(rounded(out))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
