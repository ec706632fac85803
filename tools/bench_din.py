"""DIN's target attention on the HIP engine (rc_din_attention_fwd + rc_din_attention_bwd) against the same expression in torch
ops, forward + backward, on one GPU; prints ONE JSON line (and writes it to --out, default profiles/din_bench.json).

    python tools/bench_din.py [--shapes B,C,L,H,A1[xA2[xA3]];...] [--seconds 0.5] [--out FILE]

Every figure is a HIP-event time of warm calls, accumulated over at least --seconds per shape and route; the two routes alternate
block by block in the same process (tools/bench_fpmc.py's protocol).  The default shapes are the reference's demo lines: the CTR
training shape of CTR_MIND.sh:24 (B = 1,024, C = 1, L = 40, att [64, 64]) at H = 192 and 448, the TopK evaluation shape of
Topk_MIND.sh:24 (B = 128, C = 100, L = 10, att [256]) and B = 65,536 at the first shape.
  hip_ms     one forward (with the weights output) + one backward through the engine wrappers; hip_fwd_ms / hip_bwd_ms: each alone
  torch_ms   DIN.attention's expression (repeat, cat[q, k, q - k, q * k], Linear / sigmoid layers, mask, scale, matmul) and
             torch.autograd.grad to q, keys and every parameter; "oom" where it does not fit
  mfma_frac  the algorithmic flops of the FOLDED form, forward + backward counted as 3 x forward (the backward's recomputation of
             the forward is not counted), over hip_ms as a fraction of the 157.3 TFLOP/s fp32 MFMA peak -- a whole-call figure
             from HIP events over three launches, not a kernel-trace time
bench.py is not involved.  Not measured here: kernel traces, the model's training step, MIND, ML-1M.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_fpmc import alternate  # noqa: E402

MFMA_PEAK = 157.3e12
DEFAULT = "1024,1,40,192,64x64;1024,1,40,448,64x64;128,100,10,192,256;65536,1,40,192,64x64"


def folded_forward_flops(B, C, L, H, widths):
    N = B * C
    f = 2.0 * widths[0] * H * (N + B * L + N * L)          # q term per instance, k term per (b, l), Wp term per (n, l)
    K = widths[0]
    for A in widths[1:]:
        f += 2.0 * A * K * N * L
        K = A
    return f + 2.0 * K * N * L + 2.0 * H * N * L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "din_bench.json"))
    a = ap.parse_args()
    import torch
    from rechorus_amd import engine
    if not torch.cuda.is_available():
        raise SystemExit("bench_din.py measures on the GPU only")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(2)
    out = {"bench": "din", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "mfma_peak_tflops": MFMA_PEAK / 1e12,
           "shapes": [], "not_measured": ["kernel traces", "the model's training step and the tower's share of it", "MIND", "ML-1M"]}
    for spec in a.shapes.split(";"):
        B, C, L, H, w = spec.split(",")
        B, C, L, H, widths = int(B), int(C), int(L), int(H), [int(x) for x in w.split("x")]
        N = B * C
        q = torch.randn((N, H), device=dev, generator=gen)
        keys = torch.randn((B, L, H), device=dev, generator=gen)
        lens = torch.randint(1, L + 1, (B,), device=dev, generator=gen)
        d_out = torch.randn((N, H), device=dev, generator=gen)
        params, K = [], 4 * H
        for A in widths + [1]:
            params.append((torch.randn((A, K), device=dev, generator=gen) / (1.5 * K) ** 0.5, torch.randn(A, device=dev, generator=gen) * 0.1))
            K = A
        flat = torch.cat([t.reshape(-1) for p in params for t in p])

        def hip():
            engine.din_attention_fwd(q, keys, lens, flat, C, widths, want_att=True)
            return engine.din_attention_bwd(q, keys, lens, flat, d_out, C, widths)

        leaves = [q.clone().requires_grad_(), keys.clone().requires_grad_()] + [t.clone().requires_grad_() for p in params for t in p]

        def torch_ops():
            tq, tk, tp = leaves[0], leaves[1], leaves[2:]
            k = tk.unsqueeze(1).repeat(1, C, 1, 1).view(N, L, H)
            qq = tq.repeat(1, L).view(N, L, H)
            h = torch.cat([qq, k, qq - k, qq * k], dim=-1)
            for j in range(len(widths)):
                h = torch.sigmoid(torch.nn.functional.linear(h, tp[2 * j], tp[2 * j + 1]))
            s = torch.nn.functional.linear(h, tp[-2], tp[-1]).squeeze(-1)
            mask = torch.arange(L, device=dev).view(1, -1) >= lens.repeat_interleave(C).unsqueeze(1)
            att = s.masked_fill(mask, 0.0) / H ** 0.5
            o = torch.matmul(att.unsqueeze(1), k).squeeze(1)
            return torch.autograd.grad((o * d_out).sum(), leaves)

        rec = {"B": B, "C": C, "L": L, "H": H, "att_layers": widths}
        try:
            g = torch_ops()
            dq, dkeys, dflat = hip()
            rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
            rec["dq_rel_diff"], rec["dkeys_rel_diff"] = rel(dq, g[0]), rel(dkeys, g[1])
            rec["dW1_rel_diff"] = rel(dflat[:g[2].numel()].view_as(g[2]), g[2])
            del g
            hip_ms, torch_ms = alternate([hip, torch_ops], a.seconds)
            fwd_ms, bwd_ms = alternate([lambda: engine.din_attention_fwd(q, keys, lens, flat, C, widths, want_att=True),
                                        lambda: engine.din_attention_bwd(q, keys, lens, flat, d_out, C, widths)], a.seconds / 2)
            rec["hip_fwd_ms"], rec["hip_bwd_ms"] = round(fwd_ms, 4), round(bwd_ms, 4)
            rec["torch_ms"] = round(torch_ms, 4)
            rec["ratio"] = round(torch_ms / hip_ms, 3)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            hip_ms, = alternate([hip], a.seconds)
            rec["torch_ms"] = "oom"
        rec["hip_ms"] = round(hip_ms, 4)
        flops = 3.0 * folded_forward_flops(B, C, L, H, widths)
        rec["folded_gflop_fwd_bwd"] = round(flops / 1e9, 3)
        rec["mfma_frac"] = round(flops / (hip_ms * 1e-3) / MFMA_PEAK, 4)
        out["shapes"].append(rec)
        del leaves
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
