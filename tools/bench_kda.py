"""KDA's relational dynamic aggregation on the HIP engine (rc_kda_aggregate_fwd + rc_kda_aggregate_bwd) against the same expression
in torch ops, forward + backward, on one GPU; prints ONE JSON line (and writes it to --out, default profiles/kda_bench.json).

    python tools/bench_kda.py [--shapes B,C,L,R,V,F;...] [--seconds 0.5] [--out FILE]

Every figure is a HIP-event time of warm calls, accumulated over at least --seconds per shape and route; the two routes alternate
block by block in the same process (tools/bench_fpmc.py's protocol).  The default shapes are the reference's default batch
(B = 256 rows of C = 100 candidates, --history_max 20, --emb_size 64, --n_dft 64, five relations) and B = 4,096 at the same shape.
  hip_ms     one forward + one backward through the engine wrappers; hip_fwd_ms / hip_bwd_ms: each alone
  torch_ms   RelationalDynamicAggregation's expression (the [B, C, L, R, V] product and sum for the scores, the masked softmax, the
             Fourier decay with its clamp, the second [B, C, L, R, V] product and sum) and torch.autograd.grad to seq, target,
             value, rel and both frequency tables; "oom" where it does not fit
  *_rel_diff the largest difference between the two routes' results over the largest entry, per quantity
bench.py is not involved.  Not measured here: kernel traces, the model's training step, a real dataset.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_fpmc import alternate  # noqa: E402

DEFAULT = "256,100,20,5,64,33;4096,100,20,5,64,33"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kda_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from rechorus_amd import engine
    if not torch.cuda.is_available():
        raise SystemExit("bench_kda.py measures on the GPU only")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(2)
    out = {"bench": "kda", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "include_val": 1, "shapes": [],
           "not_measured": ["kernel traces", "the model's training step", "a real dataset"]}
    for spec in a.shapes.split(";"):
        B, C, L, R, V, F = (int(x) for x in spec.split(","))
        s = (1.5 / math.sqrt(2. * V)) ** (1. / 3.)
        rnd = lambda *shape, sd=1.0: torch.randn(shape, device=dev, generator=gen) * sd
        seq, target, value, rel = rnd(B, L, V, sd=s), rnd(B, C, V, sd=s), rnd(B, C, R, V, sd=s), rnd(R, V, sd=s)
        sigma = 0.7 * 2 * F / math.sqrt(F - 1)
        fre, fim = rnd(R, F, sd=sigma), rnd(R, F, sd=sigma)
        fre[:, 0] = 0.5 * 2 * F
        dt = torch.rand((B, L), device=dev, generator=gen) * 20
        lens = torch.randint(1, L + 1, (B,), device=dev, generator=gen)
        hist = (torch.arange(L, device=dev).view(1, -1) < lens.view(-1, 1)).long()       # right-padded, every row valid somewhere
        d_ctx = rnd(B, C, R, V)
        freqs = torch.from_numpy(np.concatenate((np.linspace(0, 1, F) / 2., -np.linspace(0, 1, F) / 2.))).to(dev).float()

        def hip():
            engine.kda_aggregate_fwd(seq, hist, dt, target, value, rel, fre, fim, True)
            return engine.kda_aggregate_bwd(seq, hist, dt, target, value, rel, fre, fim, d_ctx, True)

        leaves = [t.clone().requires_grad_() for t in (seq, target, value, rel, fre, fim)]
        valid = (hist > 0).view(B, 1, L, 1)

        def torch_ops():
            tseq, ttarget, tvalue, trel, tre, tim = leaves
            ri = (trel[None, None] + tvalue) * ttarget[:, :, None, :]
            att = (tseq[:, None, :, None, :] * ri[:, :, None, :, :]).sum(-1)
            att = (att - att.max()).masked_fill(valid == 0, -np.inf).softmax(dim=-2)
            w = 2. * np.pi * freqs * dt.unsqueeze(-1)
            x_real, x_imag = torch.cat([tre, tre], dim=-1), torch.cat([tim, -tim], dim=-1)
            decay = (w.cos()[:, :, None, :] * x_real[None, None] - w.sin()[:, :, None, :] * x_imag[None, None]).mean(dim=-1) / 2.
            att = att * decay.clamp(0, 1).unsqueeze(1).masked_fill(valid == 0, 0.)
            ctx = (tseq[:, None, :, None, :] * att[:, :, :, :, None]).sum(-3)
            return torch.autograd.grad((ctx * d_ctx).sum(), leaves)

        rec = {"B": B, "C": C, "L": L, "R": R, "V": V, "F": F,
               "torch_product_mb": round(B * C * L * R * V * 4 / 1e6, 1), "context_mb": round(B * C * R * V * 4 / 1e6, 1)}
        try:
            g = torch_ops()
            mine = hip()
            diff = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
            for name, x, y in zip(("dseq", "dtarget", "dvalue", "drel", "dfreq_real", "dfreq_imag"), mine, g):
                rec[name + "_rel_diff"] = diff(x, y)
            del g, mine
            hip_ms, torch_ms = alternate([hip, torch_ops], a.seconds)
            rec["torch_ms"] = round(torch_ms, 4)
            rec["ratio"] = round(torch_ms / hip_ms, 3)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            hip_ms, = alternate([hip], a.seconds)
            rec["torch_ms"] = "oom"
        fwd_ms, bwd_ms = alternate([lambda: engine.kda_aggregate_fwd(seq, hist, dt, target, value, rel, fre, fim, True),
                                    lambda: engine.kda_aggregate_bwd(seq, hist, dt, target, value, rel, fre, fim, d_ctx, True)],
                                   a.seconds / 2)
        rec["hip_fwd_ms"], rec["hip_bwd_ms"], rec["hip_ms"] = round(fwd_ms, 4), round(bwd_ms, 4), round(hip_ms, 4)
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
