"""DirectAU's loss on the HIP engine vs the torch formulation of the reference, on one GPU; prints ONE JSON line.

    python tools/bench_directau.py [--shapes 256x64,4096x64,65536x64,4096x128] [--iters 20]

For each batch size x emb_size it times, with HIP events after a warm-up of that shape:
  pair_ms_by_difference  the pairwise pass of both sets, as rc_directau_fwd minus the same call without uniformity terms: two
                    separately timed loops, so below ~0.05 ms it is within their noise.  The pairwise kernel's own time per shape
                    comes from a rocprofv3 --kernel-trace run of this tool, read by tools/directau_pair_times.py
  rows_finish_ms    row pass + reduce (rc_directau_fwd without uniformity terms) + the backward launch
  fwd_ms / bwd_ms   rc_directau_fwd (both sets) / rc_directau_bwd
  step_eager_ms     one training step of the DirectAU model file (gathers, scores, loss, backward, dense Adam), eager
  step_replayed_ms  the same step replayed from a hipGraph (rechorus_amd/graph.py)
  torch_ms          F.normalize + torch.pdist + autograd of DirectAU.py:54-88 on the same GPU (skipped past --torch_max)
and the algorithmic flops of the pairs, 3 d B (B - 1) per set (Gram + e x^ products over i < j), plus the largest |difference|
against torch.  bench.py is not involved.
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

PEAK_FLOPS = 157.3e12


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


def torch_loss(u, v, gamma):
    import torch
    import torch.nn.functional as F

    def unif(x):
        x = F.normalize(x, dim=-1)
        return torch.pdist(x, p=2).pow(2).mul(-2).exp().mean().log()
    a, b = F.normalize(u, dim=-1), F.normalize(v, dim=-1)
    align = (a - b).norm(p=2, dim=1).pow(2).mean()
    return align + gamma * (unif(u) + unif(v)) / 2


def bench_shape(B, d, iters, torch_max, gamma=0.3):
    import torch
    from helpers.BaseRunner import BaseRunner
    from models.general.DirectAU import DirectAU
    from rechorus_amd import engine, graph as hgraph
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(B + d)
    u = torch.randn(B, d, device=dev, generator=gen)
    v = torch.randn(B, d, device=dev, generator=gen)
    ws = engine.DirectAUWorkspace()
    g1 = torch.ones(1, device=dev)
    coef = (1.0, gamma / 2, gamma / 2)
    res = {"B": B, "d": d, "gamma": gamma}
    it = max(3, iters if B <= 8192 else iters // 4)
    state = {}

    def fwd(sets):
        state["buf"] = engine.directau_fwd(u, v, gamma, sets=sets, workspace=ws)[2]

    res["fwd_ms"] = timed(lambda: fwd(3), it)
    res["bwd_ms"] = timed(lambda: engine.directau_bwd(g1, B, d, coef, state["buf"]), it)
    rows_ms = timed(lambda: fwd(0), it)
    res["pair_ms_by_difference"] = res["fwd_ms"] - rows_ms
    res["rows_finish_ms"] = rows_ms + res["bwd_ms"]
    res["algorithmic_flops"] = 2 * 3.0 * d * B * (B - 1)
    res["owner_computes_flops"] = 2 * 4.0 * d * B * B

    # against torch: loss and both row gradients
    out, _, buf, _ = engine.directau_fwd(u, v, gamma, workspace=ws)
    gu, gv = engine.directau_bwd(g1, B, d, coef, buf)
    if B <= torch_max:
        uu, vv = u.clone().requires_grad_(True), v.clone().requires_grad_(True)
        ref = torch_loss(uu, vv, gamma)
        ref.backward()
        res["max_abs_diff_loss"] = "%.3e" % abs(float(out[0]) - float(ref))
        res["max_abs_diff_grad"] = "%.3e" % max(float((gu - uu.grad).abs().max()), float((gv - vv.grad).abs().max()))
        res["max_abs_grad"] = "%.3e" % max(float(uu.grad.abs().max()), float(vv.grad.abs().max()))

        def torch_step():
            a, b = u.clone().requires_grad_(True), v.clone().requires_grad_(True)
            torch_loss(a, b, gamma).backward()
        res["torch_ms"] = timed(torch_step, max(3, it // 2), warmup=1)
        res["fwd_bwd_speedup_vs_torch"] = res["torch_ms"] / (res["fwd_ms"] + res["bwd_ms"])
        del uu, vv, ref
        torch.cuda.empty_cache()
    else:
        res["torch_ms"] = None

    # the training step of the model file, eager and replayed (Adam, dense updates)
    n_users, n_items = 100000, 50000
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=0, dropout=0, test_all=0, emb_size=d, gamma=gamma)
    m = DirectAU(args, SimpleNamespace(n_users=n_users, n_items=n_items)).to(dev)
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.train, a.log_file = 1, "/tmp/rc_bench_directau/log.txt"
    a.optimizer, a.lr, a.l2, a.engine = "Adam", 1e-3, 1e-5, "dense"
    m.optimizer = BaseRunner(a)._build_optimizer(m)
    m.train()
    feed = {"user_id": torch.randint(1, n_users, (B,), device=dev, generator=gen),
            "item_id": torch.randint(1, n_items, (B, 1), device=dev, generator=gen), "batch_size": B, "phase": "train"}

    def eager():
        m.optimizer.zero_grad()
        m.loss(m(feed)).backward()
        m.optimizer.step()
    res["step_eager_ms"] = timed(eager, it)
    if hgraph.usable():
        step = hgraph.GraphedStep(m)
        res["step_replayed_ms"] = timed(lambda: step.run(feed), it)
    for k, val in list(res.items()):
        if isinstance(val, float):
            res[k] = round(val, 4) if val < 1e6 else val
    del m
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x64,4096x64,65536x64,4096x128")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch_max", type=int, default=16384, help="largest batch the torch formulation is run at")
    a = ap.parse_args()
    import torch
    out = {"bench": "directau", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True,
           "peak_fp32_mfma_tflops": PEAK_FLOPS / 1e12, "shapes": {}}
    for s in a.shapes.split(","):
        B, d = (int(x) for x in s.split("x"))
        out["shapes"][s] = bench_shape(B, d, a.iters, a.torch_max)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
