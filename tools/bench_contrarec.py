"""ContraRec on the HIP engine, on one GPU; prints ONE JSON line (kept as profiles/contrarec_bench.json).

    python tools/bench_contrarec.py [--batches 256,4096,16384] [--iters 20] [--repeats 5] [--d 64 --L 20]

Per batch size B (N = 2 B stacked rows), HIP-event times of warm calls, each the MEDIAN of --repeats windows of --iters calls (ms):
  fwd_ms / bwd_ms     rc_contra_loss_fwd (rows, stats sweep, finish, reduce) / rc_contra_loss_bwd (weight sweep, rows)
  hip_ms              the autograd node end to end: forward + backward to the two views' gradients
  torch_ms            the same expression (ContraRec.py:92,148-193) in torch ops with autograd, on the same GPU in the same run
  flops / fraction_of_fp32_mfma_peak   algorithmic flops 6 d N^2 (the Gram tile in both sweeps, the weight product in the second)
                      over fwd_ms + bwd_ms, against the 157.3 TFLOP/s fp32 MFMA peak
  encoder_3b_fwd_ms / encoder_3b_fwd_bwd_ms   nn.bert4rec_encode_layers on the 3 B sequences of a training forward (L positions)
  step_eager_ms       one eager training step of the model file: forward, both losses, backward, dense Adam
and the largest |difference| of loss and gradients against the torch-op route.  bench.py is not involved.
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

PEAK_FLOPS = 157.3e12


def timed(fn, iters, repeats, warmup=3):
    """median over `repeats` windows of `iters` warm calls, ms per call"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out)


def torch_contra_loss(va, vb, labels, t):
    """the context-context loss in torch ops: normalise, stack view-major, N x N logits, masked log-softmax over the positives"""
    import torch
    import torch.nn.functional as F
    z = F.normalize(torch.cat([va, vb], 0), dim=-1)
    n = z.shape[0]
    lab = torch.cat([labels, labels])
    logits = z @ z.t() / t
    logits = logits - logits.max(dim=1, keepdim=True)[0].detach()
    off = ~torch.eye(n, dtype=torch.bool, device=z.device)
    pos = (lab[:, None] == lab[None, :]) & off
    log_prob = logits - torch.log((logits.exp() * off).sum(1, keepdim=True) + 1e-10)
    return (-t * (pos * log_prob).sum(1) / (pos.sum(1) + 1e-10)).mean()


def bench_batch(B, d, L, iters, repeats, t=0.2):
    import torch
    from helpers.BaseRunner import BaseRunner
    from models.sequential.ContraRec import ContraRec
    from rechorus_amd import engine, nn as hnn
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(B)
    n_items = 20000
    va = torch.randn(B, d, device=dev, generator=gen, requires_grad=True)
    vb = torch.randn(B, d, device=dev, generator=gen, requires_grad=True)
    labels = torch.randint(1, n_items, (B,), device=dev, generator=gen)
    ws = engine.ContraWorkspace()
    g1 = torch.ones(1, device=dev)
    it = max(3, iters if B <= 4096 else iters // 4)
    res = {"B": B, "N": 2 * B, "d": d, "temperature": t, "chunks": engine.contra_layout(d, B)[0]}
    state = {}

    def fwd():
        state["f"] = engine.contra_loss_fwd(va.detach(), vb.detach(), labels, t, workspace=ws)
    res["fwd_ms"] = timed(fwd, it, repeats)
    buf = state["f"][1]
    res["bwd_ms"] = timed(lambda: engine.contra_loss_bwd(g1, labels, B, d, t, buf), it, repeats)

    def zero():
        va.grad = vb.grad = None

    def hip_route():
        zero()
        hnn.contra_loss(va, vb, labels, t, workspace=ws).backward()

    def torch_route():
        zero()
        torch_contra_loss(va, vb, labels, t).backward()
    res["hip_ms"] = timed(hip_route, it, repeats)
    hip_route()
    loss_hip, ga, gb = hnn.contra_loss(va, vb, labels, t).item(), va.grad.clone(), vb.grad.clone()
    res["torch_ms"] = timed(torch_route, max(2, it // 4), repeats, warmup=2)
    torch_route()
    loss_torch = torch_contra_loss(va, vb, labels, t).item()
    res["loss_diff_vs_torch"] = "%.3e" % abs(loss_hip - loss_torch)
    res["grad_rel_diff_vs_torch"] = "%.3e" % max(float((a - b.grad).abs().max() / b.grad.abs().max()) for a, b in ((ga, va), (gb, vb)))
    res["hip_vs_torch_speedup"] = res["torch_ms"] / res["hip_ms"]
    res["flops"] = 6.0 * d * (2.0 * B) ** 2
    res["tflops"] = res["flops"] / ((res["fwd_ms"] + res["bwd_ms"]) * 1e-3) / 1e12
    res["fraction_of_fp32_mfma_peak"] = res["flops"] / ((res["fwd_ms"] + res["bwd_ms"]) * 1e-3) / PEAK_FLOPS
    torch.cuda.empty_cache()

    # the model file: the 3 B encoder pass and the eager training step
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, emb_size=d, history_max=L, gamma=1.0,
                           beta_a=3, beta_b=3, ctc_temp=1.0, ccc_temp=t, encoder="BERT4Rec", batch_size=B)
    model = ContraRec(args, SimpleNamespace(n_users=1000, n_items=n_items)).to(dev)
    lengths = torch.randint(1, L + 1, (B,), device=dev, generator=gen)
    valid = torch.arange(L, device=dev)[None, :] < lengths[:, None]
    hists = [torch.randint(1, n_items + 1, (B, L), device=dev, generator=gen) * valid for _ in range(3)]
    feed = {"item_id": torch.randint(1, n_items, (B, 2), device=dev, generator=gen), "history_items": hists[0].clamp(max=n_items - 1),
            "history_items_a": hists[1], "history_items_b": hists[2], "lengths": lengths, "batch_size": B, "phase": "train"}
    stacked, len3 = torch.cat([feed["history_items"], hists[1], hists[2]], 0), lengths.repeat(3)

    def enc_fwd():
        with torch.no_grad():
            model.encoder(model.i_embeddings.weight, stacked, len3)

    def enc_fwd_bwd():
        model.zero_grad(set_to_none=True)
        model.encoder(model.i_embeddings.weight, stacked, len3).sum().backward()
    res["encoder_3b_fwd_ms"] = timed(enc_fwd, it, repeats)
    res["encoder_3b_fwd_bwd_ms"] = timed(enc_fwd_bwd, it, repeats)
    a, _ = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    a.train, a.log_file, a.optimizer, a.lr, a.l2, a.graph, a.engine = 1, "/tmp/rechorus_amd_bench/log.txt", "Adam", 1e-4, 1e-6, 0, "dense"
    model.optimizer = BaseRunner(a)._build_optimizer(model)
    model.train()

    def step():
        model.optimizer.zero_grad()
        model.loss(model(feed)).backward()
        model.optimizer.step()
    res["step_eager_ms"] = timed(step, it, repeats)
    for k, v in list(res.items()):
        if isinstance(v, float):
            res[k] = round(v, 4) if v < 1e6 else v
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,4096,16384")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--L", type=int, default=20)
    a = ap.parse_args()
    import torch
    out = {"bench": "contrarec", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "peak_fp32_mfma_tflops": PEAK_FLOPS / 1e12,
           "timing": "median of %d windows of warm calls, HIP events" % a.repeats, "batches": {}}
    for b in a.batches.split(","):
        out["batches"][b] = bench_batch(int(b), a.d, a.L, a.iters, a.repeats)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
