"""ComiRec's multi-interest extraction on the HIP engine vs the same forward + backward written with torch ops over HipEmbedding
(what a user's ComiRec model file gets through adopt_embeddings), on one GPU; prints ONE JSON line.

    python tools/bench_comirec.py [--batches 256,4096,65536] [--iters 20] [--d 64 --attn_size 8 --K 4 --L 20 --C 100]

Per batch size (HIP-event times of warm calls, ms):
  fwd_ms / bwd_ms     rc_comirec_fwd (with the hard selection) / rc_comirec_bwd (both launches)
  score_max_ms        rc_comirec_score_max on C candidates per sequence
  fused_train_ms      the autograd node end to end: forward, backward, the two dense table gradients
  torch_train_ms      the reference's formulation in torch ops over HipEmbedding tables: forward + backward to the same gradients
  fwd_bytes / fwd_tbps   algorithmic bytes of the forward (B L d 4 history rows once + interests, attention weights, user rows)
                         and the rate they give against the 8 TB/s HBM peak; likewise bwd_bytes (rows once + g_hist + g_x written)
bench.py is not involved.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

HBM_PEAK = 8.0e12


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


def torch_user_vector(i_emb, p_emb, W1, W2, hist, lengths, target):
    """ComiRec.py:64-87 in torch ops (per-row softmax maximum; the tables are HipEmbedding modules)"""
    import torch
    B, L = hist.shape
    valid = (hist > 0).long()
    his = i_emb(hist)
    pos = p_emb((lengths[:, None] - torch.arange(L, device=hist.device)[None, :]) * valid)
    score = W2(W1(his + pos).tanh()).masked_fill(valid.unsqueeze(-1) == 0, float("-inf")).transpose(-1, -2)
    attn = score.softmax(dim=-1)
    attn = attn.masked_fill(torch.isnan(attn), 0)
    interests = (his[:, None, :, :] * attn[:, :, :, None]).sum(-2)
    sel = (interests * i_emb(target)[:, None, :]).sum(-1).max(-1)[1]
    return interests[torch.arange(B, device=hist.device), sel]


def bench_batch(B, d, A, K, L, C, iters):
    import torch
    import torch.nn as nn
    from rechorus_amd import engine, nn as hnn
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(B)
    n_items = 200000
    i_emb, p_emb = hnn.HipEmbedding(n_items, d).to(dev), hnn.HipEmbedding(L + 1, d).to(dev)
    W1, W2 = nn.Linear(d, A).to(dev), nn.Linear(A, K).to(dev)
    with torch.no_grad():
        for p in (i_emb.weight, p_emb.weight, W1.weight, W1.bias, W2.weight, W2.bias):
            p.copy_(torch.randn(p.shape, device=dev, generator=gen) * 0.5)
    lengths = torch.randint(1, L + 1, (B,), device=dev, generator=gen)
    hist = torch.randint(1, n_items, (B, L), device=dev, generator=gen)
    hist = hist * (torch.arange(L, device=dev)[None, :] < lengths[:, None])
    target = torch.randint(1, n_items, (B,), device=dev, generator=gen)
    cand = torch.randint(1, n_items, (B, C), device=dev, generator=gen)
    d_user = torch.randn(B, d, device=dev, generator=gen)
    params = (i_emb.weight, p_emb.weight, W1.weight, W1.bias, W2.weight, W2.bias)
    det = [p.detach() for p in params]
    ws = engine.ComiRecWorkspace()
    it = max(3, iters if B <= 8192 else iters // 4)
    res = {"B": B, "d": d, "attn_size": A, "K": K, "L": L, "C": C}
    state = {}

    def fwd():
        state["f"] = engine.comirec_fwd(*det, hist, lengths, targets=target)
    res["fwd_ms"] = timed(fwd, it)
    interests, attn, sel, user = state["f"]
    res["bwd_ms"] = timed(lambda: engine.comirec_bwd(*det[:5], hist, lengths, attn, sel, user, d_user, workspace=ws), it)
    res["score_max_ms"] = timed(lambda: engine.comirec_score_max(interests, det[0], cand), it)

    def zero():
        for p in params:
            p.grad = None

    def fused():
        zero()
        hnn.comirec_user_vector(*params, hist, lengths, target, workspace=ws).backward(d_user)

    def torch_route():
        zero()
        torch_user_vector(i_emb, p_emb, W1, W2, hist, lengths, target).backward(d_user)
    res["fused_train_ms"] = timed(fused, it)
    fused()
    g_fused = [p.grad.clone() for p in params]
    res["torch_train_ms"] = timed(torch_route, max(3, it // 2), warmup=2)
    torch_route()
    same_sel = bool((torch_user_vector(i_emb, p_emb, W1, W2, hist, lengths, target).detach() - user).abs().max() < 1e-3)
    res["max_rel_diff_vs_torch"] = "%.3e" % max(float((a - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30))
                                                for a, p in zip(g_fused[:5], params[:5]))
    res["same_selection_as_torch"] = same_sel
    res["fused_vs_torch_speedup"] = res["torch_train_ms"] / res["fused_train_ms"]
    rows = float(hist.gt(0).sum().item()) * d * 4
    res["fwd_bytes"] = rows + 4.0 * B * (K * d + K * L + d) + 8.0 * B * L
    res["bwd_bytes"] = rows + 2 * 4.0 * B * L * d + 4.0 * B * (2 * d + L) + 8.0 * B * L
    res["score_bytes"] = 4.0 * B * C * d + 8.0 * B * C + 4.0 * B * (K * d + C)
    for k in ("fwd", "bwd", "score"):
        ms = res[{"fwd": "fwd_ms", "bwd": "bwd_ms", "score": "score_max_ms"}[k]]
        res[k + "_tbps"] = res[k + "_bytes"] / (ms * 1e-3) / 1e12
        res[k + "_fraction_of_hbm_peak"] = res[k + "_bytes"] / (ms * 1e-3) / HBM_PEAK
    for k, v in list(res.items()):
        if isinstance(v, float):
            res[k] = round(v, 4) if v < 1e6 else v
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,4096,65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--attn_size", type=int, default=8)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--L", type=int, default=20)
    ap.add_argument("--C", type=int, default=100)
    a = ap.parse_args()
    import torch
    out = {"bench": "comirec", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "hbm_peak_tbps": HBM_PEAK / 1e12,
           "batches": {}}
    for b in a.batches.split(","):
        out["batches"][b] = bench_batch(int(b), a.d, a.attn_size, a.K, a.L, a.C, a.iters)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
