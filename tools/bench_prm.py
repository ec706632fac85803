"""PRM's encoder stack on the HIP engine vs torch's own nn.TransformerEncoderLayer and vs the composition of the existing
rc_linear_* / rc_seq_attention_* / rc_seq_add_layernorm_* entry points, on the same GPU in the same process.
Prints ONE JSON line (and writes it to --out).

    python tools/bench_prm.py [--seconds 0.5] [--out FILE]

Shape: the default lists (train_max_pos_item + train_max_neg_item = 40 slots), num_hidden_unit 64, 4 heads, feed-forward 128, 4 blocks;
256, 4,096 and 65,536 lists, every second list with 30 % of its slots padded (12 of 40, scattered over both segments).
Every figure is a HIP-event time of warm calls, accumulated over at least --seconds per shape and route; the routes alternate block by
block.  Per shape:
  fwd_*    the forward of the stack under torch.no_grad(): fused_ms (nn.list_encoder_block_eval per block), torch_ms (fp32
           nn.TransformerEncoderLayer modules, batch_first, in training mode with dropout 0 so that torch's padded-row fast path, which
           does not compute padded queries, stays out), composed_ms (per block: one in-projection GEMM, the per-row attention kernel
           under a [B, n, n] mask, the out-projection, add + LayerNorm, two feed-forward GEMMs, add + LayerNorm)
  step_*   forward + backward of the stack with every gradient (X and the twelve tensors of every block)
  flop_fraction   algorithmic flops -- per list and block 2 n d (3 d + d + 2 d_ff) for the four projections plus 4 n^2 d for the two
           attention products, forward; three times that forward + backward (the backward's recomputation is not counted) -- per second
           over the 157.3 TFLOP/s fp32 MFMA peak
  max_rel_diff    largest relative difference of the fused route's outputs / gradients from torch's
float64_check: at 256 and 16,384 lists, the fused stack and torch's fp32 modules each against torch's modules in float64 on the device
(the worst of Y, dX and every gradient): which of the two fp32 routes a max_rel_diff above comes from.
train_step: the whole training step of PRMGeneral over a frozen BPRMFImpression (the ranker's forward and the rank computation of
collate_batch, forward, list-level BPR, backward, Adam) at 256 and 4,096 lists a batch.
bench.py is not involved."""
import argparse
import json
import os
import sys
import tempfile
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dcnv2 import alternate  # noqa: E402

MFMA_F32_PEAK = 157.3e12
N_SLOTS, D, H, DFF, BLOCKS = 40, 64, 4, 128, 4
LISTS = [256, 4096, 65536]


def composed_block(x, allow, w, B, n):
    """one block on the existing entry points; x [B * n, d], allow uint8 [B, n, n] (1 = the key may be attended)"""
    from rechorus_amd import nn as hnn
    Win, bin_, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2 = w
    d = x.shape[1]
    qkv = hnn.linear(x, Win, bin_)
    q, k, v = (qkv[:, j * d:(j + 1) * d].contiguous() for j in range(3))
    c = hnn._SeqAttentionFn.apply(q, k, v, None, B, n, H, allow, False)
    x1 = hnn._AddLayerNormFn.apply(hnn.linear(c, Wo, bo), x, g1, be1, None, n, 0.0, None, 0)
    f = hnn.linear(hnn.linear(x1, W1, b1, relu=True), W2, b2)
    return hnn._AddLayerNormFn.apply(f, x1, g2, be2, None, n, 0.0, None, 1)


def bench_stack(torch, dev, a):
    from rechorus_amd import engine, nn as hnn
    gen = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s, sd=1.0, mean=0.0: (torch.randn(*s, device=dev, generator=gen) * sd + mean).requires_grad_(True)
    out = []
    for B in LISTS:
        n, d = N_SLOTS, D
        X = rnd(B, n, d)
        pad = torch.zeros(B, n, dtype=torch.bool, device=dev)
        holes = torch.rand(B, n, device=dev, generator=gen).argsort(1)[:, :12]
        pad[1::2] = pad[1::2].scatter(1, holes[1::2], True)
        pad8 = pad.to(torch.uint8)
        allow = (~pad)[:, None, :].expand(B, n, n).to(torch.uint8).contiguous()
        blocks = [[rnd(3 * d, d, sd=1.5 * d ** -0.5), rnd(3 * d, sd=0.1), rnd(d, d, sd=d ** -0.5), rnd(d, sd=0.1), rnd(d, sd=0.3, mean=1.0),
                   rnd(d, sd=0.1), rnd(DFF, d, sd=d ** -0.5), rnd(DFF, sd=0.1), rnd(d, DFF, sd=DFF ** -0.5), rnd(d, sd=0.1),
                   rnd(d, sd=0.3, mean=1.0), rnd(d, sd=0.1)] for _ in range(BLOCKS)]
        leaves = [X] + [p for w in blocks for p in w]
        mods = torch.nn.ModuleList([torch.nn.TransformerEncoderLayer(d, H, DFF, dropout=0.0, batch_first=True) for _ in range(BLOCKS)])
        mods = mods.to(dev).train()
        keys = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "norm1.weight",
                "norm1.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm2.weight", "norm2.bias")
        for m, w in zip(mods, blocks):
            m.load_state_dict({k: t.detach() for k, t in zip(keys, w)})
        tleaves = [X] + [dict(m.named_parameters())[k] for m in mods for k in keys]
        dY = torch.randn(B, n, d, device=dev, generator=gen)
        ws = engine.ListEncWorkspace()

        def fused(train):
            x = X
            for w in blocks:
                x = hnn.list_encoder_block(x, pad8, w, H, ws) if train else hnn.list_encoder_block_eval(x, pad8, w, H)
            return x

        def by_torch():
            x = X
            for m in mods:
                x = m(x, src_key_padding_mask=pad)
            return x

        def composed():
            x = X.reshape(B * n, d)
            for w in blocks:
                x = composed_block(x, allow, w, B, n)
            return x.view(B, n, d)

        def fwd(route):
            def fn():
                with torch.no_grad():
                    return route()
            return fn

        def step(route, params):
            def fn():
                for p in params:
                    p.grad = None
                route().backward(dY)
                return [p.grad for p in params]
            return fn
        rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
        res = dict(lists=B, n=n, d=d, heads=H, d_ff=DFF, blocks=BLOCKS, padded_lists=int(pad.any(1).sum()))
        routes = [fwd(lambda: fused(False)), fwd(by_torch), fwd(composed)]
        res["fwd_fused_ms"], res["fwd_torch_ms"], res["fwd_composed_ms"] = alternate(routes, a.seconds)
        res["fwd_torch_over_fused"] = res["fwd_torch_ms"] / res["fwd_fused_ms"]
        res["fwd_composed_over_fused"] = res["fwd_composed_ms"] / res["fwd_fused_ms"]
        y_f, y_t, y_c = (r() for r in routes)
        res["fwd_max_rel_diff"] = "%.3e" % rel(y_f, y_t)
        res["fwd_composed_max_rel_diff"] = "%.3e" % rel(y_c, y_t)
        flops = B * BLOCKS * (2 * n * d * (4 * d + 2 * DFF) + 4 * n * n * d)
        res["fwd_flop_fraction"] = flops / (res["fwd_fused_ms"] * 1e-3) / MFMA_F32_PEAK
        steps = [step(lambda: fused(True), leaves), step(by_torch, tleaves), step(composed, leaves)]
        res["step_fused_ms"], res["step_torch_ms"], res["step_composed_ms"] = alternate(steps, a.seconds)
        res["step_torch_over_fused"] = res["step_torch_ms"] / res["step_fused_ms"]
        res["step_composed_over_fused"] = res["step_composed_ms"] / res["step_fused_ms"]
        gf, gt = [g.clone() for g in steps[0]()], [g.clone() for g in steps[1]()]
        res["step_max_rel_diff"] = "%.3e" % max(rel(x, y) for x, y in zip(gf, gt))
        res["step_flop_fraction"] = 3 * flops / (res["step_fused_ms"] * 1e-3) / MFMA_F32_PEAK
        res["bwd_workspace_bytes"] = int(engine._lib.load().rc_listenc_block_bwd_workspace_bytes(B, n, d, H, DFF))
        out.append(res)
        del X, blocks, leaves, mods, tleaves, dY, ws, gf, gt, allow
        torch.cuda.empty_cache()
    return out


TORCH_KEYS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "norm1.weight",
              "norm1.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm2.weight", "norm2.bias")


def float64_check(torch, dev):
    """the fused stack and torch's fp32 modules, each against torch's modules in float64 on the device, on a problem drawn like the
    timed ones: the worst tensor (Y, dX, the twelve gradients of every block) of each route, as largest |difference| / largest |float64
    entry|.  Says which of the two fp32 routes the timed shapes' max_rel_diff comes from."""
    from rechorus_amd import engine, nn as hnn
    out = []
    for B in (256, 16384):
        n, d = N_SLOTS, D
        gen = torch.Generator(device=dev).manual_seed(3)
        rnd = lambda *s, sd=1.0, mean=0.0: torch.randn(*s, device=dev, generator=gen) * sd + mean
        X = rnd(B, n, d)
        pad = torch.zeros(B, n, dtype=torch.bool, device=dev)
        holes = torch.rand(B, n, device=dev, generator=gen).argsort(1)[:, :12]
        pad[1::2] = pad[1::2].scatter(1, holes[1::2], True)
        blocks = [[rnd(3 * d, d, sd=1.5 * d ** -0.5), rnd(3 * d, sd=0.1), rnd(d, d, sd=d ** -0.5), rnd(d, sd=0.1), rnd(d, sd=0.3, mean=1.0),
                   rnd(d, sd=0.1), rnd(DFF, d, sd=d ** -0.5), rnd(DFF, sd=0.1), rnd(d, DFF, sd=DFF ** -0.5), rnd(d, sd=0.1),
                   rnd(d, sd=0.3, mean=1.0), rnd(d, sd=0.1)] for _ in range(BLOCKS)]
        dY = torch.randn(B, n, d, device=dev, generator=gen)

        def by_torch(dtype):
            mods = torch.nn.ModuleList([torch.nn.TransformerEncoderLayer(d, H, DFF, dropout=0.0, batch_first=True) for _ in range(BLOCKS)])
            mods = mods.to(dev).to(dtype).train()
            for m, w in zip(mods, blocks):
                m.load_state_dict({k: t.to(dtype) for k, t in zip(TORCH_KEYS, w)})
            x = X.to(dtype).clone().requires_grad_(True)
            y = x
            for m in mods:
                y = m(y, src_key_padding_mask=pad)
            y.backward(dY.to(dtype))
            return [y.detach(), x.grad] + [dict(m.named_parameters())[k].grad for m in mods for k in TORCH_KEYS]

        def fused():
            x, ws = X.clone().requires_grad_(True), engine.ListEncWorkspace()
            leaves = [[t.clone().requires_grad_(True) for t in w] for w in blocks]
            y = x
            for w in leaves:
                y = hnn.list_encoder_block(y, pad.to(torch.uint8), w, H, ws)
            y.backward(dY)
            return [y.detach(), x.grad] + [t.grad for w in leaves for t in w]
        r64, r32, rf = by_torch(torch.float64), by_torch(torch.float32), fused()
        rel = lambda x, y: float((x.double() - y).abs().max() / y.abs().max().clamp_min(1e-300))
        out.append(dict(lists=B, fused_worst_vs_float64="%.3e" % max(rel(c, a_) for a_, c in zip(r64, rf)),
                        torch_fp32_worst_vs_float64="%.3e" % max(rel(b, a_) for a_, b in zip(r64, r32))))
        del r64, r32, rf, X, blocks, dY
        torch.cuda.empty_cache()
    return out


def bench_train_step(torch, dev, a):
    import yaml
    from helpers.ImpressionRunner import ImpressionRunner
    from models.general.BPRMF import BPRMFImpression
    from models.reranker.PRM import PRMGeneral
    from rechorus_amd import nn as hnn
    n_users, n_items, P, N = 50000, 20000, 20, 20
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, loss_n="BPR", emb_size=64,
                           train_max_pos_item=P, train_max_neg_item=N, test_max_pos_item=P, test_max_neg_item=N, ranker_name="BPRMF",
                           ranker_config_file="BPRMF.yaml", ranker_model_file="ranker.pt", tuneranker=0, n_blocks=BLOCKS, num_heads=H,
                           num_hidden_unit=D)
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items)
    out, here = [], os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs("model/BPRMFImpression")
            torch.save(BPRMFImpression(args, corpus).state_dict(), "model/BPRMFImpression/ranker.pt")
            with open("model/BPRMFImpression/BPRMF.yaml", "w") as f:
                yaml.safe_dump({"emb_size": 64}, f)
            model = PRMGeneral(args, corpus).to(dev)
        finally:
            os.chdir(here)
    model.train()
    opt = hnn.HipOptimizer(model.customize_parameters(), "Adam", lr=1e-3, weight_decay=0.0)
    gen = torch.Generator().manual_seed(4)
    for B in (256, 4096):
        pos, neg = torch.randint(1, P + 1, (B,), generator=gen), torch.randint(1, N + 1, (B,), generator=gen)
        col = torch.arange(P + N)[None, :]
        valid = (col < pos[:, None]) | ((col >= P) & (col < P + neg[:, None]))
        items = torch.randint(1, n_items, (B, P + N), generator=gen) * valid
        host = dict(user_id=torch.randint(1, n_users, (B,), generator=gen), item_id=items, pos_num=pos, neg_num=neg)
        host = {k: v.to(dev) for k, v in host.items()}

        def train_step():
            feed = model.add_ranker_outputs(dict(host), B)
            opt.zero_grad()
            o = model(feed)
            loss = model.loss(o, ImpressionRunner._labels(feed, P + N, P, dev))
            loss.backward()
            opt.step()
            return loss
        (ms,) = alternate([train_step], a.seconds)
        out.append(dict(lists=B, slots=P + N, step_ms=ms, loss=float(train_step().item())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    out = {"bench": "prm", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "mfma_f32_peak_tflops": MFMA_F32_PEAK / 1e12,
           "shapes": bench_stack(torch, dev, a), "float64_check": float64_check(torch, dev), "train_step": bench_train_step(torch, dev, a),
           "not_measured": ["kernel trace", "PMC counters", "MIND"]}

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
