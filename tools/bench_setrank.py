"""SetRank's block stacks on the HIP engine vs the same blocks composed from torch's own nn.MultiheadAttention / LayerNorm / Linear, on
the same GPU in the same process.  Prints ONE JSON line (and writes it to --out).

    python tools/bench_setrank.py [--seconds 0.5] [--out profiles/setrank_bench.json]

Shape: the default lists (train_max_pos_item + train_max_neg_item = 40 slots), num_hidden_unit 64, 4 heads, feed-forward 128, 4 blocks;
256, 4,096 and 65,536 lists, every second list with 30 % of its slots padded (12 of 40, scattered over both segments).  Two stacks:
  IMSAB   per block h = MAB1(I, x, x; mask), x' = MAB2(x, h, h) with 20 inducing points: nn.induced_set_block (two rc_setmab launches
          forward; the torch route repeats I over the lists as SetRank.py:77 does)
  MSAB    per block one self-attention block: nn.list_encoder_block (the PRM kernels)
Every figure is a HIP-event time of warm calls, accumulated over at least --seconds per shape and route; the routes alternate call by
call.  Per shape and stack:
  fwd_*    the forward of the stack under torch.no_grad(): fused_ms, torch_ms (fp32 modules in training mode with dropout 0)
  step_*   forward + backward of the stack with every gradient (x, every block's I and the twelve tensors of every MAB)
  flop_fraction   algorithmic flops per second over the 157.3 TFLOP/s fp32 MFMA peak.  A MAB with nq query and nk key rows is
           2 nq d (2 d + 2 d_ff) + 4 nk d d + 4 nq nk d flops forward per list (a shared source's projection, done once, is left out);
           forward + backward counts three times that (the backward's recomputation is not counted)
  max_rel_diff    largest relative difference of the fused route's outputs / gradients from torch's
train_step: the whole training step of SetRankGeneral (IMSAB) over a frozen BPRMFImpression (the ranker's forward and the rank
computation of collate_batch, forward, list-level BPR, backward, Adam) at 256 and 4,096 lists a batch.
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
N_SLOTS, D, H, DFF, BLOCKS, M = 40, 64, 4, 128, 4, 20
LISTS = [256, 4096, 65536]
KEYS = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "norm1.weight", "norm1.bias",
        "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm2.weight", "norm2.bias")


def torch_mab(torch, w, dev):
    """one MAB from torch's own modules, batch-first, carrying the twelve tensors `w` -> (module, its parameters in KEYS order)"""
    nn = torch.nn

    class Mab(nn.Module):
        def __init__(self):
            super().__init__()
            self.attn = nn.MultiheadAttention(D, H, dropout=0.0, batch_first=True)
            self.linear1, self.linear2 = nn.Linear(D, DFF), nn.Linear(DFF, D)
            self.norm1, self.norm2 = nn.LayerNorm(D), nn.LayerNorm(D)

        def forward(self, q, k, pad=None):
            x = self.norm1(q + self.attn(q, k, k, key_padding_mask=pad, need_weights=False)[0])
            return self.norm2(x + self.linear2(torch.relu(self.linear1(x))))
    m = Mab()
    m.load_state_dict({k: t.detach() for k, t in zip(KEYS, w)})
    m = m.to(dev).train()
    return m, [m.get_parameter(k) for k in KEYS]


def mab_flops(nq, nk, shared):
    return 2 * nq * D * ((1 if shared else 2) * D + 2 * DFF) + 4 * nk * D * D + 4 * nq * nk * D


def bench_stacks(torch, dev, a):
    from rechorus_amd import engine, nn as hnn
    gen = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s, sd=1.0, mean=0.0: (torch.randn(*s, device=dev, generator=gen) * sd + mean).requires_grad_(True)
    weights = lambda: [rnd(3 * D, D, sd=1.5 * D ** -0.5), rnd(3 * D, sd=0.1), rnd(D, D, sd=D ** -0.5), rnd(D, sd=0.1), rnd(D, sd=0.3, mean=1.0),
                       rnd(D, sd=0.1), rnd(DFF, D, sd=D ** -0.5), rnd(DFF, sd=0.1), rnd(D, DFF, sd=DFF ** -0.5), rnd(D, sd=0.1),
                       rnd(D, sd=0.3, mean=1.0), rnd(D, sd=0.1)]
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
    out = []
    for B in LISTS:
        n = N_SLOTS
        X = rnd(B, n, D)
        pad = torch.zeros(B, n, dtype=torch.bool, device=dev)
        holes = torch.rand(B, n, device=dev, generator=gen).argsort(1)[:, :12]
        pad[1::2] = pad[1::2].scatter(1, holes[1::2], True)
        pad8 = pad.to(torch.uint8)
        dY = torch.randn(B, n, D, device=dev, generator=gen)
        for kind in ("IMSAB", "MSAB"):
            blocks = [dict(I=rnd(M, D), w1=weights(), w2=weights() if kind == "IMSAB" else None) for _ in range(BLOCKS)]
            mods = [(torch_mab(torch, b["w1"], dev), torch_mab(torch, b["w2"], dev) if kind == "IMSAB" else None) for b in blocks]
            if kind == "IMSAB":
                leaves = [X] + [t for b in blocks for t in [b["I"]] + b["w1"] + b["w2"]]
                tI = [b["I"].detach().clone().requires_grad_(True) for b in blocks]
                tleaves = [X] + [t for i, (m1, m2) in zip(tI, mods) for t in [i] + m1[1] + m2[1]]
                ws = engine.SetMabWorkspace()
                flops = B * BLOCKS * (mab_flops(M, n, True) + mab_flops(n, M, False))
            else:
                leaves = [X] + [t for b in blocks for t in b["w1"]]
                tleaves = [X] + [t for (m1, _) in mods for t in m1[1]]
                ws = engine.ListEncWorkspace()
                flops = B * BLOCKS * mab_flops(n, n, False)

            def fused(train):
                x = X
                for b in blocks:
                    if kind == "IMSAB":
                        x = (hnn.induced_set_block(x, pad8, b["I"], b["w1"], b["w2"], H, ws) if train
                             else hnn.induced_set_block_eval(x, pad8, b["I"], b["w1"], b["w2"], H))
                    else:
                        x = hnn.list_encoder_block(x, pad8, b["w1"], H, ws) if train else hnn.list_encoder_block_eval(x, pad8, b["w1"], H)
                return x

            def by_torch():
                x = X
                for l, ((m1, _), m2) in enumerate(mods):
                    if kind == "IMSAB":
                        x = m2[0](x, m1(tI[l].unsqueeze(0).repeat(B, 1, 1), x, pad))
                    else:
                        x = m1(x, x, pad)
                return x

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
            res = dict(stack=kind, lists=B, n=n, d=D, heads=H, d_ff=DFF, blocks=BLOCKS, inducing_points=M if kind == "IMSAB" else 0,
                       padded_lists=int(pad.any(1).sum()))
            routes = [fwd(lambda: fused(False)), fwd(by_torch)]
            res["fwd_fused_ms"], res["fwd_torch_ms"] = alternate(routes, a.seconds)
            res["fwd_torch_over_fused"] = res["fwd_torch_ms"] / res["fwd_fused_ms"]
            y_f, y_t = (r() for r in routes)
            res["fwd_max_rel_diff"] = "%.3e" % rel(y_f, y_t)
            res["fwd_flop_fraction"] = flops / (res["fwd_fused_ms"] * 1e-3) / MFMA_F32_PEAK
            steps = [step(lambda: fused(True), leaves), step(by_torch, tleaves)]
            res["step_fused_ms"], res["step_torch_ms"] = alternate(steps, a.seconds)
            res["step_torch_over_fused"] = res["step_torch_ms"] / res["step_fused_ms"]
            gf, gt = [g.clone() for g in steps[0]()], [g.clone() for g in steps[1]()]
            res["step_max_rel_diff"] = "%.3e" % max(rel(x, y) for x, y in zip(gf, gt))
            res["step_flop_fraction"] = 3 * flops / (res["step_fused_ms"] * 1e-3) / MFMA_F32_PEAK
            lib = engine._lib.load()
            res["bwd_workspace_bytes"] = (int(lib.rc_setmab_bwd_workspace_bytes(B, M, n, D, H, DFF) + lib.rc_setmab_bwd_workspace_bytes(B, n, M, D, H, DFF))
                                          if kind == "IMSAB" else int(lib.rc_listenc_block_bwd_workspace_bytes(B, n, D, H, DFF)))
            out.append(res)
            del blocks, mods, leaves, tleaves, ws, gf, gt, y_f, y_t
            X.grad = None
            torch.cuda.empty_cache()
        del X, dY
        torch.cuda.empty_cache()
    return out


def bench_train_step(torch, dev, a):
    import yaml
    from helpers.ImpressionRunner import ImpressionRunner
    from models.general.BPRMF import BPRMFImpression
    from models.reranker.SetRank import SetRankGeneral
    from rechorus_amd import nn as hnn
    n_users, n_items, P, N = 50000, 20000, 20, 20
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, loss_n="BPR", emb_size=64,
                           train_max_pos_item=P, train_max_neg_item=N, test_max_pos_item=P, test_max_neg_item=N, ranker_name="BPRMF",
                           ranker_config_file="BPRMF.yaml", ranker_model_file="ranker.pt", tuneranker=0, n_blocks=BLOCKS, num_heads=H,
                           num_hidden_unit=D, setrank_type="IMSAB")
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items)
    out, here = [], os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs("model/BPRMFImpression")
            torch.save(BPRMFImpression(args, corpus).state_dict(), "model/BPRMFImpression/ranker.pt")
            with open("model/BPRMFImpression/BPRMF.yaml", "w") as f:
                yaml.safe_dump({"emb_size": 64}, f)
            model = SetRankGeneral(args, corpus).to(dev)
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
        out.append(dict(lists=B, slots=P + N, setrank_type="IMSAB", step_ms=ms, loss=float(train_step().item())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    out = {"bench": "setrank", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "one_box_one_run": True,
           "mfma_f32_peak_tflops": MFMA_F32_PEAK / 1e12, "shapes": bench_stacks(torch, dev, a), "train_step": bench_train_step(torch, dev, a),
           "not_measured": ["kernel trace", "PMC counters", "run-to-run spread (one run)", "MIND", "SetRankSequential's training step",
                            "the MSAB training step", "widths other than 64"]}

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
