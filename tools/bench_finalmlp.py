"""FinalMLP on the HIP engine vs the torch-op route on the same GPU in the same process: the model's own CPU-path modules (the gate
MLP_Block's last Linear + Sigmoid, the product, each stream's first Linear + ReLU; InteractionAggregation.forward) applied to device
tensors.  Prints ONE JSON line (and writes it to --out).

    python tools/bench_finalmlp.py [--batches 1024,131072] [--topk 1024x100] [--seconds 0.5] [--out FILE]

Every figure is a HIP-event time of warm calls, accumulated over at least --seconds per shape and route; the two routes alternate
block by block.  MIND demo shape: F = 8 fields, emb_size 64, fs [64], contexts of CTR_MIND.sh:20 (stream 1: the situation features,
one gate row per batch row; stream 2: the item features, one per instance), mlp1 [64], mlp2 [256], one head.
  gate     forward + backward of the gated first layers of both streams with every gradient (dX, dZin, dWg, dbg, dW, db per stream):
           fused_ms (hnn.finalmlp_gate) / torch_ms and their ratio, the largest relative difference of the gradients between the
           routes, and the fused route's bytes/s against what it has to move (forward: X and Zin read, A written; backward: X, Zin, A,
           dA read, dX and dZin written) over the 8 TB/s HBM peak
  fusion   the same for the bilinear fusion (forward: x, y read, out written; backward: x, y, dout read, dx, dy written)
  step     the whole FinalMLPCTR training step (gather, gate MLPs, streams, fusion, sigmoid + BCE, backward, dense Adam), eager and
           replayed from a hipGraph, with the DeepFMCTR step on the same data beside it (CTR shapes only)
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

from bench_autoint import alternate, build_deepfm  # noqa: E402

HBM_PEAK = 8.0e12
D_EMB = 64
ITEM, SIT = ["i_category_c", "i_subcategory_c"], ["c_day_f", "c_hour_c", "c_period_c", "c_weekday_c"]
VOCAB = {"i_category_c": 18, "i_subcategory_c": 300, "c_hour_c": 24, "c_period_c": 9, "c_weekday_c": 7, "c_day_f": 7}
N_USERS, N_ITEMS = 100001, 50001
FLAGS = dict(emb_size=D_EMB, mlp1_hidden_units="[64]", mlp1_hidden_activations="ReLU", mlp1_dropout=0, mlp1_batch_norm=0,
             mlp2_hidden_units="[256]", mlp2_hidden_activations="ReLU", mlp2_dropout=0, mlp2_batch_norm=0, use_fs=1, fs_hidden_units="[64]",
             fs1_context="c_hour_c,c_weekday_c,c_period_c,c_day_f", fs2_context="i_category_c,i_subcategory_c", num_heads=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,131072")
    ap.add_argument("--topk", default="1024x100", help="BxC of the TopK shape")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from helpers.CTRRunner import CTRRunner
    from models.context.DeepFM import DeepFMCTR
    from models.context.FinalMLP import FinalMLPCTR, FinalMLPTopK
    from rechorus_amd import graph as hgraph, nn as hnn

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(2)
    corpus = SimpleNamespace(n_users=N_USERS, n_items=N_ITEMS, user_feature_names=[], item_feature_names=ITEM, situation_feature_names=SIT,
                             feature_max=dict(VOCAB, user_id=N_USERS, item_id=N_ITEMS))

    def build(cls):
        args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=0, dropout=0, test_all=0,
                               loss_n="BCE" if cls is FinalMLPCTR else "BPR", **FLAGS)
        torch.manual_seed(1)
        m = cls(args, corpus).to(dev)
        with torch.no_grad():      # away from the near-zero native init: gates that are not all 1, a ReLU half active
            for p in m.parameters():
                p.mul_(20.0)
            for s in (1, 2):
                [mod for mod in getattr(m.fs_module, "fs%d_gate" % s).mlp if isinstance(mod, torch.nn.Linear)][-1].weight.mul_(4.0)
            m.fusion_module.w_xy.mul_(0.05)
        return m

    def feed(bs, C):
        f = {"user_id": torch.randint(1, N_USERS, (bs,), device=dev, generator=gen),
             "item_id": torch.randint(1, N_ITEMS, (bs, C), device=dev, generator=gen),
             "label": torch.randint(0, 2, (bs, 1), device=dev, generator=gen), "batch_size": bs, "phase": "train"}
        for name in ITEM + SIT:
            f[name] = torch.randint(0, VOCAB[name], (bs, C) if name.startswith("i_") else (bs,), device=dev, generator=gen)
        return f

    out = {"bench": "finalmlp", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "F": 8, "d": D_EMB, "flags": FLAGS,
           "hbm_peak_tbps": HBM_PEAK / 1e12, "gate": [], "fusion": [], "step": []}
    ra, _ = CTRRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    ra.train, ra.log_file, ra.optimizer, ra.lr, ra.l2, ra.graph, ra.engine = 1, "/tmp/bench_finalmlp/log.txt", "Adam", 1e-3, 0.0, 1, "dense"

    def step_times(model, fd):
        model.optimizer = CTRRunner(ra)._build_optimizer(model)
        model.train()

        def eager():
            model.optimizer.zero_grad()
            model.loss(model(fd)).backward()
            model.optimizer.step()
        res = {}
        res["eager_ms"], = alternate([eager], a.seconds, block=3, warmup=2)
        if hgraph.usable():
            step = hgraph.GraphedStep(model)
            for _ in range(step.WARMUP + 1):
                step.run(fd)
            res["replayed_ms"], = alternate([lambda: step.run(fd)], a.seconds, block=3, warmup=2)
        return res

    rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
    shapes = [(int(b), 1, FinalMLPCTR) for b in a.batches.split(",") if b]
    if a.topk:
        b, c = a.topk.split("x")
        shapes.append((int(b), int(c), FinalMLPTopK))
    for bs, C, cls in shapes:
        model = build(cls).train()
        fd = feed(bs, C)
        N = bs * C
        with torch.no_grad():
            X = model._flat_fields(fd, C).reshape(N, -1).clone()
            specs = [model._stream_spec(s, fd, C, False)[0] for s in (1, 2)]
            zins = [sp[0].clone() for sp in specs]
        lasts = [[m for m in getattr(model.fs_module, "fs%d_gate" % s).mlp if isinstance(m, torch.nn.Linear)][-1] for s in (1, 2)]
        firsts = [model.mlp1.mlp[0], model.mlp2.mlp[0]]
        params = [p for mod in lasts + firsts for p in mod.parameters()]
        dA = [torch.randn(N, f.out_features, device=dev, generator=gen) for f in firsts]
        ws = model._workspace

        def leaves():
            for p in params:
                p.grad = None
            return X.detach().requires_grad_(True), [z.detach().requires_grad_(True) for z in zins]

        def fused_gate():
            x, z = leaves()
            A1, A2 = hnn.finalmlp_gate(x, C, (z[0], lasts[0].weight, lasts[0].bias, firsts[0].weight, firsts[0].bias),
                                       (z[1], lasts[1].weight, lasts[1].bias, firsts[1].weight, firsts[1].bias), workspace=ws)
            torch.autograd.backward([A1, A2], dA)
            return [x.grad] + [t.grad for t in z] + [p.grad for p in params]

        def torch_gate():
            x, z = leaves()
            outs = []
            for s in (0, 1):
                zz = z[s] if z[s].shape[0] == N else z[s].unsqueeze(1).expand(-1, N // z[s].shape[0], -1).reshape(N, -1)
                gate = torch.sigmoid(lasts[s](zz)) * 2           # FinalMLP.py:203 / :219
                outs.append(torch.relu(firsts[s](x * gate)))    # :204 / :220, MLP_Block's first Linear + ReLU
            torch.autograd.backward(outs, dA)
            return [x.grad] + [t.grad for t in z] + [p.grad for p in params]

        res = {"B": bs, "C": C, "gate_rows": [int(z.shape[0]) for z in zins]}
        res["fused_ms"], res["torch_ms"] = alternate([fused_gate, torch_gate], a.seconds)
        res["torch_over_fused"] = res["torch_ms"] / res["fused_ms"]
        gf, gt = [g.clone() for g in fused_gate()], [g.clone() for g in torch_gate()]
        res["max_rel_diff_vs_torch"] = "%.3e" % max(rel(u, v) for u, v in zip(gf, gt))
        Dw = X.shape[1]
        H = [f.out_features for f in firsts]
        nbytes = 4 * (N * Dw + sum(z.numel() for z in zins) + N * sum(H)) + 4 * (N * Dw + sum(z.numel() for z in zins) + 2 * N * sum(H) + N * Dw
                                                                                 + sum(z.numel() for z in zins))
        res["bytes"], res["fraction_of_hbm_peak"] = nbytes, nbytes / (res["fused_ms"] * 1e-3) / HBM_PEAK
        out["gate"].append(res)

        fm = model.fusion_module
        fpar = list(fm.parameters())
        xs, ys = torch.rand(N, H[0], device=dev, generator=gen), torch.rand(N, H[1], device=dev, generator=gen)
        dout = torch.randn(bs, C, device=dev, generator=gen)

        def fusion(route):
            def fn():
                for p in fpar:
                    p.grad = None
                x, y = xs.detach().requires_grad_(True), ys.detach().requires_grad_(True)
                if route == "fused":
                    o = hnn.finalmlp_fusion(x.view(bs, C, -1), y.view(bs, C, -1), fm.w_xy, fm.w_x.weight, fm.w_x.bias, fm.w_y.weight,
                                            fm.w_y.bias, fm.num_heads, workspace=ws)
                else:
                    o = fm(x.view(bs, C, -1), y.view(bs, C, -1))
                o.backward(dout)
                return [x.grad, y.grad] + [p.grad for p in fpar]
            return fn
        res = {"B": bs, "C": C, "x_dim": H[0], "y_dim": H[1], "heads": fm.num_heads}
        res["fused_ms"], res["torch_ms"] = alternate([fusion("fused"), fusion("torch")], a.seconds)
        res["torch_over_fused"] = res["torch_ms"] / res["fused_ms"]
        gf, gt = [g.clone() for g in fusion("fused")()], [g.clone() for g in fusion("torch")()]
        res["max_rel_diff_vs_torch"] = "%.3e" % max(rel(u, v) for u, v in zip(gf, gt))
        nbytes = 4 * (N * sum(H) + N) + 4 * (2 * N * sum(H) + N)
        res["bytes"], res["fraction_of_hbm_peak"] = nbytes, nbytes / (res["fused_ms"] * 1e-3) / HBM_PEAK
        out["fusion"].append(res)
        if C == 1:
            out["step"].append({"B": bs, "finalmlp": step_times(model, fd), "deepfm": step_times(build_deepfm(DeepFMCTR, corpus, dev), fd)})
        del model

    def rnd(o):
        if isinstance(o, dict):
            return {k: rnd(v) for k, v in o.items()}
        if isinstance(o, list):
            return [rnd(v) for v in o]
        return round(o, 5) if isinstance(o, float) and abs(o) < 1e6 else o
    line = json.dumps(rnd(out))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
