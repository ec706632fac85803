"""AutoInt on the HIP engine vs the torch-op route on the same GPU in the same process: the model's own CPU-path modules
(utils.layers.MultiHeadAttention + the residual nn.Linear + relu) applied to device tensors, over the same gathered field vectors.
Prints ONE JSON line (and writes it to --out).

    python tools/bench_autoint.py [--batches 1024,131072] [--heads 1,2] [--layers 1,3] [--seconds 0.5] [--out FILE]

Every figure is a HIP-event time of warm calls, accumulated over at least --seconds per shape and route; the two routes alternate
block by block.  MIND shape: F = 8 fields, emb_size 64, attention_size 32.
  layers   per (B, heads, layers): forward + backward of the stack of interacting layers with every gradient (dX and the five
           weight gradients per layer): fused_ms (hnn.autoint_layer) / torch_ms, their ratio, the largest relative difference of the
           gradients between the two and of each against the same modules in float64 (with the count of ReLU masks on which each
           route disagrees with float64), and the fused route's achieved bytes/s against what it has to move -- X read + Y written in
           the forward, X, Y, dY read + dX written in the backward, per layer -- over the 8 TB/s HBM peak
  step     per (B, heads, layers): the whole AutoIntCTR training step (gather, layers, tower, BCE head, backward, dense Adam), eager
           and replayed from a hipGraph, on the fused route and on the torch-op route; the DeepFMCTR step on the same data beside it
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
F_FIELDS, D, A = 8, 64, 32
VOCAB = {"u_age_c": 10, "u_gender_c": 3, "i_category_c": 18, "i_subcategory_c": 300, "c_hour_c": 24, "c_weekday_c": 7}
N_USERS, N_ITEMS = 100001, 50001


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,131072")
    ap.add_argument("--heads", default="1,2")
    ap.add_argument("--layers", default="1,3")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from helpers.CTRRunner import CTRRunner
    from models.context.AutoInt import AutoIntCTR
    from models.context.DeepFM import DeepFMCTR
    from rechorus_amd import graph as hgraph

    class TorchRouteCTR(AutoIntCTR):
        """the same model with the interacting layers on torch ops (the CPU path's modules, on the device)"""

        def interacting_layers(self, x):
            outs = []
            for att, res in zip(self.autoint_attentions, self.residual_embeddings):
                x = (att(x, x, x) + res(x)).relu()
                outs.append(x)
            return outs

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(2)
    side = list(VOCAB)
    corpus = SimpleNamespace(n_users=N_USERS, n_items=N_ITEMS, user_feature_names=side[:2], item_feature_names=side[2:4],
                             situation_feature_names=side[4:], feature_max=dict(VOCAB, user_id=N_USERS, item_id=N_ITEMS))

    def build(cls, H, L):
        args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=0, dropout=0, test_all=0, emb_size=D, attention_size=A,
                               num_heads=H, num_layers=L, layers="[64]", loss_n="BCE")
        torch.manual_seed(1)
        m = cls(args, corpus).to(dev)
        with torch.no_grad():      # away from the near-zero native init: softmax rows that are not uniform, a ReLU half active
            for p in m.parameters():
                p.mul_(20.0)
        return m

    def feed(bs):
        f = {"user_id": torch.randint(1, N_USERS, (bs,), device=dev, generator=gen),
             "item_id": torch.randint(1, N_ITEMS, (bs, 1), device=dev, generator=gen),
             "label": torch.randint(0, 2, (bs, 1), device=dev, generator=gen), "batch_size": bs, "phase": "train"}
        for name, v in VOCAB.items():
            f[name] = torch.randint(0, v, (bs, 1) if name.startswith("i_") else (bs,), device=dev, generator=gen)
        return f

    out = {"bench": "autoint", "device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "F": F_FIELDS, "d": D, "A": A,
           "hbm_peak_tbps": HBM_PEAK / 1e12, "layers": [], "step": []}
    ra, _ = CTRRunner.parse_runner_args(argparse.ArgumentParser()).parse_known_args([])
    ra.train, ra.log_file, ra.optimizer, ra.lr, ra.l2, ra.graph, ra.engine = 1, "/tmp/bench_autoint/log.txt", "Adam", 1e-3, 0.0, 1, "dense"

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

    for bs in (int(x) for x in a.batches.split(",")):
        fd = feed(bs)
        deepfm = step_times(build_deepfm(DeepFMCTR, corpus, dev), fd)
        for H in (int(x) for x in a.heads.split(",")):
            for L in (int(x) for x in a.layers.split(",")):
                fused_m, torch_m = build(AutoIntCTR, H, L), build(TorchRouteCTR, H, L)
                torch_m.load_state_dict(fused_m.state_dict())
                with torch.no_grad():
                    X = fused_m._fused_fields(fd)[0].clone()
                dY = torch.randn(bs, 1, F_FIELDS, A, device=dev, generator=gen)

                def run(m):
                    params = [p for mod in (m.autoint_attentions, m.residual_embeddings) for p in mod.parameters()]

                    def fn():
                        for p in params:
                            p.grad = None
                        x = X.detach().requires_grad_(True)
                        m.interacting_layers(x)[-1].backward(dY)
                        return [x.grad] + [p.grad for p in params]
                    return fn
                f_fn, t_fn = run(fused_m), run(torch_m)
                res = {"B": bs, "heads": H, "layers": L}
                res["fused_ms"], res["torch_ms"] = alternate([f_fn, t_fn], a.seconds)
                res["torch_over_fused"] = res["torch_ms"] / res["fused_ms"]
                gf, gt = [g.clone() for g in f_fn()], [g.clone() for g in t_fn()]
                rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
                res["max_rel_diff_dX_vs_torch"] = "%.3e" % rel(gf[0], gt[0])
                res["max_rel_diff_weights_vs_torch"] = "%.3e" % max(rel(x, y) for x, y in zip(gf[1:], gt[1:]))
                # both fp32 routes against the same modules in float64 (the torch route's backward sends the round-off of a sum over
                # every score of the batch through the global-maximum shift of utils/layers.py:60 into one element)
                m64 = build(TorchRouteCTR, H, L)
                m64.load_state_dict(fused_m.state_dict())
                m64 = m64.double()
                p64 = [p for mod in (m64.autoint_attentions, m64.residual_embeddings) for p in mod.parameters()]
                x64 = X.detach().double().requires_grad_(True)
                m64.interacting_layers(x64)[-1].backward(dY.double())
                g64 = [x64.grad] + [p.grad for p in p64]
                res["fused_max_rel_err_vs_float64"] = "%.3e" % max(rel(x.double(), y) for x, y in zip(gf, g64))
                res["torch_max_rel_err_vs_float64"] = "%.3e" % max(rel(x.double(), y) for x, y in zip(gt, g64))
                # a pre-activation within round-off of the ReLU's kink flips Y > 0 on one route and not on another, and a flipped
                # mask moves one row of dX by a whole dY: count the mask elements on which each fp32 route disagrees with float64
                with torch.no_grad():
                    y64 = m64.interacting_layers(X.double())
                    yf, yt = fused_m.interacting_layers(X), torch_m.interacting_layers(X)
                res["relu_mask_flips_vs_float64"] = {
                    "fused": [int(((u > 0) != (w > 0)).sum()) for u, w in zip(yf, y64)],
                    "torch": [int(((u > 0) != (w > 0)).sum()) for u, w in zip(yt, y64)], "elements_per_layer": yf[0].numel()}
                # dX's error on the instances whose masks agree with float64 in every layer (fused route)
                same = torch.ones(X.shape[:2], dtype=torch.bool, device=dev)
                for u, w in zip(yf, y64):
                    same &= ((u > 0) == (w > 0)).flatten(2).all(-1)
                if bool(same.any()):
                    dxe = (gf[0].double() - g64[0]).abs()[same].max() / g64[0].abs().max()
                    res["fused_dX_err_vs_float64_where_masks_agree"] = "%.3e" % float(dxe)
                res["instances_with_a_flipped_mask_fused"] = int((~same).sum())
                del m64, p64, x64, g64, gf, gt, y64, yf, yt
                nbytes = 0
                for l in range(L):
                    din = D if l == 0 else A
                    nbytes += 4 * bs * F_FIELDS * ((din + A) + (din + 2 * A + din))
                res["bytes"] = nbytes
                res["fused_gbps"] = nbytes / (res["fused_ms"] * 1e-3) / 1e9
                res["fraction_of_hbm_peak"] = nbytes / (res["fused_ms"] * 1e-3) / HBM_PEAK
                out["layers"].append(res)
                st = {"B": bs, "heads": H, "layers": L, "fused": step_times(fused_m, fd), "torch": step_times(torch_m, fd), "deepfm": deepfm}
                out["step"].append(st)
                del fused_m, torch_m

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


def build_deepfm(cls, corpus, dev):
    import torch
    args = SimpleNamespace(device=dev, model_path="", buffer=1, num_neg=0, dropout=0, test_all=0, emb_size=D, layers="[64]", loss_n="BCE")
    torch.manual_seed(1)
    m = cls(args, corpus).to(dev)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(20.0)
    return m


if __name__ == "__main__":
    main()
