"""The gated first layers of FinalMLP at the MIND demo widths (D = 512, G = 64, H = 64 / 256, one gate row per instance), N instances:
the forward and the backward timed apart on the fused route and on torch ops (HIP events, warm calls), and both fp32 routes against
the float64 restatement (tests/finalmlp_np.py) computed on the host: the ReLU masks on which each route disagrees with float64, every
fused gradient given the kernel's own masks, and dX of both routes against float64's masks.  Prints two JSON lines (the second holds
everything; profiles/finalmlp_gate_probe.json is that line).

    python tools/finalmlp_gate_probe.py 131072
"""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import finalmlp_np as fnp
from rechorus_amd import engine

dev = torch.device("cuda:0")
N, C, D, G, H = int(sys.argv[1]), 1, 512, (64, 64), (64, 256)
rng = np.random.default_rng(1)
X = rng.standard_normal((N, D)).astype(np.float32)
def stream(G, H):
    return [rng.standard_normal((N, G)).astype(np.float32), (rng.standard_normal((D, G)) * 1.5 / np.sqrt(G)).astype(np.float32),
            (0.5 * rng.standard_normal(D)).astype(np.float32), (rng.standard_normal((H, D)) / np.sqrt(D)).astype(np.float32),
            (0.5 * rng.standard_normal(H)).astype(np.float32)]
st = [stream(G[s], H[s]) for s in (0, 1)]
dA = [rng.standard_normal((N, H[s])).astype(np.float32) for s in (0, 1)]
Xd = torch.from_numpy(X).to(dev)
std = [[torch.from_numpy(a).to(dev) for a in s] for s in st]
dAd = [torch.from_numpy(a).to(dev) for a in dA]
full = [tuple(std[s]) + (0.0, None, 0) for s in (0, 1)]
ws = engine.FinalMLPWorkspace()

def timed(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps

A = engine.finalmlp_gate_fwd(Xd, C, *full)
out = {"N": N}
out["fused_fwd_ms"] = timed(lambda: engine.finalmlp_gate_fwd(Xd, C, *full))
out["fused_bwd_ms"] = timed(lambda: engine.finalmlp_gate_bwd(Xd, C, *full, A[0], dAd[0], A[1], dAd[1], workspace=ws))

def torch_fwd(x, z, par):
    return [torch.relu((x * (torch.sigmoid(z[s] @ par[s][0].T + par[s][1]) * 2)) @ par[s][2].T + par[s][3]) for s in (0, 1)]
par = [[t for t in std[s][1:]] for s in (0, 1)]
zin = [std[s][0] for s in (0, 1)]
with torch.no_grad():
    out["torch_fwd_ms"] = timed(lambda: torch_fwd(Xd, zin, par))
    At = torch_fwd(Xd, zin, par)
def torch_both():
    x = Xd.detach().requires_grad_(True)
    z = [t.detach().requires_grad_(True) for t in zin]
    p = [[t.detach().requires_grad_(True) for t in q] for q in par]
    torch.autograd.backward(torch_fwd(x, z, p), dAd)
    return x.grad
out["torch_fwd_bwd_ms"] = timed(torch_both, reps=5)
dX_t = torch_both().cpu().numpy()
print(json.dumps(out), flush=True)

dX_f, g1, g2 = engine.finalmlp_gate_bwd(Xd, C, *full, A[0], dAd[0], A[1], dAd[1], workspace=ws)
torch.cuda.synchronize()
dX_f = dX_f.cpu().numpy()
want_kernel_mask, want_own_mask = 0.0, 0.0
for s in (0, 1):
    _, pre = fnp.gate_fwd(X, st[s], C)
    on_f, on_t, on64 = A[s].cpu().numpy() != 0, At[s].cpu().numpy() != 0, pre > 0
    ff, ft = on_f != on64, on_t != on64
    out["stream%d" % (s + 1)] = {"mask_flips_fused": int(ff.sum()), "mask_flips_torch": int(ft.sum()), "elements": int(pre.size),
                                 "largest_flipped_pre_over_max_fused": float(np.abs(pre[ff]).max(initial=0.0) / np.abs(pre).max()),
                                 "largest_flipped_pre_over_max_torch": float(np.abs(pre[ft]).max(initial=0.0) / np.abs(pre).max())}
    res = fnp.gate_bwd(X, st[s], C, on_f.astype(np.float64), dA[s])
    want_kernel_mask = want_kernel_mask + res[0]
    grads = g1 if s == 0 else g2
    out["stream%d" % (s + 1)]["fused_grad_err_given_its_mask"] = {n: "%.2e" % fnp.rel_err(t.cpu().numpy(), w) for n, t, w in zip(("dZin", "dWg", "dbg", "dW", "db"), grads, res[1:])}
    want_own_mask = want_own_mask + fnp.gate_bwd(X, st[s], C, on64.astype(np.float64), dA[s])[0]
    del pre, res
out["fused_dX_err_given_its_masks"] = "%.2e" % fnp.rel_err(dX_f, want_kernel_mask)
out["fused_dX_err_vs_float64_masks"] = "%.2e" % fnp.rel_err(dX_f, want_own_mask)
out["torch_dX_err_vs_float64_masks"] = "%.2e" % fnp.rel_err(dX_t, want_own_mask)
out["fused_vs_torch_dX"] = "%.2e" % fnp.rel_err(dX_f, dX_t.astype(np.float64))
print(json.dumps(out), flush=True)
