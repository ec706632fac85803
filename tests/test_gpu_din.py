"""GPU: rc_din_attention_fwd / rc_din_attention_bwd through the engine wrappers against the float64 restatement (tests/din_np.py,
the UNFOLDED form of the reference), on both sides of every launch-geometry change: a tile is 64 rows (c, l) of one batch row with
CT = max(1, 64 // L) candidates, so L = 1 / 10 / 20 / 40 / 64 give 64 / 6 / 3 / 1 / 1 candidates per tile; C below, at and past CT
(one row's candidates span workgroups); H below and past the 16-wide reduction chunk; 1 to 3 layers of 16 to 256 units.

Tolerance: every comparison is against float64 and gets 10 x the reference expression's OWN fp32 error on that quantity and
that case -- the concatenated form in float32 torch ops on the CPU with autograd, against the same float64 restatement
(fp32_deviation) -- capped at the project's 2e-5; both are relative to the largest magnitude of the compared array.  No comparison
needs more: the folded first layer and the per-workgroup partial sums stay within about 3 x the expression's own error.  Every
error and its bound are printed; the largest are in profiles/din_tolerances.txt."""
import numpy as np
import pytest
import torch

import din_np
from oracle import mlp_oracle

pytestmark = pytest.mark.gpu

TOL = 2e-5
SEED = 0x1234567887654321

SHAPES = [      # (B, C, L, H, widths)
    (1, 1, 1, 4, [16]),
    (3, 1, 64, 512, [256]),
    (2, 101, 10, 192, [64, 64, 64]),
    (33, 1, 40, 448, [64, 64]),
    (7, 5, 20, 12, [16, 240]),          # the widths of all layers together are at most 256 (LDS): [16, 256] is refused
    (5, 7, 10, 20, [32]),               # N = 35 is no multiple of the 6 candidates a tile holds at L = 10; H = 20 ends inside a chunk
    (3, 64, 1, 16, [16, 16]),           # L = 1: 64 candidates fill a tile exactly
    (2, 65, 1, 8, [16]),                # ... and one more
]


@pytest.fixture(scope="module")
def eng(cuda):
    from rechorus_amd import engine
    return engine


def make_case(B, C, L, H, widths, lengths="mixed", seed=0):
    rng = np.random.default_rng(seed + 1000 * B + 10 * L + H)
    q = rng.standard_normal((B * C, H)).astype(np.float32)
    keys = rng.standard_normal((B, L, H)).astype(np.float32)
    params, K = [], 4 * H
    for j, A in enumerate(list(widths) + [1]):
        # pre-activations of every layer with a standard deviation of about 1: the attention weights spread
        sd = (1.0 / np.sqrt(1.5 * K)) if j == 0 else (2.0 / np.sqrt(K))
        params.append(((rng.standard_normal((A, K)) * sd).astype(np.float32), (rng.standard_normal(A) * 0.3).astype(np.float32)))
        K = A
    if lengths == "mixed":
        lens = rng.integers(1, L + 1, size=B)
        lens[0] = L
        if B > 1:
            lens[-1] = 1
        if B > 2:
            lens[1] = 0                  # one row without history
    else:
        lens = np.full(B, {"ones": 1, "full": L}[lengths])
    d_out = rng.standard_normal((B * C, H)).astype(np.float32)
    return q, keys, lens.astype(np.int64), params, d_out


def run_gpu(eng, cuda, q, keys, lens, params, d_out, C, widths, drop_p=0.0, site0=0):
    t = lambda x: torch.as_tensor(x).to(cuda)
    flat = t(din_np.flat_params(params))
    seed = torch.tensor([SEED], dtype=torch.int64, device=cuda) if drop_p else None
    tq, tk, tl, tg = t(q), t(keys), t(lens), t(d_out)
    out, att = eng.din_attention_fwd(tq, tk, tl, flat, C, widths, drop_p, seed, site0, want_att=True)
    dq, dkeys, dflat = eng.din_attention_bwd(tq, tk, tl, flat, tg, C, widths, drop_p, seed, site0)
    torch.cuda.synchronize()
    return {"out": out, "att": att, "dq": dq, "dkeys": dkeys, "dparams": dflat}


def reference(q, keys, lens, params, d_out, C, keeps=None):
    out, att, _ = din_np.forward(q, keys, lens, C, params, keeps)
    dq, dkeys, grads = din_np.backward(q, keys, lens, C, params, d_out, keeps)
    return {"out": out, "att": att, "dq": dq, "dkeys": dkeys, "dparams": din_np.flat_grads(grads)}


def fp32_deviation(q, keys, lens, params, d_out, C, want, keeps=None):
    """the concatenated expression's own fp32 error on every quantity (torch on the CPU, autograd), relative to max |float64|"""
    tq, tk = torch.tensor(q, requires_grad=True), torch.tensor(keys, requires_grad=True)
    tp = [(torch.tensor(W, requires_grad=True), torch.tensor(b, requires_grad=True)) for W, b in params]
    tkeeps = None if keeps is None else [torch.tensor(m) for m in keeps]
    out, att = din_np.torch_reference(tq, tk, torch.tensor(lens), C, tp, tkeeps)
    (out * torch.tensor(d_out)).sum().backward()
    got = {"out": out.detach(), "att": att.detach(), "dq": tq.grad, "dkeys": tk.grad,
           "dparams": torch.cat([t.grad.reshape(-1) for pair in tp for t in pair])}
    return {k: float(np.abs(got[k].numpy().astype(np.float64) - want[k]).max() / max(np.abs(want[k]).max(), 1e-30)) for k in got}


def check(got, want, what, dev):
    for k, ref in want.items():
        g = got[k].detach().cpu().numpy().astype(np.float64)
        assert g.shape == ref.shape, (what, k)
        assert np.isfinite(g).all(), (what, k)
        err = np.abs(g - ref).max() / max(np.abs(ref).max(), 1e-30) if ref.size else 0.0
        tol = min(TOL, 10 * dev[k])
        print(f"din {what} {k}: max error / max |ref| = {err:.3e}  bound {tol:.3e} (fp32 torch expression: {dev[k]:.3e})")
        assert err <= tol, (what, k, err, tol)


@pytest.mark.parametrize("B,C,L,H,widths", SHAPES)
def test_attention_forward_and_backward_match_float64(eng, cuda, B, C, L, H, widths):
    q, keys, lens, params, d_out = make_case(B, C, L, H, widths)
    got = run_gpu(eng, cuda, q, keys, lens, params, d_out, C, widths)
    want = reference(q, keys, lens, params, d_out, C)
    check(got, want, f"B{B} C{C} L{L} H{H} {widths}", fp32_deviation(q, keys, lens, params, d_out, C, want))
    # a history of length 0 gives a zero row and takes no gradient
    for b in np.nonzero(lens == 0)[0]:
        assert not got["out"][b * C:(b + 1) * C].any() and not got["att"][b * C:(b + 1) * C].any()
        assert not got["dkeys"][b].any()


@pytest.mark.parametrize("lengths", ["ones", "full"])
def test_all_lengths_one_and_all_lengths_full(eng, cuda, lengths):
    B, C, L, H, widths = 5, 4, 20, 24, [32, 16]
    q, keys, lens, params, d_out = make_case(B, C, L, H, widths, lengths)
    got = run_gpu(eng, cuda, q, keys, lens, params, d_out, C, widths)
    want = reference(q, keys, lens, params, d_out, C)
    check(got, want, lengths, fp32_deviation(q, keys, lens, params, d_out, C, want))


def test_padded_key_positions_are_never_read_as_valid(eng, cuda):
    B, C, L, H, widths = 6, 7, 10, 20, [32, 16]
    q, keys, lens, params, d_out = make_case(B, C, L, H, widths)
    clean = run_gpu(eng, cuda, q, keys, lens, params, d_out, C, widths)
    poisoned = keys.copy()
    for b in range(B):
        poisoned[b, lens[b]:] = np.nan
    got = run_gpu(eng, cuda, q, poisoned, lens, params, d_out, C, widths)
    for k in clean:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], clean[k]), k


@pytest.mark.parametrize("p", [0.5, 0.8])
def test_dropout_follows_the_linear_layers_mask_rule(eng, cuda, p):
    B, C, L, H, widths, site0 = 9, 3, 10, 16, [64, 32], 5
    q, keys, lens, params, d_out = make_case(B, C, L, H, widths)
    N = B * C
    keeps = [mlp_oracle.dropout_keep(SEED, site0 + j, N * L, A, p) for j, A in enumerate(widths)]
    kept, n = sum(int((k > 0).sum()) for k in keeps), sum(k.size for k in keeps)
    assert abs(kept / n - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / n)
    got = run_gpu(eng, cuda, q, keys, lens, params, d_out, C, widths, drop_p=p, site0=site0)
    want = reference(q, keys, lens, params, d_out, C, keeps)
    check(got, want, f"dropout {p}", fp32_deviation(q, keys, lens, params, d_out, C, want, keeps))
    # the mask matters: without it the result is another one
    plain = reference(q, keys, lens, params, d_out, C)
    assert np.abs(plain["out"] - got["out"].cpu().numpy()).max() > 100 * TOL * np.abs(plain["out"]).max()


def test_two_runs_are_bit_equal(eng, cuda):
    B, C, L, H, widths = 40, 9, 10, 192, [64, 64]
    q, keys, lens, params, d_out = make_case(B, C, L, H, widths)
    a = run_gpu(eng, cuda, q, keys, lens, params, d_out, C, widths, drop_p=0.5)
    b = run_gpu(eng, cuda, q, keys, lens, params, d_out, C, widths, drop_p=0.5)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_out_lands_inside_a_wider_buffer(eng, cuda):
    B, C, L, H, widths = 4, 3, 10, 12, [16]
    q, keys, lens, params, d_out = make_case(B, C, L, H, widths)
    t = lambda x: torch.as_tensor(x).to(cuda)
    flat = t(din_np.flat_params(params))
    wide = torch.full((B * C, 3 * H + 4), 7.0, device=cuda)
    eng.din_attention_fwd(t(q), t(keys), t(lens), flat, C, widths, out=wide[:, H:2 * H])
    plain, _ = eng.din_attention_fwd(t(q), t(keys), t(lens), flat, C, widths)
    assert torch.equal(wide[:, H:2 * H], plain)
    assert bool((wide[:, :H] == 7.0).all()) and bool((wide[:, 2 * H:] == 7.0).all())


def test_autograd_node_hands_every_layer_its_gradient(eng, cuda):
    from rechorus_amd import nn as rnn
    B, C, L, H, widths = 6, 4, 10, 24, [32, 16]
    q, keys, lens, params, d_out = make_case(B, C, L, H, widths)
    t = lambda x: torch.as_tensor(x).to(cuda)
    tq, tk = t(q).requires_grad_(), t(keys).requires_grad_()
    tp = [(t(W).requires_grad_(), t(b).requires_grad_()) for W, b in params]
    out, att = rnn.din_attention(tq, tk, t(lens), C, tp)
    (out * t(d_out)).sum().backward()
    want = reference(q, keys, lens, params, d_out, C)
    got = {"out": out, "att": att, "dq": tq.grad, "dkeys": tk.grad, "dparams": torch.cat([t.grad.reshape(-1) for pair in tp for t in pair])}
    check(got, want, "autograd", fp32_deviation(q, keys, lens, params, d_out, C, want))


def test_no_tensor_of_n_l_4h_elements_exists(eng, cuda):
    """N = 4,096 (B = 512, C = 8), L = 64, H = 512, layers [64]: the materialised [N, L, 4H] input alone would be 2.1 GB; one forward
    + backward may allocate less than 256 MB beyond its inputs and the declared workspace"""
    B, C, L, H, widths = 512, 8, 64, 512, [64]
    g = torch.Generator(device=cuda).manual_seed(3)
    q = torch.randn((B * C, H), device=cuda, generator=g)
    keys = torch.randn((B, L, H), device=cuda, generator=g)
    d_out = torch.randn((B * C, H), device=cuda, generator=g)
    lens = torch.randint(0, L + 1, (B,), device=cuda, generator=g)
    flat = torch.randn(eng.din_param_count(H, widths), device=cuda, generator=g) * 0.02
    n, arr = eng._din_widths(widths)
    ws_bytes = eng._lib.load().rc_din_attention_bwd_workspace_bytes(B, H, n, arr)
    eng.workspace(ws_bytes, cuda, "din_bwd")            # the declared workspace, allocated before the measurement starts
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(cuda)
    before = torch.cuda.memory_allocated(cuda)
    out, att = eng.din_attention_fwd(q, keys, lens, flat, C, widths, want_att=True)
    dq, dkeys, dflat = eng.din_attention_bwd(q, keys, lens, flat, d_out, C, widths)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(cuda) - before
    print(f"din memory: rise {rise / 2 ** 20:.1f} MiB, declared workspace {ws_bytes / 2 ** 20:.1f} MiB")
    assert rise < 256 * 2 ** 20
    for x in (out, att, dq, dkeys, dflat):
        assert bool(torch.isfinite(x).all())
