"""CPU: DIN's attention unit -- the float64 restatement (tests/din_np.py) against torch autograd on the reference's expression, the
folded first layer against the unfolded one, and the host logic of the rc_din_* entry points (no kernel is launched here)."""
import ctypes as C

import numpy as np
import pytest
import torch

import din_np
from rechorus_amd import _lib, engine

DEMO_SHAPES = [      # (H, L, att_layers) of the reference's four context demo lines: 3 or 7 fields x emb_size 64; history 10, 20, 40
    (192, 40, [64, 64]), (448, 40, [64, 64]), (192, 10, [256]), (448, 20, [64]), (192, 20, [64, 64, 64]), (448, 10, [256]),
]


def make_case(rng, B, C_, L, H, widths, scale=1.0):
    q = rng.standard_normal((B * C_, H)) * scale
    keys = rng.standard_normal((B, L, H)) * scale
    params, K = [], 4 * H
    for A in list(widths) + [1]:
        params.append((rng.standard_normal((A, K)) * (1.5 / np.sqrt(K)), rng.standard_normal(A) * 0.3))
        K = A
    lengths = rng.integers(0, L + 1, size=B)
    return q, keys, lengths, params


@pytest.mark.parametrize("B,C_,L,H,widths,drop", [(3, 1, 5, 8, [16], False), (2, 3, 4, 12, [16, 32], True), (4, 2, 7, 4, [16, 16, 16], True)])
def test_numpy_restatement_matches_torch_autograd(B, C_, L, H, widths, drop):
    rng = np.random.default_rng(5)
    q, keys, lengths, params = make_case(rng, B, C_, L, H, widths)
    N = B * C_
    keeps = [np.where(rng.random((N * L, A)) < 0.5, 0.0, 2.0) for A in widths] if drop else None
    d_out = rng.standard_normal((N, H))
    out, att, _ = din_np.forward(q, keys, lengths, C_, params, keeps)
    dq, dkeys, grads = din_np.backward(q, keys, lengths, C_, params, d_out, keeps)

    tq, tk = torch.tensor(q, requires_grad=True), torch.tensor(keys, requires_grad=True)
    tp = [(torch.tensor(W, requires_grad=True), torch.tensor(b, requires_grad=True)) for W, b in params]
    tkeeps = None if keeps is None else [torch.tensor(m) for m in keeps]
    tout, tatt = din_np.torch_reference(tq, tk, torch.tensor(lengths), C_, tp, tkeeps)
    (tout * torch.tensor(d_out)).sum().backward()
    np.testing.assert_allclose(out, tout.detach().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(att, tatt.detach().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(dq, tq.grad.numpy(), rtol=0, atol=1e-11)
    np.testing.assert_allclose(dkeys, tk.grad.numpy(), rtol=0, atol=1e-11)
    for (gW, gb), (W, b) in zip(grads, tp):
        np.testing.assert_allclose(gW.reshape(W.shape), W.grad.numpy(), rtol=0, atol=1e-11)
        np.testing.assert_allclose(gb, b.grad.numpy(), rtol=0, atol=1e-11)


def test_folded_first_layer_equals_the_unfolded_one():
    rng = np.random.default_rng(11)
    for B, C_, L, H, A in ((3, 4, 6, 12, 16), (2, 1, 40, 192, 64)):
        q, keys, _, params = make_case(rng, B, C_, L, H, [A])
        W1, b1 = params[0]
        a = din_np.first_layer_unfolded(q, keys, C_, W1, b1)
        b = din_np.first_layer_folded(q, keys, C_, W1, b1)
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max())


def test_flat_parameter_layout_round_trips():
    rng = np.random.default_rng(2)
    _, _, _, params = make_case(rng, 1, 1, 1, 8, [16, 32])
    flat = din_np.flat_params(params)
    assert flat.size == engine.din_param_count(8, [16, 32]) == 16 * 32 + 16 + 32 * 16 + 32 + 32 + 1
    back = din_np.split_flat(flat, 8, [16, 32])
    for (W, b), (W2, b2) in zip(params, back):
        np.testing.assert_array_equal(np.float32(W).reshape(W2.shape), W2)
        np.testing.assert_array_equal(np.float32(b), b2)


def test_check_shape_accepts_every_demo_shape_and_refuses_the_neighbours_of_each_bound():
    for H, L, widths in DEMO_SHAPES:
        for p in (0.0, 0.5, 0.8):
            engine.din_check_shape(H, L, widths, p)
    engine.din_check_shape(4, 1, [16])
    engine.din_check_shape(512, 64, [256])
    engine.din_check_shape(512, 64, [16, 240])
    refusals = [
        ((516, 10, [64]), "H=516"), ((0, 10, [64]), "H=0"), ((190, 10, [64]), "H=190"),
        ((192, 65, [64]), "L=65"), ((192, 0, [64]), "L=0"),
        ((192, 10, [24]), "width 24"), ((192, 10, [272]), "width 272"), ((192, 10, [0]), "width 0"),
        ((192, 10, [64, 64, 64, 64]), "4 hidden layers"), ((192, 10, []), "0 hidden layers"),
        ((192, 10, [64], 1.0), "dropout 1"), ((192, 10, [64], -0.1), "dropout -0.1"),
        ((192, 10, [16, 256]), "sum to 272"),       # the LDS budget: the widths of all layers together are at most 256
    ]
    for args, text in refusals:
        with pytest.raises(ValueError, match="rc_din_check_shape.*" + text):
            engine.din_check_shape(*args)


def test_entry_points_refuse_bad_arguments_before_anything_is_launched():
    lib = _lib.load()
    p, odd = C.c_void_p(64), C.c_void_p(68)      # never dereferenced; odd is not 16-byte aligned
    w = (C.c_int * 2)(64, 64)

    def fwd(q=p, out=p, ld_out=192, H=192, L=40, drop=0.0, seed=None, site0=0):
        return lib.rc_din_attention_fwd(q, p, p, p, 8, 1, L, H, 2, w, drop, seed, site0, out, ld_out, None, None)

    def bwd(ws_bytes=0, dq=p):
        return lib.rc_din_attention_bwd(p, p, p, p, p, 8, 1, 40, 192, 2, w, 0.0, None, 0, dq, p, p, p, ws_bytes, None)
    INVALID, WORKSPACE = -1, -2
    table = [
        (lambda: fwd(q=None), INVALID, b"rc_din_attention_fwd: null pointer"),
        (lambda: fwd(q=odd), INVALID, b"16-byte aligned"),
        (lambda: fwd(out=None), INVALID, b"rc_din_attention_fwd: null pointer"),
        (lambda: fwd(ld_out=190), INVALID, b"ld_out=190"),
        (lambda: fwd(ld_out=188), INVALID, b"ld_out=188"),
        (lambda: fwd(H=516), INVALID, b"H=516"),
        (lambda: fwd(L=65), INVALID, b"L=65"),
        (lambda: fwd(drop=0.5), INVALID, b"needs a device seed"),
        (lambda: fwd(drop=0.5, seed=p, site0=65535), INVALID, b"dropout site"),
        (lambda: bwd(dq=None), INVALID, b"rc_din_attention_bwd: null pointer"),
        (bwd, WORKSPACE, b"rc_din_attention_bwd: workspace 0 <"),
    ]
    for i, (call, code, text) in enumerate(table):
        got = call()
        msg = lib.rc_last_error_string()
        assert got == code and text in msg, (i, got, msg)


def test_backward_workspace_is_one_slice_per_workgroup():
    lib = _lib.load()
    w = (C.c_int * 2)(64, 64)
    H = 192
    P = 3 * 64 * H + 64 + 64 * 64 + 64 + 64 + 1          # [dWqd | dWkd | dWp] then the layout of the parameters
    for B, groups in ((1, 1), (7, 7), (512, 512), (65536, 512)):
        assert lib.rc_din_attention_bwd_workspace_bytes(B, H, 2, w) == -(-groups * P * 4 // 256) * 256, B
    big = (C.c_int * 1)(256)                                # 128 MiB of slices at the most: fewer workgroups at the widest shape
    P = 3 * 256 * 512 + 256 + 256 + 1
    assert lib.rc_din_attention_bwd_workspace_bytes(4096, 512, 1, big) == -(-((128 << 20) // (4 * P)) * P * 4 // 256) * 256
    assert lib.rc_din_attention_bwd_workspace_bytes(4096, 516, 1, big) == 0
