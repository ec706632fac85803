"""GPU: rc_kda_aggregate_fwd / rc_kda_aggregate_bwd against the float64 numpy restatement (tests/kda_np.py) on tests/kda_data.py's
arrays: both include_val settings at the floor of the envelope, at odd sizes, at the reference's default batch shape with R at its
bound and several backward tiles of candidates, and with L, R, V and F at their upper bounds.  The arrays hold id 0 in the middle
of histories, one row without any valid position (zeros, everything finite), delta_t = 0 and decays on both sides of both clamp
bounds (asserted here).

Tolerance: every quantity gets the larger of 2e-5 and four times the reference's own fp32 deviation on that quantity and that case
(tests/golden/kda_kernel_dev.json: the reference module in fp32 against its float64 run on the same arrays), as
max |got - want| / max |want| against the float64 oracle.  Every error and its bound are printed.  No comparison needs more."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
import kda_data as KD
import kda_np

pytestmark = pytest.mark.gpu
CAP = 2e-5
DEV = json.load(open(os.path.join(GOLDEN_DIR, "kda_kernel_dev.json")))
_oracle = {}


def rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def oracle(shape, include_val):
    """computed once per case and shared (forward, backward, determinism)"""
    key = (shape, include_val)
    if key not in _oracle:
        q = KD.kernel_inputs(shape)
        args = {k: q[k] for k in KD.ARG_ORDER}
        ctx, parts = kda_np.forward(**args, include_val=include_val, parts=True)
        _oracle[key] = (q, ctx, kda_np.backward(**args, d_context=q["d_context"], include_val=include_val), parts)
    return _oracle[key]


def on_gpu(q, cuda, include_val):
    t = {k: torch.from_numpy(q[k]).to(cuda) for k in KD.ARG_ORDER + ("d_context",)}
    if not include_val:
        t["value"] = None
    return t


@pytest.fixture(scope="module")
def eng(cuda):
    from rechorus_amd import engine
    return engine


@pytest.mark.parametrize("include_val", [True, False])
@pytest.mark.parametrize("shape", KD.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_match_the_float64_oracle(shape, include_val, cuda, eng):
    q, ctx64, grads64, parts = oracle(shape, include_val)
    B, C, L, R, V, F = shape
    valid = parts["valid"]
    if L > 1:   # the case really holds what it is meant to hold
        assert min(KD.clamp_shares(parts["x"], valid)) >= 0.1
        assert (q["hist"][:, 1:-1] == 0).any() and (q["delta_t"][valid] == 0).any()
    t = on_gpu(q, cuda, include_val)
    args = [t[k] for k in KD.ARG_ORDER]
    ctx = eng.kda_aggregate_fwd(*args, include_val)
    grads = dict(zip(KD.GRADS, eng.kda_aggregate_bwd(*args, t["d_context"], include_val)))
    torch.cuda.synchronize()
    dev = DEV[KD.case_name(shape, include_val)]
    checks = [("context", ctx.cpu().numpy(), ctx64)] + [(k, grads[k].cpu().numpy(), grads64[k]) for k in KD.GRADS if grads64[k] is not None]
    assert (grads["dvalue"] is None) == (not include_val)
    for key, got, want in checks:
        assert np.isfinite(got).all(), key
        err, tol = rel(got, want), max(CAP, 4 * dev[key])
        print(f"kda kernel {KD.case_name(shape, include_val)} {key}: error {err:.3e} bound {tol:.3e}")
        assert err <= tol, (shape, include_val, key, err, tol)
    empty = ~valid.any(axis=1)
    assert empty.any() == (B > 2)
    if empty.any():      # a row without a valid position: a zero context and zero gradients
        assert not ctx.cpu().numpy()[empty].any()
        for k in ("dseq", "dtarget") + (("dvalue",) if include_val else ()):
            assert not grads[k].cpu().numpy()[empty].any(), k
    # invalid positions receive no gradient
    assert not grads["dseq"].cpu().numpy()[~valid].any()


@pytest.mark.parametrize("shape", [KD.KERNEL_SHAPES[1], KD.KERNEL_SHAPES[2]], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bit_equal(shape, cuda, eng):
    q = oracle(shape, True)[0]
    t = on_gpu(q, cuda, True)
    args = [t[k] for k in KD.ARG_ORDER]
    first = [eng.kda_aggregate_fwd(*args, True).clone()] + [x.clone() for x in eng.kda_aggregate_bwd(*args, t["d_context"], True)]
    second = [eng.kda_aggregate_fwd(*args, True)] + list(eng.kda_aggregate_bwd(*args, t["d_context"], True))
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_the_autograd_node_hands_every_input_its_gradient(cuda):
    from rechorus_amd import nn as hnn
    shape = KD.KERNEL_SHAPES[1]
    for include_val in (True, False):
        q, _, grads64, _ = oracle(shape, include_val)
        t = on_gpu(q, cuda, True)
        leaves = {k: t[k].clone().requires_grad_() for k in ("seq", "target", "value", "rel", "freq_real", "freq_imag")}
        ctx = hnn.kda_aggregate(leaves["seq"], t["hist"], t["delta_t"], leaves["target"], leaves["value"], leaves["rel"],
                                leaves["freq_real"], leaves["freq_imag"], include_val)
        ctx.backward(t["d_context"])
        dev = DEV[KD.case_name(shape, include_val)]
        for name, key in (("seq", "dseq"), ("target", "dtarget"), ("value", "dvalue"), ("rel", "drel"), ("freq_real", "dfreq_real"),
                          ("freq_imag", "dfreq_imag")):
            if grads64[key] is None:
                assert leaves[name].grad is None       # value is not read without include_val
                continue
            assert rel(leaves[name].grad.cpu().numpy(), grads64[key]) <= max(CAP, 4 * dev[key]), (include_val, name)


def test_shapes_outside_the_envelope_are_refused(cuda, eng):
    q = KD.kernel_inputs(KD.KERNEL_SHAPES[1])
    t = on_gpu(q, cuda, True)
    for bad in ((12, 7, 3, 5), (256, 7, 3, 5), (32, 0, 3, 5), (32, 65, 3, 5), (32, 7, 0, 5), (32, 7, 9, 5), (32, 7, 3, 1), (32, 7, 3, 130)):
        with pytest.raises(ValueError):
            eng.kda_check_shape(*bad)
    for ok in ((16, 1, 1, 2), (128, 64, 8, 129)):
        eng.kda_check_shape(*ok)
    with pytest.raises(ValueError):      # V = 24 rows
        eng.kda_aggregate_fwd(t["seq"][:, :, :24].contiguous(), t["hist"], t["delta_t"], t["target"][:, :, :24].contiguous(),
                              t["value"][..., :24].contiguous(), t["rel"][:, :24].contiguous(), t["freq_real"], t["freq_imag"], True)
    with pytest.raises(ValueError):      # hist of another length
        eng.kda_aggregate_fwd(t["seq"], t["hist"][:, :-1].contiguous(), t["delta_t"], t["target"], t["value"], t["rel"],
                              t["freq_real"], t["freq_imag"], True)
