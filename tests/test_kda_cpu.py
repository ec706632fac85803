"""CPU: tests/kda_np.py, the float64 numpy restatement of KDA's relational dynamic aggregation and of its gradients, against what
the reference computed (tests/golden/make_golden_kda.py):
  * kda_agg_*.npz -- the reference module's float64 context and autograd gradients on tests/kda_data.py's arrays, both include_val
    settings, for the kernel-test shapes small enough to commit;
  * kda_d*.npz -- the aggregation's fp32 output inside the whole model, at the bound the GPU tests use (the larger of 2e-5 and four
    times the reference's own fp32 deviation, dev/context);
and its properties: the gradients are the derivative of its forward (central differences), a row without a valid position gives
zeros, the clamp passes at its bounds."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, golden_cases, load_golden
import kda_data as KD
import kda_model_cases as MC
import kda_np

AGG = golden_cases("kda_agg_")


def rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def test_the_recorded_cases_are_there():
    assert len(AGG) == 6 and sorted(golden_cases("kda_d")) == sorted(MC.CASES)
    dev = json.load(open(os.path.join(GOLDEN_DIR, "kda_kernel_dev.json")))
    assert sorted(dev) == sorted(KD.case_name(s, v) for s in KD.KERNEL_SHAPES for v in (0, 1))
    for name, rec in dev.items():
        assert set(rec) == {"context", "dseq", "dtarget", "drel", "dfreq_real", "dfreq_imag"} | ({"dvalue"} if name.endswith("val1") else set())
        assert all(0 <= v < 1e-5 for v in rec.values()), name     # the reference's fp32 run is within the project's cap at every shape


@pytest.mark.parametrize("name", AGG)
def test_forward_and_gradients_equal_the_reference_in_float64(name):
    g = load_golden(name)
    shape = next(s for s in KD.KERNEL_SHAPES for v in (0, 1) if "kda_agg_" + KD.case_name(s, v) == name)
    include_val = name.endswith("val1")
    q, keep = KD.kernel_inputs(shape), g["keep"]
    assert np.array_equal(keep, (q["hist"] > 0).any(axis=1))
    args = {k: q[k] for k in KD.ARG_ORDER}
    ctx = kda_np.forward(**args, include_val=include_val)
    grads = kda_np.backward(**args, d_context=q["d_context"], include_val=include_val)
    assert rel(ctx[keep], g["context"]) < 1e-12
    assert not ctx[~keep].any()                                   # here a row without a valid position gives zeros, not NaN
    for k in ("dseq", "dtarget") + (("dvalue",) if include_val else ()):
        assert rel(grads[k][keep], g[k]) < 1e-11, k
        assert not grads[k][~keep].any(), k
    for k in ("drel", "dfreq_real", "dfreq_imag"):
        assert rel(grads[k], g[k]) < 1e-11, k
    assert (grads["dvalue"] is None) == (not include_val)


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_the_aggregation_inside_the_model_equals_the_golden(name):
    g = load_golden(name)
    model, _, _ = MC.build(name)
    model = MC.scale_to_p0(model, g)
    E = model.entity_embeddings.weight.detach().numpy().astype(np.float64)
    agg = model.relational_dynamic_aggregation
    hist = g["b1/history_items"]
    ctx = kda_np.forward(E[hist], hist, g["b1/history_delta_t"].astype(np.float32), E[g["b1/item_id"]], E[g["b1/item_val"]],
                         model.relation_embeddings.weight.detach().numpy(), agg.freq_real.weight.detach().numpy(),
                         agg.freq_imag.weight.detach().numpy(), include_val=bool(model.include_val))
    err, tol = rel(ctx, g["context"]), max(2e-5, 4 * float(g["dev/context"]))
    print(f"kda_np {name} context: error {err:.3e} bound {tol:.3e}")
    assert err <= tol


def test_gradients_are_the_derivative_of_the_forward():
    shape = (2, 3, 5, 2, 16, 4)
    q = KD.kernel_inputs(shape, seed=3)
    args = {k: np.asarray(q[k], np.float64) if q[k].dtype == np.float32 else q[k] for k in KD.ARG_ORDER}
    # keep every raw decay away from the clamp's kinks, where no derivative exists
    x = kda_np.decay_raw(args["delta_t"], args["freq_real"], args["freq_imag"])[0]
    assert np.abs(x).min() > 1e-4 and np.abs(x - 1).min() > 1e-4
    g = np.asarray(q["d_context"], np.float64)
    grads = kda_np.backward(**args, d_context=g)
    rng = np.random.default_rng(0)
    for name, key in (("seq", "dseq"), ("target", "dtarget"), ("value", "dvalue"), ("rel", "drel"), ("freq_real", "dfreq_real"),
                      ("freq_imag", "dfreq_imag")):
        direction = rng.normal(size=args[name].shape)
        h = 1e-6
        up = kda_np.forward(**{**args, name: args[name] + h * direction})
        down = kda_np.forward(**{**args, name: args[name] - h * direction})
        numeric = ((up - down) * g).sum() / (2 * h)
        analytic = (grads[key] * direction).sum()
        assert abs(numeric - analytic) <= 1e-6 * max(abs(analytic), 1.0), (name, numeric, analytic)


def test_the_clamp_passes_at_its_bounds_and_not_outside():
    # F = 2, delta_t = 0: x = (real[0] + real[1]) / 4, so x = 0, 1 exactly, and one value on either side
    seq, target, value = np.ones((4, 1, 16)), np.ones((4, 1, 16)), np.zeros((4, 1, 4, 16))
    hist, dt = np.ones((4, 1), dtype=np.int64), np.zeros((4, 1))
    fre = np.array([[0., 0.], [4., 0.], [-2., 0.], [8., 0.]])       # x = 0, 1, -0.5, 2 for relation 0 .. 3
    grads = kda_np.backward(seq, hist, dt, target, value, np.ones((4, 16)), fre, np.zeros((4, 2)), np.ones((4, 1, 4, 16)))
    assert (grads["dfreq_real"][:2] != 0).all() and not grads["dfreq_real"][2:].any()
