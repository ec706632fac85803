"""CPU: FinalMLP's float64 restatement (tests/finalmlp_np.py) and the model file's torch path against the goldens of the reference
(tests/golden/make_golden_finalmlp.py); the state_dict's keys, order and initial bits; every refusal at construction;
rc_finalmlp_check_shape at both edges of each limit; where the classes are defined; the goldens' sizes."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT, golden_cases, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
PLUGIN = os.path.join(ROOT, "rechorus_amd", "rechorus")
if PLUGIN not in sys.path:
    sys.path.insert(0, PLUGIN)
import finalmlp_np as fnp  # noqa: E402
from finalmlp_np import TOL, rel_err  # noqa: E402

CASES = golden_cases("finalmlp_")
CPU = torch.device("cpu")


def test_goldens_present_and_small():
    assert len(CASES) == 5, CASES
    for c in CASES:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, c + ".npz")) <= 512 * 1024, c
    cfgs = [fnp.config(load_golden(c)) for c in CASES]
    assert sum(c["ctr"] for c in cfgs) == 2 and any(not c["flags"]["use_fs"] for c in cfgs)
    assert any(len(c["context_features"]) == 3 and c["flags"]["emb_size"] == 4 for c in cfgs)      # the floor of the envelope


def _check(got, want, what, bound=TOL, floor=0.0):
    if torch.is_tensor(got):
        got = got.detach().numpy()
    err = rel_err(np.asarray(got).reshape(np.shape(want)), want, floor)
    assert err <= bound, f"{what}: largest error / largest entry {err:.3e} > {bound:g}"


@pytest.mark.parametrize("case", CASES)
def test_restatement_against_golden(case):
    g = load_golden(case)
    cfg = fnp.config(g)
    out = fnp.model64(g).forward(fnp.batch(g, 1))
    for key in ("gate1", "gate2", "A1", "A2"):
        if key in g:
            _check(out[key], g[key], f"{case} {key}")
    _check(out["prediction"], g["pred"].reshape(out["prediction"].shape), case + " pred", fnp.bound_for(g, "pred")[0])
    pred = torch.from_numpy(np.asarray(out["prediction"]))
    o = {"prediction": pred, "label": torch.from_numpy(fnp.batch(g, 1)["label"]).view(-1)} if cfg["ctr"] else {"prediction": pred}
    loss = fnp.torch_loss(g, o).item()
    assert abs(loss - float(g["loss"])) <= TOL * max(1.0, abs(float(g["loss"]))), (case, loss, float(g["loss"]))


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_model_torch_path_against_golden(case, double):
    """the model file off the GPU: prediction, loss and every gradient (fp32, and in float64 where no numeric field stops it)"""
    g = load_golden(case)
    cfg = fnp.config(g)
    numeric = any(f.endswith("_f") for f in cfg["context_features"])
    if double and numeric:
        return      # (`.float()` on the numeric values, as in the reference)
    model = fnp.build_model(g, CPU)
    if double:
        model = model.double()
    model.train()
    out = model(fnp.feed(g, 1, CPU))
    loss = fnp.torch_loss(g, out)
    loss.backward()
    _check(out["prediction"], g["pred"], case + " pred", fnp.bound_for(g, "pred")[0])
    assert abs(loss.item() - float(g["loss"])) <= TOL * max(1.0, abs(float(g["loss"])))
    for k, p in model.named_parameters():
        _check(p.grad, g["G/" + k], f"{case} grad {k}", fnp.bound_for(g, k)[0], fnp.grad_floor(g))


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_order_and_initial_bits(case):
    g = load_golden(case)
    model = fnp.build_model(g, CPU, which=None, seed=fnp.config(g)["seed"])
    sd = model.state_dict()
    assert list(sd.keys()) == fnp.state_keys(g)
    for k, v in sd.items():
        assert v.numpy().tobytes() == g["I0/" + k].tobytes(), (case, k)
    fs = [k for k in sd if k.startswith("fs_module.")]
    if fnp.config(g)["flags"]["use_fs"]:
        assert fs and all(k.split(".")[1].startswith(("fs1_", "fs2_")) for k in fs)
    assert [k for k in sd if k.startswith("fusion_module.")] == ["fusion_module.w_xy", "fusion_module.w_x.weight", "fusion_module.w_x.bias",
                                                                 "fusion_module.w_y.weight", "fusion_module.w_y.bias"]


def test_kernel_restatements_against_autograd():
    """finalmlp_np.gate_bwd / fusion_bwd (what the GPU tests hold the kernels to) against torch autograd in float64"""
    rng = np.random.default_rng(3)
    for N, C, D, G, H, rows in ((12, 3, 20, 8, 12, 1), (12, 3, 20, 8, 12, 4), (12, 3, 20, 8, 12, 12)):
        X = rng.standard_normal((N, D))
        st = [rng.standard_normal((rows, G)), rng.standard_normal((D, G)), rng.standard_normal(D), rng.standard_normal((H, D)), rng.standard_normal(H)]
        dA = rng.standard_normal((N, H))
        t = [torch.tensor(a, requires_grad=True) for a in [X] + st]
        idx = torch.from_numpy(fnp.gate_rows(rows, N, C))
        gate = 2 * torch.sigmoid(t[1] @ t[2].T + t[3])[idx]
        pre = (t[0] * gate) @ t[4].T + t[5]
        mask = (pre.detach() > 0).double().numpy() * 1.25
        (pre * torch.from_numpy(mask * dA)).sum().backward()
        g64, pre64 = fnp.gate_fwd(X, st, C)
        assert rel_err(g64, gate.detach().numpy()) < 1e-12 and rel_err(pre64, pre.detach().numpy()) < 1e-12
        for got, want in zip(fnp.gate_bwd(X, st, C, mask, dA), [p.grad.numpy() for p in t]):
            assert rel_err(got, want) < 1e-12
    for N, H1, H2, h in ((7, 12, 20, 4), (5, 8, 8, 1)):
        ar = [rng.standard_normal(s) for s in ((N, H1), (N, H2), (h * (H1 // h) * (H2 // h), 1), (1, H1), (1,), (1, H2), (1,))]
        dout = rng.standard_normal(N)
        t = [torch.tensor(a, requires_grad=True) for a in ar]
        xh, yh = t[0].view(N, h, -1), t[1].view(N, h, -1)
        out = (t[0] @ t[3].T).view(-1) + t[4] + (t[1] @ t[5].T).view(-1) + t[6] + torch.einsum('nhi,hij,nhj->n', xh, t[2].view(h, H1 // h, H2 // h), yh)
        (out * torch.from_numpy(dout)).sum().backward()
        assert rel_err(fnp.fusion_fwd(*ar, h), out.detach().numpy()) < 1e-12
        want = [t[0].grad, t[1].grad, t[2].grad, t[3].grad, t[4].grad, t[5].grad, t[6].grad]
        for got, w in zip(fnp.fusion_bwd(ar[0], ar[1], ar[2], ar[3], ar[5], dout, h), want):
            assert rel_err(np.asarray(got).reshape(-1), w.numpy().reshape(-1)) < 1e-12


def _construct(case="finalmlp_topk_d8_h4_ctx", corpus_edit=None, **flags):
    from models.context.FinalMLP import FinalMLPCTR, FinalMLPTopK
    g = load_golden(case)
    args, corpus = fnp.model_args(g, CPU, **flags)
    if corpus_edit:
        corpus_edit(corpus)
    return (FinalMLPCTR if fnp.config(g)["ctr"] else FinalMLPTopK)(args, corpus)


@pytest.mark.parametrize("flags,named", [
    (dict(mlp1_batch_norm=1), "--mlp1_batch_norm"),
    (dict(mlp2_batch_norm=1), "--mlp2_batch_norm"),
    (dict(mlp1_hidden_activations="Tanh"), "--mlp1_hidden_activations"),
    (dict(mlp2_hidden_activations="Dice"), "--mlp2_hidden_activations"),
    (dict(fs1_context="c_nosuch_c"), "--fs1_context"),
    (dict(fs2_context="i_category"), "--fs2_context"),
    (dict(fs2_context="user_id"), "--fs2_context"),
    (dict(num_heads=3), "num_heads"),
    (dict(emb_size=6), "emb_size"),
    (dict(mlp1_hidden_units="[260]"), "envelope"),
    (dict(mlp2_hidden_units="[16, 6]"), "envelope"),
    (dict(fs_hidden_units="[256]", mlp1_hidden_units="[256]"), "LDS"),
    (dict(mlp1_dropout=1.0), "dropout"),
])
def test_refusals_name_the_flag(flags, named):
    with pytest.raises(ValueError, match=named):
        _construct(**flags)


def test_refusals_of_the_corpus():
    def with_user(corpus):
        corpus.user_feature_names = ["u_age_c"]
        corpus.feature_max["u_age_c"] = 5

    def without_situation(corpus):
        corpus.situation_feature_names = []
    with pytest.raises(ValueError, match="u_"):
        _construct(corpus_edit=with_user)
    with pytest.raises(ValueError, match="c_"):
        _construct(corpus_edit=without_situation, fs1_context="")
    _construct()      # the golden's own flags construct


def test_check_shape_edges():
    from rechorus_amd import engine
    ok = dict(n_fields=8, emb_size=64, gate_in_1=64, first_1=64, gate_in_2=64, first_2=256, x_dim=64, y_dim=256, num_heads=1)
    engine.finalmlp_check_shape(**ok)      # the demo scripts' shape
    inside = [dict(n_fields=3), dict(n_fields=32), dict(emb_size=4, n_fields=3), dict(emb_size=128), dict(gate_in_1=4), dict(gate_in_2=256, first_2=4),
              dict(first_1=4), dict(first_1=256), dict(x_dim=4, y_dim=4), dict(x_dim=256, y_dim=256, num_heads=256), dict(num_heads=64),
              dict(drop_p_1=0.0, drop_p_2=0.999), dict(gate_in_1=192, first_1=192), dict(gate_in_1=256, first_1=192)]
    for edit in inside:
        engine.finalmlp_check_shape(**dict(ok, **edit))
    outside = [dict(n_fields=2), dict(n_fields=33), dict(emb_size=0), dict(emb_size=132), dict(emb_size=6), dict(gate_in_1=0), dict(gate_in_1=260),
               dict(gate_in_2=6), dict(first_1=0), dict(first_2=260), dict(first_2=10), dict(x_dim=0), dict(y_dim=260), dict(x_dim=6),
               dict(num_heads=0), dict(num_heads=3), dict(drop_p_1=1.0), dict(drop_p_2=-0.1), dict(gate_in_1=256, first_1=256),
               dict(gate_in_2=224, first_2=256)]
    for edit in outside:
        with pytest.raises(ValueError, match="FinalMLP on the HIP engine"):
            engine.finalmlp_check_shape(**dict(ok, **edit))
    engine.finalmlp_fusion_check_shape(64, 256, 1)
    with pytest.raises(ValueError, match="num_heads"):
        engine.finalmlp_fusion_check_shape(64, 256, 3)


def test_where_the_classes_live():
    import models.context.FinalMLP as re_export
    import models.finalmlp_model as bodies
    for name in ("FinalMLPBase", "FinalMLPCTR", "FinalMLPTopK"):
        assert getattr(re_export, name) is getattr(bodies, name)
        assert getattr(bodies, name).__module__ == "models.finalmlp_model"
    assert bodies.FinalMLPCTR.candidate_permutation_equivariant is True
    assert bodies.FinalMLPCTR.extra_log_args == ["emb_size", "loss_n", "use_fs"] == bodies.FinalMLPTopK.extra_log_args
    assert (bodies.FinalMLPCTR.reader, bodies.FinalMLPCTR.runner) == ("ContextReader", "CTRRunner")
    assert (bodies.FinalMLPTopK.reader, bodies.FinalMLPTopK.runner) == ("ContextReader", "BaseRunner")
    import argparse
    a, _ = bodies.FinalMLPCTR.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
    assert (a.emb_size, a.mlp1_hidden_units, a.mlp2_hidden_units, a.fs_hidden_units, a.use_fs, a.num_heads, a.loss_n) == \
        (64, '[64,64,64]', '[64,64,64]', '[64]', 1, 1, 'BCE')
    assert (a.mlp1_dropout, a.mlp2_batch_norm, a.fs1_context, a.fs2_context, a.mlp1_hidden_activations) == (0, 0, '', '', 'ReLU')
    b, _ = bodies.FinalMLPTopK.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
    assert b.loss_n == 'BPR'
