"""CPU: who takes NeuMF's one-kernel step.  The rule is written once -- engine.neumf_head_kernel_selected (the kernel is switched on
and has an instance) inside engine.neumf_fused_step_selected (plus what the step's table updates need: the bucket plan switched on,
a row-wise optimizer) -- and three places decide by it: the model file (through neumf_fused_step_selected), NeumfTrainer.step (which
adds what only the batch tells: the plan has a geometry for its id lists) and the sharded step's HipOps.neumf_head (the head alone:
it updates no table, so RC_TABLE_UPDATE is not its business).  Over a truth table of the switches and of what the library answers
(stubbed: rc_neumf_supported, rc_neumf_train_step_supported, rc_bucket_plan_supported) the three agree wherever they share a
question; NeumfTrainer.step is stubbed below the decision."""
import itertools

import pytest
import torch

from rechorus_amd import _lib, engine, sharded


class _Lib:
    def __init__(self, step_ok, plan_ok, three_kernel_ok=True):
        self.rc_neumf_train_step_supported = lambda Cn, d, l1: int(step_ok)
        self.rc_bucket_plan_supported = lambda n_a, n_b, range_a, range_b: int(plan_ok)
        self.rc_neumf_supported = lambda d, l1: int(three_kernel_ok)


D, L1, B = 32, 32, 6


def _trainer(monkeypatch, opt="SGD", rowwise=True):
    f = lambda *s: torch.zeros(s, dtype=torch.float32)
    P = {"mf_u": f(10, D), "mf_i": f(20, D), "mlp_u": f(10, D), "mlp_i": f(20, D), "W1": f(L1, 2 * D), "b1": f(L1), "w_out": f(D + L1)}
    tr = engine.NeumfTrainer(P, opt=opt, rowwise=rowwise)
    taken = []
    monkeypatch.setattr(tr, "_step_fused", lambda uid, iid, next_batch=None: taken.append("fused"))
    monkeypatch.setattr(tr, "_step_three_kernels", lambda uid, iid, use_plan: taken.append(("three", bool(use_plan))))
    return tr, taken


def _head(monkeypatch, Cn):
    monkeypatch.setattr(engine, "neumf_head_fwd_bwd", lambda *a, **k: ("loss_vec", "gu", "gi", "dense", None))
    P = {"W1": torch.zeros(L1, 2 * D), "b1": torch.zeros(L1), "w_out": torch.zeros(D + L1)}
    return sharded.HipOps().neumf_head(torch.zeros(B, 2 * D), torch.zeros(B * Cn, 2 * D), P, B, Cn, 1.0 / B)


@pytest.mark.parametrize("fused,use_plan,step_ok,plan_ok,Cn", list(itertools.product([True, False], [True, False], [True, False],
                                                                                    [True, False], [1, 3])))
def test_one_rule_three_readers(fused, use_plan, step_ok, plan_ok, Cn, monkeypatch):
    monkeypatch.setattr(engine, "_NEUMF_FUSED", fused)
    monkeypatch.setattr(engine, "_USE_PLAN", use_plan)
    monkeypatch.setattr(_lib, "load", lambda: _Lib(step_ok, plan_ok))
    kernel = fused and Cn >= 2 and step_ok               # the rule, written out
    selected = use_plan and kernel
    assert engine.neumf_head_kernel_selected(Cn, D, L1) is kernel
    assert engine.neumf_fused_step_selected(Cn, D, L1, "SGD") is selected
    # the trainer: the rule and the batch's plan geometry
    tr, taken = _trainer(monkeypatch)
    uid, iid = torch.zeros(B, dtype=torch.int64), torch.zeros((B, Cn), dtype=torch.int64)
    tr.step(uid, iid)
    assert taken == (["fused"] if (selected and plan_ok) else [("three", use_plan and plan_ok)])
    assert tr.step_count == 1
    # the sharded step's head
    head = _head(monkeypatch, Cn)
    assert (head is not None) is kernel
    if head is not None:
        assert head == ("loss_vec", "gu", "gi", "dense")
    # where the plan is switched on and has a geometry, all three say the same
    if use_plan and plan_ok:
        assert (taken == ["fused"]) is selected is (head is not None)


@pytest.mark.parametrize("opt,rowwise,want", [("SGD", True, True), ("Adam", True, True), ("Adagrad", True, True), ("Adam", False, False)])
def test_the_step_is_fused_for_every_rowwise_optimizer_and_never_in_dense_gradient_mode(opt, rowwise, want, monkeypatch):
    monkeypatch.setattr(engine, "_NEUMF_FUSED", True)
    monkeypatch.setattr(engine, "_USE_PLAN", True)
    monkeypatch.setattr(_lib, "load", lambda: _Lib(True, True))
    assert engine.neumf_fused_step_selected(3, D, L1, opt) is True
    assert engine.neumf_fused_step_selected(3, D, L1, "Adadelta") is False       # no row-wise Adadelta
    tr, taken = _trainer(monkeypatch, opt, rowwise)
    tr.step(torch.zeros(B, dtype=torch.int64), torch.zeros((B, 3), dtype=torch.int64))
    assert taken == (["fused"] if want else [("three", False)])


def test_a_tower_of_the_one_kernel_step_only_says_why_it_cannot_run(monkeypatch):
    """hidden 16 exists inside rc_neumf_train_step only: where the step is not selected, NeumfTrainer.step raises with the reason
    instead of failing inside rc_neumf_fwd"""
    monkeypatch.setattr(engine, "_NEUMF_FUSED", False)
    monkeypatch.setattr(engine, "_USE_PLAN", True)
    monkeypatch.setattr(_lib, "load", lambda: _Lib(True, True, three_kernel_ok=False))
    tr, taken = _trainer(monkeypatch)
    with pytest.raises(RuntimeError, match="RC_NEUMF_FUSED=0"):
        tr.step(torch.zeros(B, dtype=torch.int64), torch.zeros((B, 3), dtype=torch.int64))
    assert taken == []


def test_trainers_have_every_attribute_from_the_start():
    """what tests and tools read exists before the first step (None / empty until a step fills it)"""
    f = lambda *s: torch.zeros(s, dtype=torch.float32)
    tr = engine.NeumfTrainer({"mf_u": f(4, D), "mf_i": f(4, D), "mlp_u": f(4, D), "mlp_i": f(4, D), "W1": f(L1, 2 * D), "b1": f(L1),
                              "w_out": f(D + L1)}, opt="Adam")
    assert tr._marks is None and tr._ahead is None and tr._side is None and tr._side2 is None and tr.timing is None and tr.loss is None
    assert tr._fused_out == (None, None) and tr.step_count == 0 and set(tr.state["mf_i"]) == {"m", "v"}
    st = engine.SasrecTrainer({"item_emb": f(4, D), "pos_emb": f(3, D), "layers": []}, 2, opt="Adagrad")
    assert st._rows_by == {} and st._graphs == {} and st._graph_seen == {} and st._side is None and st._step_dev is None
    assert st.timing is None and st.loss is None and st.step_count == 0 and st.state == {}
    assert set(st._st(st.P["pos_emb"])) == {"m"} and st._st(st.P["pos_emb"]) is st._st(st.P["pos_emb"])
