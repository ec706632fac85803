"""CPU: the C-ABI library builds, loads, and exports every symbol include/rechorus_hip.h
declares; argument validation works without a GPU (no kernels are launched here)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from rechorus_amd import _lib

HEADER = os.path.join(ROOT, "include", "rechorus_hip.h")


def header_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from rechorus_amd.csrc.build import build
        build(verbose=False)
    return _lib.load()


def test_header_declares_the_expected_surface():
    syms = header_symbols()
    for must in ("rc_gather_dot_fwd", "rc_bpr_loss_fwd_bwd", "rc_bprmf_fwd_bwd", "rc_sort_ids",
                 "rc_segmented_update", "rc_dense_update", "rc_bprmf_train_step"):
        assert must in syms


def test_library_exports_every_declared_symbol(lib):
    for name in header_symbols():
        assert hasattr(lib, name), f"{name} declared in rechorus_hip.h but not exported"


def test_python_binding_covers_every_declared_symbol():
    assert sorted(_lib.SIGNATURES) == header_symbols()


def test_version_and_error_reporting(lib):
    assert lib.rc_version() == 1
    rc = lib.rc_gather_rows(None, 64, None, 4, None, None)
    assert rc == -1  # RC_ERR_INVALID_ARG
    assert b"null pointer" in lib.rc_last_error_string()
    with pytest.raises(_lib.RechorusHipError):
        _lib.call("rc_bpr_loss_fwd_bwd", C.c_void_p(8), 4, 1, 0.25, C.c_void_p(8), None, None)
    assert b"C >= 2" in lib.rc_last_error_string()


def test_folded_entry_points_reject_meaningless_argument_combinations(lib):
    """rc_plan_update_pair and rc_bprmf_fwd_bwd_update express what used to be separate entry points as argument combinations; the
    combinations that mean nothing are RC_ERR_INVALID_ARG with a message, before anything is launched.  (The arguments are chosen so
    that a missing check could not launch either: an empty occurrence list, a null table.)"""
    p = C.c_void_p(64)      # non-null and 16-byte aligned; never dereferenced
    h = C.byref(_lib.OptHyper(opt=_lib.RC_OPT_SGD, lr=0.1))
    d = 32

    def pair(src_b, src_ld):
        return lib.rc_plan_update_pair(p, None, None, p, None, None, d, p, p, p, 0, p, src_b, src_ld, 0, h, None, p, 1 << 20, None)
    # two contiguous sources take no row stride; a block source needs one: a multiple of 4 floats, at least 2 d
    for src_b, src_ld in ((p, 2 * d), (p, 4), (None, 0), (None, 2 * d - 4), (None, 2 * d + 2), (None, 2 * d + 1), (None, -4)):
        assert pair(src_b, src_ld) == -1, (src_b, src_ld)
        assert b"rc_plan_update_pair: src_ld" in lib.rc_last_error_string(), (src_b, src_ld)
    assert pair(p, 0) == 0 and pair(None, 2 * d) == 0 and pair(None, 2 * d + 4) == 0     # (n_occ = 0: accepted, nothing to do)

    def fused(single, multi):
        return lib.rc_bprmf_fwd_bwd_update(None, p, None, None, p, p, single, multi, 8, 4, d, 0.125, h, None, p, p, p, None)
    for single, multi in ((p, p), (None, None)):
        assert fused(single, multi) == -1
        assert b"exactly one of single / multi" in lib.rc_last_error_string()
    for single, multi in ((p, None), (None, p)):      # a valid pair gets as far as the next check (U is null)
        assert fused(single, multi) == -1
        assert b"null pointer" in lib.rc_last_error_string()


def test_segmented_update_entry_points_refuse_bad_arguments(lib):
    """The four segmented-update entry points share their SegArgs setup; each keeps its own argument checks.  Every refusal carries
    the entry point's name, and everything that inspects only the arguments comes before the workspace-size check: ws_bytes = 0 in
    every case, so a lost check ends in RC_ERR_WORKSPACE instead of a launch on the made-up pointers below."""
    p, q = C.c_void_p(64), C.c_void_p(68)      # never dereferenced; q is not 16-byte aligned
    n_occ, d, n_rows = 100, 64, 10

    def hyper(opt):
        return C.byref(_lib.OptHyper(opt=opt, lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, step=1))
    sgd, adam, adagrad, adadelta = (hyper(o) for o in (_lib.RC_OPT_SGD, _lib.RC_OPT_ADAM, _lib.RC_OPT_ADAGRAD, _lib.RC_OPT_ADADELTA))

    def seg(W=p, m=None, v=None, h=sgd, dense_grad=None, heads=None, n_heads=None, src2=None, n_split=n_occ):
        return lib.rc_segmented_update(W, m, v, d, p, p, n_occ, None, p, None, 1, src2, n_split, 0, 0, h, dense_grad, heads, n_heads, 0,
                                       p, 0, None)

    def rows(W=p, m=None, v=None, h=sgd, d=d):
        return lib.rc_segmented_update_rows(W, m, v, d, n_rows, p, p, n_occ, None, p, None, 1, None, n_occ, h, None, None, p, 0, None)

    def plan(m=None, v=None, h=sgd, n_rows=n_rows):
        return lib.rc_rows_plan_update(p, m, v, d, n_rows, n_occ, None, p, None, 1, None, n_occ, h, None, None, p, 0, None)

    def pair(h=sgd, d=32, dense_grad_a=None):
        return lib.rc_segmented_update_pair(p, None, None, p, None, None, d, p, p, n_occ, p, p, h, dense_grad_a, None, None, None,
                                            p, 0, None)
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    table = [
        ("rc_segmented_update", lambda: seg(W=None), INVALID, b"no output"),
        ("rc_segmented_update", lambda: seg(heads=p), INVALID, b"go together"),
        ("rc_segmented_update", lambda: seg(src2=p, n_split=n_occ + 1), INVALID, b"n_split"),
        ("rc_segmented_update", lambda: seg(h=adam), INVALID, b"Adam"),
        ("rc_segmented_update", lambda: seg(h=adagrad), INVALID, b"Adagrad"),
        ("rc_segmented_update", lambda: seg(h=adadelta), INVALID, b"dense steps only"),
        ("rc_segmented_update_rows", lambda: rows(W=q), INVALID, b"16-byte aligned"),
        ("rc_segmented_update_rows", lambda: rows(d=48), UNSUPPORTED, b""),
        ("rc_segmented_update_rows", lambda: rows(h=adam), INVALID, b""),
        ("rc_rows_plan_update", lambda: plan(n_rows=20000), UNSUPPORTED, b""),
        ("rc_rows_plan_update", lambda: plan(h=adam), INVALID, b""),
        ("rc_segmented_update_pair", lambda: pair(dense_grad_a=p), INVALID, b"both dense gradients or none"),
        ("rc_segmented_update_pair", lambda: pair(d=24), UNSUPPORTED, b""),
        ("rc_segmented_update_pair", lambda: pair(h=adam), INVALID, b""),
        ("rc_segmented_update", seg, WORKSPACE, b"workspace 0 <"),
        ("rc_segmented_update_rows", rows, WORKSPACE, b"workspace 0 <"),
        ("rc_rows_plan_update", plan, WORKSPACE, b"workspace 0 <"),
        ("rc_segmented_update_pair", pair, WORKSPACE, b"workspace 0 <"),
    ]
    for i, (name, call, code, text) in enumerate(table):
        got = call()
        msg = lib.rc_last_error_string()
        assert got == code, (i, name, got, msg)
        assert msg.startswith(name.encode() + b":") and text in msg, (i, name, msg)


def test_bprmf_train_step_refuses_bad_arguments_before_the_workspace_check(lib):
    """rc_bprmf_train_step / _ahead: everything that inspects only the arguments -- null pointers, shape, distinct tables, the
    optimizer and its state tensors -- is refused in the entry point, before the workspace-size check and so before anything is
    enqueued (the optimizer used to be validated inside the launch sequences, behind the first kernel).  ws_bytes = 0 in every
    case: a lost check ends in RC_ERR_WORKSPACE instead of a launch on the made-up pointers below.  Both entry points report as
    rc_bprmf_train_step; only the ticket messages carry _ahead."""
    p, r = C.c_void_p(64), C.c_void_p(128)      # non-null, 16-byte aligned, distinct; never dereferenced
    B, Cn, d = 8, 4, 32

    def hyper(opt, step=1):
        return C.byref(_lib.OptHyper(opt=opt, lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, step=step))
    sgd, adam, adagrad, adadelta = (hyper(o) for o in (_lib.RC_OPT_SGD, _lib.RC_OPT_ADAM, _lib.RC_OPT_ADAGRAD, _lib.RC_OPT_ADADELTA))
    ticket = _lib.StepTicket()

    def plain(U=p, I=r, m=None, v=None, h=sgd, C_=Cn):
        return lib.rc_bprmf_train_step(U, I, m, v, m, v, p, p, B, C_, d, 100, 1000, h, 1.0 / B, p, None, p, 0, None, None)

    def ahead(U=p, I=r, m=None, v=None, h=sgd, C_=Cn, t=C.byref(ticket)):
        return lib.rc_bprmf_train_step_ahead(U, I, m, v, m, v, p, p, 0, None, None, 0, t, B, C_, d, 100, 1000, h, 1.0 / B, p, None,
                                             p, 0, None, None)
    INVALID, WORKSPACE = -1, -2
    table = []
    for call in (plain, ahead):
        table += [
            (lambda call=call: call(h=adam), INVALID, b"Adam needs m and v"),
            (lambda call=call: call(h=adam, m=p), INVALID, b"Adam needs m and v"),
            (lambda call=call: call(h=adagrad), INVALID, b"Adagrad needs m"),
            (lambda call=call: call(h=adadelta, m=p, v=p), INVALID, b"dense steps only"),
            (lambda call=call: call(h=hyper(_lib.RC_OPT_ADAM, step=0), m=p, v=p), INVALID, b"step >= 1"),
            (lambda call=call: call(I=p), INVALID, b"distinct"),
            (lambda call=call: call(C_=1), INVALID, b""),
            (lambda call=call: call(h=None), INVALID, b""),
            (call, WORKSPACE, b"workspace 0 <"),
            (lambda call=call: call(h=adam, m=p, v=p), WORKSPACE, b"workspace 0 <"),
            (lambda call=call: call(h=adagrad, m=p), WORKSPACE, b"workspace 0 <"),
        ]
    table.append((lambda: ahead(t=None), INVALID, b"ticket missing"))
    for i, (call, code, text) in enumerate(table):
        got = call()
        msg = lib.rc_last_error_string()
        assert got == code, (i, got, msg)
        assert msg.startswith(b"rc_bprmf_train_step") and text in msg, (i, msg)
    assert ticket.generation == 0


def test_step_and_small_plan_workspace_sizes(lib):
    """The byte counts callers allocate by (the small plan's layout is carved in one place; these are the sizes of the layout as it
    was when five copies of it agreed)."""
    for (B, Cn, d), want in (((8, 4, 32), 8495616), ((3, 5, 32), 8494080), ((256, 100, 64), 66634752), ((300, 100, 64), 78087680),
                             ((2048, 100, 64), 30142976), ((65536, 100, 64), 701639168), ((500, 4, 128), 9052672)):
        assert lib.rc_bprmf_step_workspace_bytes(B, Cn, d) == want, (B, Cn, d)
    for n, want in ((1, 4608), (1000, 2562048), (8192, 20973568), (32768, 83888128), (32769, 83890688)):
        assert lib.rc_small_row_sums_workspace_bytes(n) == want, n
    assert lib.rc_small_row_sums_workspace_bytes(0) == 4608      # n < 1 is sized as n = 1


def test_context_model_entry_points_refuse_bad_arguments(lib):
    """The context-model path has one entry point per launch sequence; an argument subset is a NULL or a zero.  The refusals that
    guard a kernel precondition carry the surviving entry point's name.  Nothing can launch on the made-up pointers below: field 1
    of every gather has a null table, ws_bytes = 0 in every row-sums and sort call, and the CTR head gets a null bias."""
    p = C.c_void_p(64)      # non-null and 16-byte aligned; never dereferenced
    INVALID, WORKSPACE = -1, -2
    ptrs = lambda *v: (C.c_void_p * len(v))(*v)
    ints = lambda *v: (C.c_int * len(v))(*v)
    tabs, tabs1, ids, per_row, offs = ptrs(64, None), ptrs(64, 64), ptrs(64, 64), ints(0, 0), (C.c_int64 * 2)(0, 10)

    def gather(tables1=None, out1=None, kind=None, row_flags=None, step_dev=None, F=2, fused=None):
        args = [tabs, tables1, ids, per_row, kind, -1, offs, F, 4, 1, 16, p, out1, None, row_flags, step_dev, 1]
        if fused is None:
            return lib.rc_gather_fields(*args, None)
        return lib.rc_gather_fields_fused(*args, *fused, None)      # fused = (fm_out, fm_sum, plan_ws, plan_ws_bytes, bump)

    num = (ptrs(64), ints(1), ints(1), ints(0))     # values, per_row, kind (RC_FIELD_F32), field of ONE numeric field
    no_num = (None, None, None, None)
    n, F, B = 96, 3, 32

    def sums(src1=None, out1=None, arrays=no_num, n_numeric=0, F=F, B=B, d=16, dW=None, dw1=None):
        return lib.rc_small_row_sums(p, n, 10, p, d, p, src1, out1, *arrays, n_numeric, F, B, 1, dW, dw1, p, 0, None)

    def planned(src1=None, out1=None, d=16, fm=(None, None, None), F=0, B=0):
        return lib.rc_small_row_sums_planned(n, 10, p, d, p, src1, out1, *no_num, 0, F, B, 1, None, None, *fm, p, 0, None)

    def head(n=100, g_lin=None, g_bias=None):
        return lib.rc_ctr_head_fwd_bwd_sums(None, p, 3, None, None, p, n, p, p, p, p, g_lin, g_bias, None, None)

    def sort(ids_b=None, n_b=0, key_offset_b=0, key_range=10):
        return lib.rc_sort_ids(p, 100, ids_b, n_b, key_offset_b, key_range, p, p, p, 0, None)
    one = ptrs(64)
    table = [
        ("rc_gather_fields", gather, INVALID, b"null table / ids for field 1"),                     # (what stops every valid case below)
        ("rc_gather_fields", lambda: gather(tables1=tabs1), INVALID, b"come together"),
        ("rc_gather_fields", lambda: gather(out1=p), INVALID, b"come together"),
        ("rc_gather_fields", lambda: gather(row_flags=p), INVALID, b"row flags"),
        ("rc_gather_fields", lambda: gather(kind=ints(7, 0)), INVALID, b"kind[0] = 7"),
        ("rc_gather_fields", lambda: gather(F=0), INVALID, b"F must be in [1, 48]"),
        ("rc_gather_fields", lambda: gather(F=49), INVALID, b"F must be in [1, 48]"),
        ("rc_gather_fields_fused", lambda: gather(fused=(None, None, None, 0, None)), INVALID, b"neither"),
        ("rc_gather_fields_fused", lambda: gather(fused=(p, None, None, 0, None)), INVALID, b"come together"),
        ("rc_gather_fields_fused", lambda: gather(row_flags=p, step_dev=p, fused=(p, p, None, 0, p)), INVALID, b"cannot be the counter"),
        ("rc_gather_fields_fused", lambda: gather(tables1=tabs1, out1=p, fused=(p, p, None, 0, None)), INVALID, b"null table / ids for field 1"),
        ("rc_small_row_sums", sums, WORKSPACE, b"workspace 0 <"),
        ("rc_small_row_sums", lambda: sums(src1=p, out1=p), WORKSPACE, b"workspace 0 <"),
        ("rc_small_row_sums", lambda: sums(src1=p), INVALID, b"src1 / out1 together"),
        ("rc_small_row_sums", lambda: sums(src1=p, out1=p, n_numeric=1), INVALID, b"null pointer (numeric fields)"),
        ("rc_small_row_sums", lambda: sums(arrays=num, n_numeric=1, dW=one, dw1=one), INVALID, b"null pointer (numeric fields)"),
        ("rc_small_row_sums", lambda: sums(src1=p, out1=p, arrays=num, n_numeric=5, F=8, B=12, dW=one, dw1=one), INVALID, b"5 numeric fields"),
        ("rc_small_row_sums", lambda: sums(src1=p, out1=p, arrays=num, n_numeric=1, B=B - 1, dW=one, dw1=one), INVALID, b"bad shape"),
        ("rc_small_row_sums", lambda: sums(arrays=num, n_numeric=1, d=4, dW=one, dw1=one), INVALID, b"bad shape"),
        ("rc_small_row_sums", lambda: sums(src1=p, out1=p, arrays=num, n_numeric=1, dW=one, dw1=one), WORKSPACE, b"workspace 0 <"),
        ("rc_small_row_sums_planned", lambda: planned(d=4), WORKSPACE, b"workspace 0 <"),         # another source on the same grouping, any width
        ("rc_small_row_sums_planned", lambda: planned(src1=p, out1=p, fm=(p, p, None), F=F, B=B), INVALID, b"come together"),
        ("rc_small_row_sums_planned", lambda: planned(d=4, fm=(p, p, p), F=F, B=B), INVALID, b"bad shape"),
        ("rc_small_row_sums_planned", lambda: planned(src1=p, out1=p, fm=(p, p, p), F=F, B=B), WORKSPACE, b"workspace 0 <"),
        ("rc_ctr_head_fwd_bwd_sums", head, INVALID, b"null pointer"),
        ("rc_ctr_head_fwd_bwd_sums", lambda: head(g_lin=p), INVALID, b"g_lin and g_bias come together"),
        ("rc_ctr_head_fwd_bwd_sums", lambda: head(n=65537), INVALID, b"n=65537"),
        ("rc_sort_ids", sort, WORKSPACE, b"workspace 0 <"),
        ("rc_sort_ids", lambda: sort(n_b=5), INVALID, b"null pointer"),
        ("rc_sort_ids", lambda: sort(ids_b=p, n_b=5, key_offset_b=10), INVALID, b"out of range"),
    ]
    for i, (name, call, code, text) in enumerate(table):
        got = call()
        msg = lib.rc_last_error_string()
        assert got == code, (i, name, got, msg)
        assert msg.startswith(name.encode() + b":") and text in msg, (i, name, msg)


def test_sasrec_shape_envelope(lib):
    """rc_sasrec_supported is host logic: d in {32, 64}, 1..4 blocks, heads | d, history_max <= 64 on every route; 65..128 with ONE
    block and 1 / 2 / 4 heads (the batch encoder's one-row path).  engine.sasrec_supported adds: no training-mode dropout there."""
    from rechorus_amd import engine
    ok = lambda *a: bool(lib.rc_sasrec_supported(*a))   # (d, n_layers, n_heads, L)
    assert ok(64, 1, 4, 50) and ok(32, 4, 2, 64) and ok(64, 2, 8, 20) and ok(64, 1, 1, 1)
    assert not ok(128, 1, 4, 50) and not ok(64, 5, 4, 50) and not ok(64, 1, 3, 50) and not ok(64, 1, 4, 0)
    assert ok(64, 1, 4, 65) and ok(64, 1, 1, 128) and ok(32, 1, 2, 100) and ok(32, 1, 4, 128)
    assert not ok(64, 2, 4, 65) and not ok(64, 1, 8, 100) and not ok(64, 1, 4, 129)
    assert engine.sasrec_supported(64, 1, 4, 100) and not engine.sasrec_supported(64, 1, 4, 100, dropout=0.1)
    assert engine.sasrec_supported(64, 2, 4, 64, dropout=0.5)


def test_opt_hyper_struct_layout():
    # struct rc_opt_hyper: 2 ints, 5 doubles, 1 int64 -> 56 bytes, natural alignment
    assert C.sizeof(_lib.OptHyper) == 56
    assert _lib.OptHyper.lr.offset == 8 and _lib.OptHyper.step.offset == 48


def test_engine_refuses_cpu_tensors():
    import torch
    from rechorus_amd import engine
    W = torch.zeros(4, 64)
    with pytest.raises(ValueError, match="GPU"):
        engine.gather_rows(W, torch.zeros(2, dtype=torch.int64))


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.RechorusHipMissing):
        _lib.load()


def test_integration_doc_names_every_entry_point():
    """INTEGRATION.md's table is the map from reference code to entry points: it has to mention all of them"""
    import re
    header = open(os.path.join(ROOT, "include", "rechorus_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = sorted(set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(", header)))
    missing = [n for n in names if n not in doc and not (n.endswith("_fwd") or n.endswith("_bwd")) ]
    # `rc_x_fwd/bwd` is written as one cell for pairs
    missing += [n for n in names if (n.endswith("_fwd") or n.endswith("_bwd")) and n not in doc and n[:-4] + "_fwd/bwd" not in doc]
    assert not missing, missing
