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
