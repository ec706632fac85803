"""The set attention block's rows of the guard-band coverage table: which rc_setmab_* entry points run between guard bands
(tests/test_gpu_setmab_guard_bands.py) and which do not, with the reason.  Same shape as tests/guard_table.py, which holds every
`int rc_*(` prototype; the set-attention entry points are declared `enum rc_status rc_setmab_*(` / `size_t rc_setmab_*(` and are held
to THIS table by tests/test_setmab_guarded_cpu.py, as the list encoder's are to tests/listenc_guard_table.py.

Run-to-run determinism: csrc/setmab.hip has no atomic of any kind; every result is compared bit for bit."""
from guard_table import _g

GUARDED = {
    "rc_setmab_fwd": _g("setmab_fwd", "case_setmab_block", "case_setmab_stack_step", "case_setmab_model_step"),
    "rc_setmab_bwd": _g("setmab_bwd", "case_setmab_block", "case_setmab_stack_step", "case_setmab_model_step"),
}

EXEMPT = {
    "rc_setmab_check_shape": "host logic: compares nq, nk, d, heads and d_ff with constants and an LDS byte count, launches nothing",
    "rc_setmab_bwd_workspace_bytes": "host logic: a size; every rc_setmab_bwd case is served exactly this many bytes",
}
