"""The list encoder's rows of the guard-band coverage table: which rc_listenc_* entry points run between guard bands
(tests/test_gpu_listenc_guard_bands.py) and which do not, with the reason.  Same shape as tests/guard_table.py, which holds every
`int rc_*(` prototype; the list-encoder entry points are declared `enum rc_status rc_listenc_*(` / `size_t rc_listenc_*(` and are
held to THIS table by tests/test_listenc_guarded_cpu.py, as DCNv2's are to tests/dcnv2_guard_table.py.

Run-to-run determinism: csrc/listenc.hip has no atomic of any kind; every result is compared bit for bit."""
from guard_table import _g

GUARDED = {
    "rc_listenc_block_fwd": _g("listenc_block_fwd", "case_listenc_block", "case_listenc_stack_step", "case_listenc_model_step"),
    "rc_listenc_block_bwd": _g("listenc_block_bwd", "case_listenc_block", "case_listenc_stack_step", "case_listenc_model_step"),
}

EXEMPT = {
    "rc_listenc_check_shape": "host logic: compares n, d, heads and d_ff with constants and an LDS byte count, launches nothing",
    "rc_listenc_block_bwd_workspace_bytes": "host logic: a size; every rc_listenc_block_bwd case is served exactly this many bytes",
}
