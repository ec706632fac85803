"""CFKG's rows of the guard-band coverage table: which rc_cfkg_* entry points run between guard bands
(tests/test_gpu_cfkg_guard_bands.py) and which do not, with the reason.  Same shape as tests/guard_table.py, which holds every
`int rc_*(` prototype; the CFKG entry points are declared `enum rc_status rc_cfkg_*(` / `size_t rc_cfkg_*(` and are held to THIS
table by tests/test_cfkg_guarded_cpu.py, as SLRC+'s are to tests/slrc_guard_table.py.

Run-to-run determinism: csrc/cfkg.hip has no atomic of any kind; the relation gradient is summed in a fixed order (register
accumulators, a fixed butterfly per wave, waves in order through LDS, workgroup partials in workgroup order) -- every result is
compared bit for bit."""
from guard_table import _g

GUARDED = {
    "rc_cfkg_scores": _g("cfkg_scores", "case_cfkg_front"),
    "rc_cfkg_scores_bwd": _g("cfkg_scores_grads", "case_cfkg_front"),
    "rc_cfkg_fwd_bwd": _g("cfkg_fwd_bwd", "case_cfkg_front", "case_cfkg_trainer"),
}

EXEMPT = {
    "rc_cfkg_check_shape": "host logic: compares d, C and n_rel with constants, launches nothing and touches no buffer",
    "rc_cfkg_fwd_bwd_rows_per_block": "host logic: the launch geometry for d as a number, launches nothing and touches no buffer",
    "rc_cfkg_fwd_bwd_workspace_bytes": "host logic: a size; every rc_cfkg_fwd_bwd case is served exactly this many bytes",
}
