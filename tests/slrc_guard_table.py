"""SLRC+'s rows of the guard-band coverage table: which rc_slrc_* entry points run between guard bands
(tests/test_gpu_slrc_guard_bands.py) and which do not, with the reason.  Same shape as tests/guard_table.py, which holds every
`int rc_*(` prototype; the SLRC+ entry points are declared `enum rc_status rc_slrc_*(` / `size_t rc_slrc_*(` and are held to THIS
table by tests/test_slrc_guarded_cpu.py, as FPMC's are to tests/fpmc_guard_table.py.

Run-to-run determinism: csrc/slrc.hip has no floating-point atomic.  Its one atomic is the integer ticket that lists rows with more
than 32 occurrences (atomicAdd(a.n_long, 1u)); the list's order decides which workgroup sums which row, never the order of a sum,
and the list lives in the workspace, not in a result -- every result is compared bit for bit."""
from guard_table import _g

GUARDED = {
    "rc_slrc_scores": _g("slrc_scores", "case_slrc_front"),
    "rc_slrc_fwd_bwd": _g("slrc_fwd_bwd", "case_slrc_front", "case_slrc_trainer"),
    "rc_slrc_excitation_bwd": _g("slrc_excitation_grads", "case_slrc_front"),
    "rc_slrc_item_update": _g("slrc_item_update", "case_slrc_item_update", "case_slrc_trainer"),
    "rc_slrc_user_bias_update": _g("slrc_user_bias_update", "case_slrc_user_bias", "case_slrc_trainer"),
}

EXEMPT = {
    "rc_slrc_check_shape": "host logic: compares d, C and R with constants, launches nothing and touches no buffer",
    "rc_slrc_fwd_bwd_layout": "host logic: the dispatcher's choice for (d, C, R) as a number, launches nothing and touches no buffer",
    "rc_slrc_item_update_workspace_bytes": "host logic: a size; every rc_slrc_item_update case is served exactly this many bytes",
}
