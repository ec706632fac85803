"""FPMC's rows of the guard-band coverage table: which rc_fpmc_* entry points run between guard bands
(tests/test_gpu_fpmc_guard_bands.py) and which do not, with the reason.  Same shape as tests/guard_table.py, which holds every
`int rc_*(` prototype; the FPMC entry points are declared `enum rc_status rc_fpmc_*(` / `size_t rc_fpmc_*(` and are held to THIS
table by tests/test_fpmc_guarded_cpu.py.  Folding these rows into tests/guard_table.py is a maintenance follow-up.

Run-to-run determinism: csrc/fpmc.hip has no floating-point atomic.  Its one atomic is the integer ticket that lists rows with more
than 32 occurrences (atomicAdd(a.n_long, 1u)); the list's order decides which workgroup sums which row, never the order of a sum,
and the list lives in the workspace, not in a result -- every result is compared bit for bit."""
from guard_table import _g

GUARDED = {
    "rc_fpmc_scores": _g("fpmc_scores", "case_fpmc_front"),
    "rc_fpmc_fwd_bwd": _g("fpmc_fwd_bwd", "case_fpmc_front", "case_fpmc_trainer"),
    "rc_fpmc_item_update": _g("fpmc_item_update", "case_fpmc_item_update", "case_fpmc_trainer"),
}

EXEMPT = {
    "rc_fpmc_check_shape": "host logic: compares d and C with constants, launches nothing and touches no buffer",
    "rc_fpmc_fwd_bwd_layout": "host logic: the dispatcher's choice for (d, C) as a number, launches nothing and touches no buffer",
    "rc_fpmc_item_update_workspace_bytes": "host logic: a size; every rc_fpmc_item_update case is served exactly this many bytes",
}
