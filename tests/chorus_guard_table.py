"""Chorus's rows of the guard-band coverage table: which rc_chorus_* entry points run between guard bands
(tests/test_gpu_chorus_guard_bands.py) and which do not, with the reason.  Same shape as tests/guard_table.py, which holds every
`int rc_*(` prototype; the Chorus entry points are declared `enum rc_status rc_chorus_*(` / `size_t rc_chorus_*(` and are held to THIS
table by tests/test_chorus_guarded_cpu.py, as SLRC+'s are to tests/slrc_guard_table.py.

Run-to-run determinism: csrc/chorus.hip has no atomic of any kind; every result is compared bit for bit."""
from guard_table import _g

GUARDED = {
    "rc_chorus_scores": _g("chorus_scores", "case_chorus_front"),
    "rc_chorus_fwd_bwd": _g("chorus_fwd_bwd", "case_chorus_front", "case_chorus_trainer"),
    "rc_chorus_scores_bwd": _g("chorus_scores_grads", "case_chorus_front"),
    "rc_chorus_category_update": _g("chorus_category_update", "case_chorus_category_update", "case_chorus_trainer"),
}

EXEMPT = {
    "rc_chorus_check_shape": "host logic: compares d, C and R with constants, launches nothing and touches no buffer",
    "rc_chorus_front_tuples_per_block": "host logic: a constant of the launch geometry, launches nothing and touches no buffer",
    "rc_chorus_category_piece": "host logic: the piece size as a number, launches nothing and touches no buffer",
    "rc_chorus_front_workspace_bytes": "host logic: a size; every rc_chorus_fwd_bwd / rc_chorus_scores_bwd case is served exactly this many bytes",
    "rc_chorus_category_update_workspace_bytes": "host logic: a size; every rc_chorus_category_update case is served exactly this many bytes",
}
