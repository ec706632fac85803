"""KDA's rows of the guard-band coverage table: which rc_kda_* entry points run between guard bands
(tests/test_gpu_kda_guard_bands.py) and which do not, with the reason.  Same shape as tests/guard_table.py, which holds every
`int rc_*(` prototype; the KDA entry points are declared `enum rc_status rc_kda_*(` / `size_t rc_kda_*(` and are held to THIS table
by tests/test_kda_guarded_cpu.py, as DIN's are to tests/din_guard_table.py.

Run-to-run determinism: csrc/kda.hip has no atomic of any kind; a workgroup of the backward owns whole batch rows, accumulates drel
and dfreq_* in its own slice of the workspace and the slices are summed in workgroup order -- every result is compared bit for bit."""
from guard_table import _g

GUARDED = {
    "rc_kda_aggregate_fwd": _g("kda_aggregate_fwd", "case_kda_aggregate"),
    "rc_kda_aggregate_bwd": _g("kda_aggregate_bwd", "case_kda_aggregate"),
}

EXEMPT = {
    "rc_kda_check_shape": "host logic: compares V, L, R and F with constants, launches nothing and touches no device buffer",
    "rc_kda_aggregate_bwd_workspace_bytes": "host logic: a size; every rc_kda_aggregate_bwd case is served exactly this many bytes",
}
