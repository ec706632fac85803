"""DIN's rows of the guard-band coverage table: which rc_din_* entry points run between guard bands
(tests/test_gpu_din_guard_bands.py) and which do not, with the reason.  Same shape as tests/guard_table.py, which holds every
`int rc_*(` prototype; the DIN entry points are declared `enum rc_status rc_din_*(` / `size_t rc_din_*(` and are held to THIS table
by tests/test_din_guarded_cpu.py, as CFKG's are to tests/cfkg_guard_table.py.

Run-to-run determinism: csrc/din.hip has no atomic of any kind; a workgroup of the backward owns whole batch rows, accumulates the
parameter gradients in its own slice of the workspace and the slices are summed in workgroup order -- every result is compared bit
for bit."""
from guard_table import _g

GUARDED = {
    "rc_din_attention_fwd": _g("din_attention_fwd", "case_din_attention"),
    "rc_din_attention_bwd": _g("din_attention_bwd", "case_din_attention"),
}

EXEMPT = {
    "rc_din_check_shape": "host logic: compares H, L, the widths and drop_p with constants, launches nothing and touches no device buffer",
    "rc_din_param_count": "host logic: a count from H and the widths, launches nothing and touches no device buffer",
    "rc_din_attention_bwd_workspace_bytes": "host logic: a size; every rc_din_attention_bwd case is served exactly this many bytes",
}
