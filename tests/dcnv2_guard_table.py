"""DCNv2's rows of the guard-band coverage table: which rc_dcnv2_* entry points run between guard bands
(tests/test_gpu_dcnv2_guard_bands.py) and which do not, with the reason.  Same shape as tests/guard_table.py, which holds every
`int rc_*(` prototype; the DCNv2 entry points are declared `enum rc_status rc_dcnv2_*(` / `size_t rc_dcnv2_*(` and are held to THIS
table by tests/test_dcnv2_guarded_cpu.py, as Chorus's are to tests/chorus_guard_table.py.

Run-to-run determinism: csrc/dcnv2.hip has no atomic of any kind; every result is compared bit for bit."""
from guard_table import _g

GUARDED = {
    "rc_dcnv2_mix_layer_fwd": _g("dcnv2_mix_layer_fwd", "case_dcnv2_layer", "case_dcnv2_model_step"),
    "rc_dcnv2_mix_layer_bwd": _g("dcnv2_mix_layer_bwd", "case_dcnv2_layer", "case_dcnv2_model_step"),
}

EXEMPT = {
    "rc_dcnv2_check_shape": "host logic: compares D, low_rank and expert_num with constants, launches nothing and touches no buffer",
    "rc_dcnv2_mix_layer_bwd_workspace_bytes": "host logic: a size; every rc_dcnv2_mix_layer_bwd case is served exactly this many bytes",
}
