"""The shape envelope of every hand-written kernel (the rc_*_supported predicates of include/rechorus_hip.h) and the tests that run
it at its edges.

ENVELOPES maps each predicate to
  "edges": the edge shapes it is tested at -- the largest accepted value of the bounded dimension is found by scanning the
           predicate (tests/test_gpu_envelope_edges.py), never written down here, so the tests follow the code;
  "tests": the tests (<file under tests/>::<function>) that run those edges.  Where an existing test already runs a predicate's
           edges, the entry names it instead of duplicating it.
tests/test_envelopes_cpu.py fails when a predicate of the header has no entry here, or an entry names a test that does not exist.
The GPU tests take their shapes from the tuples below."""

# rc_bprmf_fused_supported(d, C): the register path, C <= 8192 / d
BPRMF_FUSED_D = (16, 32, 64, 128)
# rc_neumf_zhead_supported(C, d, l1): (B, C, d, l1); None = the largest accepted value, found by the scan
ZHEAD_SHAPES = ((3, None, None, None), (7, None, 1, 1), (5, 37, 1023, 1023), (2, None, 1023, 1))
# rc_seq_attention_supported(L, dk) at the largest L: (n_heads, d_k) with sequence lengths {1, L - 1, L, > L}
SEQ_ATTENTION_HEADS = ((1, None), (3, 1))
# rc_list_metrics_supported(n, max_pos, n_k) at the largest n and n_k: max_pos = n and max_pos = n / 2
LIST_METRICS_MAX_POS = ("n", "n/2")
# rc_sasrec_supported, core path: (d, n_heads) down to d_k = 1, at the most layers and the largest L of that path
SASREC_CORE_HEADS = ((64, 8), (64, 16), (64, 32), (64, 64), (32, 8), (32, 16), (32, 32))
# rc_small_row_sums_supported(n, n_rows, d) at the largest n, one id holding most of the positions
SMALL_ROW_SUMS_D = (32, 1)

ENVELOPES = {
    "rc_bprmf_fused_supported": {
        "edges": "C = max and max + 1 (generic fall-back) at d = 16, 32, 64, 128; ragged B, repeated ids",
        "tests": ["test_gpu_envelope_edges.py::test_bprmf_fused_at_the_largest_candidate_count"],
    },
    "rc_neumf_zhead_supported": {
        "edges": "C = max with d = l1 = max, d = l1 = 1, d = 1023 with l1 = 1; C = 37 at d = l1 = 1023; max + 1 refused in C, d, l1",
        "tests": ["test_gpu_envelope_edges.py::test_neumf_zhead_at_its_envelope"],
    },
    "rc_seq_attention_supported": {
        "edges": "L = max with d_k = max and d_k = 1, lengths {1, L - 1, L, > L}; max + 1 refused in L and d_k; the whole block-by-block "
                 "SASRec encoder (nn.sasrec_encode_layers) forward and backward at L = max",
        "tests": ["test_gpu_envelope_edges.py::test_seq_attention_at_the_longest_history",
                  "test_gpu_envelope_edges.py::test_sasrec_encode_layers_at_the_longest_history"],
    },
    "rc_list_metrics_supported": {
        "edges": "n = max with max_pos = n and n / 2, the largest number of k values; max + 1 refused in n, max_pos, n_k",
        "tests": ["test_gpu_envelope_edges.py::test_list_metrics_at_the_widest_list"],
    },
    "rc_tower_tail_supported": {
        "edges": "every accepted (K, N2) pair at a ragged M; K = max + 1 and N2 = max + 1 refused",
        "tests": ["test_gpu_envelope_edges.py::test_tower_tail_every_accepted_pair"],
    },
    "rc_small_row_sums_supported": {
        "edges": "n = max with one hot id (most positions), d = 32 and 1; n = max + 1 refused",
        "tests": ["test_gpu_envelope_edges.py::test_small_row_sums_at_the_longest_list_with_a_hot_row"],
    },
    "rc_neumf_train_step_supported": {
        "edges": "C at the LDS bound of every (d, l1) the fused step has a kernel for, ragged B, hot ids, SGD / Adam / Adagrad; "
                 "max + 1 refused",
        "tests": ["test_gpu_envelope_edges.py::test_neumf_fused_step_at_the_lds_bound"],
    },
    "rc_neumf_supported": {
        "edges": "every (d, l1) of the three-kernel head, (128, 128) refused",
        "tests": ["test_gpu_neumf.py::test_neumf_random_shapes_vs_oracle"],
    },
    "rc_sasrec_supported": {
        "edges": "core path: heads 8 / 16 / 32 / 64 at d = 64 and 8 / 16 / 32 at d = 32 (d_k down to 1), the most layers, the largest L, "
                 "lengths {1, L - 1, L}, both encoders; buckets; long path: L in (64, 128], 1 layer, heads 1 / 2 / 4",
        "tests": ["test_gpu_envelope_edges.py::test_sasrec_core_encoders_at_the_most_heads_and_layers",
                  "test_gpu_sasrec.py::test_sasrec_length_buckets_vs_oracle",
                  "test_gpu_sasrec.py::test_sasrec_more_than_64_positions_vs_oracle",
                  "test_gpu_seq_layers.py::test_shapes_outside_every_kernel_are_refused_not_rerouted"],
    },
    "rc_rows_plan_supported": {
        "edges": "n_rows = 12,288 and the sorted-rows route it replaces",
        "tests": ["test_gpu_sasrec.py::test_rows_plan_equals_the_sorted_rows_route"],
    },
    "rc_bucket_plan_supported": {
        "edges": "the widest id ranges and list lengths one bucket level holds, and one past them",
        "tests": ["test_gpu_plan.py::test_bucket_plan_geometry_limits"],
    },
    "rc_full_catalogue_rank_supported": {
        "edges": "d = 32, 64, 128 against the oracle; NaN and exactly tied scores",
        "tests": ["test_gpu_sampler.py::test_full_catalogue_rank_vs_oracle",
                  "test_gpu_sampler.py::test_full_catalogue_and_target_rank_with_nan_and_exactly_tied_scores"],
    },
}
