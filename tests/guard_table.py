"""Which C entry points run between guard bands (tests/test_gpu_guard_bands.py) and which do not, with the reason.

GUARDED: entry point -> {"wrapper": dotted name in rechorus_amd.engine that marshals it, "cases": the case functions of
tests/test_gpu_guard_bands.py that reach it, "deterministic": False where two runs may differ (with the line of the atomic)}.
EXEMPT: entry point -> one line a reviewer can check in the code.  tests/test_guarded_cpu.py holds the two dicts to the header:
every `int rc_*(` prototype is in exactly one of them.

Run-to-run determinism was established by reading csrc/ for atomics: there is no floating-point atomic anywhere (every atomicAdd /
atomicMin is on an integer counter, histogram cell or ticket).  Integer tickets do decide the ORDER in which three entry points list
their records; their values are compared through a canonical form instead of bit for bit (see `order` below)."""


def _g(wrapper, *cases, deterministic=True, order=None):
    e = {"wrapper": wrapper, "cases": list(cases), "deterministic": deterministic}
    if order:
        e["order"] = order
    return e


GUARDED = {
    # dense layers (csrc/mlp.hip, tower_tail.hip)
    "rc_linear_fwd": _g("linear_fwd", "case_linear", "case_neumf_zhead"),
    "rc_linear_bwd": _g("linear_bwd", "case_linear", "case_neumf_zhead"),
    "rc_tower_tail_fwd": _g("tower_tail_fwd", "case_tower_tail"),
    "rc_tower_tail_bwd": _g("tower_tail_bwd", "case_tower_tail"),
    # sequence layers (csrc/seq_layers.hip)
    "rc_seq_attention_fwd": _g("seq_attention_fwd", "case_seq_attention"),
    "rc_seq_attention_bwd": _g("seq_attention_bwd", "case_seq_attention"),
    "rc_seq_add_layernorm_fwd": _g("seq_add_layernorm_fwd", "case_seq_add_layernorm"),
    "rc_seq_add_layernorm_bwd": _g("seq_add_layernorm_bwd", "case_seq_add_layernorm"),
    "rc_seq_offsets": _g("seq_offsets", "case_seq_rest", "case_seq_attention"),
    "rc_seq_embed_fwd": _g("seq_embed", "case_seq_rest"),
    "rc_seq_pick_last_fwd": _g("seq_pick_last", "case_seq_rest"),
    "rc_seq_pick_last_bwd": _g("seq_pick_last_bwd", "case_seq_rest"),
    "rc_seq_pos_grad": _g("seq_pos_grad", "case_seq_rest"),
    "rc_seq_embed_fwdpos_fwd": _g("seq_embed_fwdpos", "case_seq_fwdpos"),
    "rc_seq_pos_grad_fwdpos": _g("seq_pos_grad_fwdpos", "case_seq_fwdpos"),
    # SASRec encoders (csrc/sasrec.hip, sasrec_batch.hip)
    "rc_sasrec_fwd": _g("sasrec_fwd", "case_sasrec"),
    "rc_sasrec_bwd": _g("sasrec_bwd", "case_sasrec"),
    "rc_sasrec_batch_fwd": _g("sasrec_fwd", "case_sasrec"),
    "rc_sasrec_batch_bwd": _g("sasrec_bwd", "case_sasrec"),
    "rc_sasrec_batch_bwd_part": _g("sasrec_bwd", "case_sasrec"),
    "rc_sasrec_pos_grad": _g("sasrec_pos_grad", "case_sasrec"),
    # BPRMF (csrc/gather.hip, loss.hip, bprmf_fused.hip)
    "rc_gather_rows": _g("gather_rows", "case_gather"),
    "rc_gather_rows_pair": _g("gather_rows_pair", "case_gather"),
    "rc_gather_dot_fwd": _g("gather_dot", "case_gather"),
    "rc_weighted_row_sum": _g("weighted_row_sum", "case_gather"),
    "rc_bpr_loss_fwd_bwd": _g("bpr_loss", "case_bpr_loss"),
    "rc_reduce_sum": _g("reduce_sum", "case_bpr_loss"),
    "rc_bprmf_fwd_bwd": _g("bprmf_fwd_bwd", "case_gather"),
    # sort / segments (csrc/sort_ids.hip, seg_update.hip)
    "rc_sort_ids": _g("sort_ids", "case_sort"),
    "rc_segment_heads": _g("segment_heads", "case_sort", deterministic=False,
                           order="heads are listed in ticket order: atomicAdd(n_heads, total), csrc/seg_update.hip:141"),
    "rc_segmented_update": _g("segmented_update", "case_segmented", "case_narrow_tiles"),
    "rc_segmented_update_pair": _g("segmented_update_pair", "case_segmented_pair"),
    "rc_segmented_update_rows": _g("segmented_update2", "case_segmented_rows"),
    "rc_rows_plan_build": _g("RowsPlan", "case_rows_plan"),
    "rc_rows_plan_update": _g("RowsPlan.update", "case_rows_plan"),
    "rc_rows_plan_views": _g("RowsPlan.views", "case_rows_plan"),
    # narrow tables / small route (csrc/small_step.hip)
    "rc_small_row_sums": _g("embedding_dense_backward", "case_small_row_sums", "case_small_pair"),
    "rc_small_row_sums_planned": _g("small_row_sums_planned", "case_small_row_sums", "case_small_pair", "case_gather_fields"),
    # plan-driven step (csrc/bucket_plan.hip, plan_update.hip, train_step.hip)
    "rc_bucket_plan": _g("bucket_plan", "case_bucket_plan", "case_plan_updates", deterministic=False,
                         order="row records are listed in ticket order: atomicAdd(n_rows_a / n_rows_b, ...), csrc/bucket_plan.hip:601, :819, :953"),
    "rc_bucket_multi_bitmap": _g("bucket_multi_bitmap", "case_bprmf_update"),
    "rc_plan_update": _g("Plan.update", "case_plan_updates"),
    "rc_plan_update_pair": _g("Plan.update_pair", "case_plan_updates"),
    "rc_plan_row_sums": _g("Plan.row_sums", "case_plan_updates"),
    "rc_plan_distinct": _g("Plan.distinct", "case_plan_updates", deterministic=False,
                           order="the distinct ids come in the plan's record order (see rc_bucket_plan)"),
    "rc_bprmf_fwd_bwd_update": _g("bprmf_fwd_bwd_update", "case_bprmf_update"),
    "rc_bprmf_train_step_ahead": _g("BprmfTrainer.step", "case_bprmf_trainer"),
    # dense optimizers (csrc/dense_opt.hip), BUIR's target update
    "rc_dense_update": _g("dense_update", "case_dense_update"),
    "rc_dense_update_multi": _g("dense_update_multi", "case_dense_update"),
    "rc_dense_update_rows_dev": _g("dense_update_rows", "case_dense_rows"),
    "rc_step_increment": _g("step_increment", "case_dense_rows", "case_dense_update"),
    "rc_step_increment2": _g("step_increment", "case_dense_rows"),
    "rc_buir_ema": _g("ema_update", "case_ema"),
    # NeuMF (csrc/neumf.hip, neumf_step.hip, neumf_zhead.hip)
    "rc_neumf_fwd": _g("neumf_fwd", "case_neumf"),
    "rc_neumf_bwd": _g("neumf_bwd", "case_neumf"),
    "rc_neumf_head_fwd_bwd": _g("neumf_head_fwd_bwd", "case_neumf_head"),
    "rc_neumf_zhead_fwd_bwd": _g("neumf_zhead", "case_neumf_zhead"),
    "rc_neumf_train_step": _g("neumf_train_step", "case_neumf_step", deterministic=False,
                              order="marks its rows itself when they are not prepared: the owner words as rc_neumf_mark_rows; every other output is compared bit for bit"),
    "rc_neumf_mark_rows": _g("neumf_mark_rows", "case_neumf_step", deterministic=False,
                             order="owner[id] keeps the position of whichever occurrence stored last (plain stores, csrc/neumf_step.hip:654); the flags do not depend on it"),
    "rc_neumf_unmark_rows": _g("neumf_mark_rows", "case_neumf_step"),
    # context models (csrc/fm_bce.hip)
    "rc_fm_second_order_fwd": _g("fm_second_order", "case_fm"),
    "rc_fm_second_order_bwd": _g("fm_second_order_bwd", "case_fm"),
    "rc_gather_fields": _g("gather_fields", "case_gather_fields"),
    "rc_gather_fields_fused": _g("gather_fields", "case_gather_fields"),
    "rc_numeric_field_grads": _g("numeric_field_grads", "case_gather_fields"),
    "rc_bce_prob_fwd_bwd": _g("bce_prob", "case_ctr_heads"),
    "rc_bce_ranking_fwd_bwd": _g("bce_ranking", "case_ctr_heads"),
    "rc_ctr_head_fwd_bwd": _g("ctr_head", "case_ctr_heads"),
    "rc_ctr_head_fwd_bwd_sums": _g("ctr_head_sums", "case_ctr_heads"),
    "rc_ctr_head_bwd": _g("ctr_head_bwd", "case_ctr_heads"),
    # list-wise (csrc/listwise_loss.hip, eval_rank.hip)
    "rc_list_loss_fwd_bwd": _g("list_loss", "case_list_losses"),
    "rc_softmax_ce_fwd_bwd": _g("softmax_ce", "case_list_losses"),
    "rc_list_bpr_fwd_bwd": _g("list_bpr", "case_list_losses"),
    "rc_list_metrics": _g("list_metrics", "case_list_metrics"),
    # evaluation / sampler (csrc/eval_rank.hip, sampler.hip)
    "rc_target_rank": _g("target_rank", "case_eval"),
    "rc_full_catalogue_rank": _g("full_catalogue_rank", "case_eval"),
    "rc_comirec_score_max": _g("comirec_score_max", "case_score_max"),
    "rc_buir_scores": _g("buir_scores", "case_buir"),
    "rc_buir_query": _g("buir_query", "case_buir"),
    "rc_sample_negatives": _g("sample_negatives", "case_sampler"),
    "rc_assemble_candidates": _g("assemble_candidates", "case_sampler"),
    "rc_gather_history": _g("gather_history", "case_sampler"),
    "rc_stage_batch": _g("SasrecTrainer.step", "case_stage_batch"),
    # LightGCN (csrc/lgcn.hip)
    "rc_lgcn_propagate_fwd": _g("lgcn_propagate_fwd", "case_lgcn"),
    "rc_lgcn_propagate_bwd": _g("lgcn_propagate_bwd", "case_lgcn"),
    # newer models
    "rc_directau_fwd": _g("directau_fwd", "case_directau"),
    "rc_directau_bwd": _g("directau_bwd", "case_directau"),
    "rc_buir_fwd": _g("buir_fwd", "case_buir"),
    "rc_buir_bwd": _g("buir_bwd", "case_buir"),
    "rc_comirec_fwd": _g("comirec_fwd", "case_comirec"),
    "rc_comirec_bwd": _g("comirec_bwd", "case_comirec"),
    "rc_autoint_layer_fwd": _g("autoint_layer_fwd", "case_autoint"),
    "rc_autoint_layer_bwd": _g("autoint_layer_bwd", "case_autoint"),
    "rc_finalmlp_gate_fwd": _g("finalmlp_gate_fwd", "case_finalmlp_gate"),
    "rc_finalmlp_gate_bwd": _g("finalmlp_gate_bwd", "case_finalmlp_gate"),
    "rc_finalmlp_fusion_fwd": _g("finalmlp_fusion_fwd", "case_finalmlp_fusion"),
    "rc_finalmlp_fusion_bwd": _g("finalmlp_fusion_bwd", "case_finalmlp_fusion"),
    "rc_contra_loss_fwd": _g("contra_loss_fwd", "case_contra"),
    "rc_contra_loss_bwd": _g("contra_loss_bwd", "case_contra"),
    # sharded routing on one device (csrc/owner_step.hip)
    "rc_route_by_owner": _g("route_by_owner", "case_route"),
    "rc_owner_unpack": _g("owner_unpack", "case_route"),
    "rc_owner_backward": _g("owner_backward", "case_owner_backward"),
}

_HOST = "pure host function: no kernel, no device memory"
EXEMPT = {
    "rc_bench_mix": "bench-only measurement aid (bench.py), not a step of any path",
    "rc_bench_mfma": "bench-only measurement aid (bench.py), not a step of any path",
    "rc_bprmf_train_step": "no engine wrapper calls it: BprmfTrainer.step goes through rc_bprmf_train_step_ahead, which the header states runs the same pipeline bit for bit and which is guarded without a next batch",
    "rc_bprmf_step_ahead_reset": "waits for the library's side stream and clears a host ticket; reached only after a look-ahead, which starts a side stream",
    "rc_sasrec_batch_bwd_splits": _HOST + " (a predicate of six scalars)",
    "rc_bprmf_step_pipeline": "host switch: sets a process-wide int that rc_bprmf_train_step reads (case_bprmf_trainer runs modes 0, 1 and 2)",
    "rc_version": _HOST,
    "rc_device_count": _HOST,
    "rc_rows_plan_supported": _HOST,
    "rc_bprmf_fused_supported": _HOST,
    "rc_small_row_sums_supported": _HOST,
    "rc_sasrec_supported": _HOST,
    "rc_sasrec_dense_param_count": _HOST,
    "rc_seq_attention_supported": _HOST,
    "rc_neumf_supported": _HOST,
    "rc_neumf_train_step_supported": _HOST,
    "rc_neumf_zhead_supported": _HOST,
    "rc_tower_tail_supported": _HOST,
    "rc_list_metrics_supported": _HOST,
    "rc_full_catalogue_rank_supported": _HOST,
    "rc_bucket_plan_supported": _HOST,
    "rc_lgcn_check_shape": _HOST,
    "rc_directau_check_shape": _HOST,
    "rc_comirec_check_shape": _HOST,
    "rc_contra_check_shape": _HOST,
    "rc_buir_check_shape": _HOST,
    "rc_autoint_check_shape": _HOST,
    "rc_finalmlp_check_shape": _HOST,
}
