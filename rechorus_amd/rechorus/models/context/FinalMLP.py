""" FinalMLP on the HIP engine
Reference: 'FinalMLP: an enhanced two-stream MLP model for CTR prediction', Mao et al., AAAI 2023.
Counterpart of the reference's models/context/FinalMLP.py (same class / flag / state_dict names), e.g.
    python main.py --model_name FinalMLP --model_mode CTR --emb_size 64 --mlp1_hidden_units '[64]' --mlp2_hidden_units '[256]' \
        --fs_hidden_units '[64]' --fs1_context c_hour_c,c_weekday_c,c_period_c,c_day_f --fs2_context i_category_c,i_subcategory_c \
        --num_heads 1 --loss_n BCE --dataset MIND_Large/MINDCTR --include_item_features 1 --include_situation_features 1
Two MLP streams read the flattened field vectors X [B, C, F d] (user_id, then item_id / i_*, then c_*: FinalMLP.py:79-92), each
through its own feature gate g_s = 2 sigmoid(gate MLP(context embeddings | a learned bias)), and a bilinear head fuses their
outputs: w_x x + w_y y + sum_h x_h^T W_h y_h.  Every field, numeric ones included, comes from one rc_gather_fields launch
(rechorus_amd.nn.gather_fields_kinds).  The gate MLP's hidden layers run on rc_linear_fwd; its last Linear, the sigmoid, the product
with X and the first Linear + ReLU + Dropout of BOTH streams are one launch (rc_finalmlp_gate_fwd, rechorus_amd.nn.finalmlp_gate) that
writes neither the gates nor the gated features; its backward recomputes the gates.  A stream takes one gate row for all instances
(no contexts), one per batch row (every context a situation feature) or one per instance (an item feature among them).  The other
stream layers run on the fp32 MFMA GEMMs of csrc/mlp.hip, the fusion is rc_finalmlp_fusion_fwd / _bwd.  --use_fs 0 drops the gates:
the streams are plain MLP_Blocks.
Refused at construction with a ValueError that names the flag, nothing is rerouted: --mlp*_batch_norm 1 and hidden activations other
than ReLU (no kernels: of the reference's four demo lines CTR_ML1M.sh:20 and Topk_MIND.sh:20 set batch norm and are out of
scope, CTR_MIND.sh:20 and Topk_ML1M.sh:20 run), --fs*_context entries the
reference rejects, a corpus with u_* features or without any c_* feature (the reference itself fails on both), and shapes outside the
kernels' envelope (3..32 fields, emb_size a multiple of 4 up to 128, gate / layer widths multiples of 4 in 4..256 that fit the LDS,
num_heads a divisor of both stream outputs).
"""
from models.finalmlp_model import FinalMLPBase, FinalMLPCTR, FinalMLPTopK   # the class bodies; see that module's docstring

__all__ = ['FinalMLPBase', 'FinalMLPCTR', 'FinalMLPTopK']
