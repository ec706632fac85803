""" AutoInt on the HIP engine
Reference: 'AutoInt: Automatic Feature Interaction Learning via Self-Attentive Neural Networks', Song et al., CIKM 2018.
Counterpart of the reference's models/context/AutoInt.py (same class / flag / state_dict names), e.g.
    python main.py --model_name AutoInt --model_mode CTR --emb_size 64 --attention_size 32 --num_heads 1 --num_layers 1 \
        --layers '[64]' --loss_n BCE --dataset MIND_Large/MINDCTR --include_item_features 1 --include_situation_features 1
The F field vectors of one instance attend to each other: per layer Q | K | V = X W^T (utils.layers.MultiHeadAttention, no bias, no
output projection), softmax(Q_h K_h^T / sqrt(dk)) V_h per head, a linear residual X Wr^T + br, ReLU (:72-75); the flattened result
feeds MLP_Block, and the first-order term is FM's (:76-80).  The field vectors come from the one rc_gather_fields launch every
context head shares; each layer is ONE launch (rc_autoint_layer_fwd, rechorus_amd.nn.autoint_layer) whose backward
(rc_autoint_layer_bwd) recomputes Q, K, V and the softmax from X, so nothing of size N F F or N F 3A is kept.  The tower runs on
the fp32 MFMA GEMMs of csrc/mlp.hip; CTR training with --loss_n BCE goes through rc_ctr_head_fwd_bwd like WideDeep.
The reference shifts the scores by their global maximum and replaces NaN by 0 (utils/layers.py:60-61); for finite inputs that is
a no-op and the kernels use the row maximum.  Shapes outside the kernels' envelope (2..32 fields, widths a multiple of 4 up to
128, attention_size 4..64 divisible by num_heads) are refused at construction, nothing is rerouted.
"""
from models.autoint_model import AutoIntBase, AutoIntCTR, AutoIntTopK   # the class bodies; see that module's docstring

__all__ = ['AutoIntBase', 'AutoIntCTR', 'AutoIntTopK']
