""" DCNv2 on the HIP engine
Reference: 'DCN V2: Improved Deep & Cross Network and Practical Lessons for Web-scale Learning to Rank Systems', Wang et al., WWW 2021.
Counterpart of the reference's models/context/DCNv2.py (same class / flag / state_dict names), e.g.
    python main.py --model_name DCNv2 --model_mode CTR --emb_size 64 --layers '[64]' --cross_layer_num 3 --mixed 1 \
        --structure stacked --low_rank 64 --expert_num 2 --loss_n BCE --dataset MIND_Large/MINDCTR \
        --include_item_features 1 --include_situation_features 1
The F field vectors of an instance (ONE rc_gather_fields launch, numeric fields included) are flattened to x_0 [N, D = F * emb_size].
--mixed 1 (the default): per layer and expert t = tanh(V^T x_l), s = tanh(C t), y = U s + bias, a softmax gate over the experts
(one gating ModuleList shared by all layers, :62), x_{l+1} = x_l + x_0 * sum_e g_e y_e (:119-141).  Each layer is ONE launch
(rc_dcnv2_mix_layer_fwd, rechorus_amd.nn.dcnv2_mix_layer) on the f32-input MFMA; its backward (rc_dcnv2_mix_layer_bwd) recomputes
both tanh stages and the gate, so nothing of size N * E * low_rank is kept, and x_0's gradient is summed over the layers by autograd.
--mixed 0: x_{l+1} = x_0 * (W_l x_l + b_l) + x_l (:79-94) with W_l x_l + b_l on rechorus_amd.nn.linear and the rest in torch ops -- a
composition, not a kernel of its own, and not measured; the loss adds reg_weight * sum_l ||W_l||_2 (:192-198).
The tower is MLP_Block with BatchNorm1d before the ReLU and stays on torch's modules, as DIN's tower does.
Refused at construction, nothing rerouted: a --structure other than parallel / stacked (the reference leaves predict_layer undefined),
and with --mixed 1 a width F * emb_size outside the multiples of 4 in [8, 1024], a --low_rank outside the multiples of 4 in [4, 128],
an --expert_num outside [1, 4].  DCN (v1), xDeepFM and SAM have no model file here.
"""
from models.dcnv2_model import DCNv2Base, DCNv2CTR, DCNv2TopK   # the class bodies; see that module's docstring

__all__ = ['DCNv2Base', 'DCNv2CTR', 'DCNv2TopK']
