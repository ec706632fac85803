""" DIN on the HIP engine
Reference: 'Deep interest network for click-through rate prediction', Zhou et al., SIGKDD 2018.
Counterpart of the reference's models/context_seq/DIN.py (same class / flag / state_dict names), e.g.
    python main.py --model_name DIN --model_mode CTR --emb_size 64 --att_layers '[64,64]' --dnn_layers '[64]' --history_max 40 \
        --loss_n BCE --dataset MIND_Large/MINDCTR --include_item_features 1 --include_situation_features 1
The candidate's field vectors attend over the user's history of item (and, with --add_historical_situations 1, situation) field
vectors: an MLP on [q, k, q - k, q * k] per history position (Linear -> Sigmoid -> Dropout, Linear(., 1)), scores masked to 0 past
the history length (no softmax), divided by sqrt(H), keys summed with those weights; the result, its product with the candidate
and every context field feed a Linear -> BatchNorm1d -> Dice -> Dropout tower (:142-160).
Here the field vectors come from the field gather every context head shares (the history with L in the candidate slot), the
whole attention unit is ONE autograd node on csrc/din.hip (rechorus_amd.nn.din_attention: folded first layer on fp32 MFMA, no
[N, L, 4H] tensor, atomic-free backward), and the tower's Linear layers, BatchNorm1d and Dice stay torch modules.
Shapes outside the attention kernels' envelope ((item [+ situation] fields) x emb_size a multiple of 4 up to 512, --att_layers 1 to
3 widths, multiples of 16 up to 256 and at most 256 together, --history_max in [1, 64]) are refused at construction.
Reader helpers.ContextSeqReader; DIEN, CAN, ETA and SDIM of the same family are not built.
"""
from models.din_model import DINBase, DINCTR, DINTopK   # the class bodies; see that module's docstring

__all__ = ['DINBase', 'DINCTR', 'DINTopK']
