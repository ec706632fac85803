""" PRM on the HIP engine
Reference: "Personalized Re-ranking for Recommendation", Pei et al., RecSys'2019.
Counterpart of the reference's models/reranker/PRM.py (same class / flag / state_dict names), e.g.
    python main.py --model_name PRMGeneral --ranker_name BPRMF --ranker_config_file BPRMF.yaml --ranker_model_file <checkpoint>.pt \
        --emb_size 64 --n_blocks 4 --num_heads 4 --num_hidden_unit 64 --loss_n BPR --dataset MINDCTR --num_workers 0
    python main.py --model_name PRMSequential --ranker_name SASRec --ranker_config_file SASRec.yaml --ranker_model_file <checkpoint>.pt \
        --history_max 20 ...
The base ranker is this repository's <ranker_name>Impression, read from ./model/<ranker_name>Impression/ and frozen; it runs on the
device inside collate_batch, so the DataLoader needs --num_workers 0.  Every encoder block (nn.TransformerEncoderLayer(num_hidden_unit,
num_heads, 128), post-norm, under the key-padding mask, :64 and :90-92) is ONE launch forward (rc_listenc_block_fwd) and one launch
plus a fixed-order reduce backward (rc_listenc_block_bwd), all products on the f32-input MFMA.
Refused at construction, nothing rerouted: --dropout > 0, --tuneranker 1, evaluation list widths that differ from the training
widths, a base ranker that returns no u_v / i_v, and a shape outside the kernels' envelope (train_max_pos_item + train_max_neg_item
in [1, 64], num_hidden_unit a multiple of 16 in [16, 128] -- at 80 at most 48 slots, at 96, 112 and 128 at most 32 --, num_heads a divisor of it with
num_hidden_unit / num_heads a multiple of 4).  SetRank is models/reranker/SetRank.py; MIR has no model file here.
"""
from models.prm_model import PRMBase, PRMGeneral, PRMSequential   # the class bodies; see that module's docstring

__all__ = ['PRMBase', 'PRMGeneral', 'PRMSequential']
