""" SetRank on the HIP engine
Reference: "SetRank: Learning a Permutation-Invariant Ranking Model for Information Retrieval", Pang et al., SIGIR'2020.
Counterpart of the reference's models/reranker/SetRank.py (same class / flag / state_dict names), e.g.
    python main.py --model_name SetRankGeneral --ranker_name BPRMF --ranker_config_file BPRMF.yaml --ranker_model_file <checkpoint>.pt \
        --emb_size 64 --n_blocks 4 --num_heads 4 --num_hidden_unit 64 --setrank_type IMSAB --loss_n BPR --dataset MINDCTR --num_workers 0
    python main.py --model_name SetRankSequential --ranker_name SASRec --ranker_config_file SASRec.yaml --ranker_model_file <checkpoint>.pt \
        --history_max 20 --setrank_type MSAB ...
The base ranker is this repository's <ranker_name>Impression, read from ./model/<ranker_name>Impression/ and frozen; it runs on the
device inside collate_batch, so the DataLoader needs --num_workers 0.  --setrank_type MSAB (:58-65): every block is PRM's encoder block
with the position added after rFF0, ONE launch forward (rc_listenc_block_fwd).  --setrank_type IMSAB (:67-80, the default): every block
is two multihead attention blocks whose query rows are not their key rows -- 20 learned inducing points against the list under the
mask, then the list against the 20 results -- one launch each forward (rc_setmab_fwd), one launch plus the fixed-order reduces each
backward (rc_setmab_bwd); the inducing points' projection is computed once per workgroup and their gradient summed over the lists in a
fixed order.  All products run on the f32-input MFMA.
Refused at construction, nothing rerouted: --dropout > 0, --tuneranker 1, evaluation list widths that differ from the training
widths, a --setrank_type other than MSAB or IMSAB (the reference fails later, with an AttributeError), a base ranker that returns no
u_v / i_v, and a shape outside the kernels' envelope (MSAB: PRM's; IMSAB: train_max_pos_item + train_max_neg_item in [1, 64] at
num_hidden_unit <= 64, at most 48 slots at 80 and 96, at most 32 at 112 and 128; num_heads a divisor of num_hidden_unit with num_hidden_unit / num_heads a multiple
of 4).  MIR has no model file here.
"""
from models.setrank_model import SetRankBase, SetRankGeneral, SetRankSequential   # the class bodies; see that module's docstring

__all__ = ['SetRankBase', 'SetRankGeneral', 'SetRankSequential']
