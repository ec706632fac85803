""" ComiRec on the HIP engine
Reference: "Controllable Multi-Interest Framework for Recommendation", Cen et al., KDD'2020.
Counterpart of the reference's models/sequential/ComiRec.py (same class / flag / state_dict names), e.g.
    python main.py --model_name ComiRec --emb_size 64 --lr 1e-3 --l2 1e-6 --attn_size 8 --K 4 --add_pos 1 \
        --history_max 20 --dataset Grocery_and_Gourmet_Food
A sequence is summarised by K interest vectors: a two-layer attention (emb_size -> attn_size -> K, tanh between) over the
history rows plus their position rows gives K softmax distributions over the positions, each of which pools the history rows
themselves (ComiRec.py:64-80).  Training keeps, per sequence, the interest that scores the item in candidate column 0 highest
and scores every candidate with it; evaluation takes each candidate's best interest (:82-91).  Gather, attention, masked
softmax, pooling and selection are ONE launch (rc_comirec_fwd, rechorus_amd.nn.comirec_user_vector) whose backward
(rc_comirec_bwd) hands per-occurrence row gradients to the engine's dense table-gradient kernels; the evaluation head is
rc_comirec_score_max.  Shapes outside the kernels' envelope are refused at construction, nothing is rerouted.

"Column 0" is whatever the runner's candidate shuffle puts there, exactly as in the reference: this class does NOT declare
`candidate_permutation_equivariant`, so BaseRunner.fit shuffles the candidate columns on the host before every forward and the
dense training step runs eagerly (it is not replayed from a hipGraph).
"""
from models.comirec_model import ComiRec   # the class body; see that module's docstring for why it lives there

__all__ = ['ComiRec']
