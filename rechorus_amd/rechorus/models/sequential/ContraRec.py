""" ContraRec on the HIP engine
Reference: "Sequential Recommendation with Multiple Contrast Signals", Wang et al., TOIS'2022.
Counterpart of the reference's models/sequential/ContraRec.py (same class / flag / state_dict names), e.g.
    python main.py --model_name ContraRec --emb_size 64 --lr 1e-4 --l2 1e-6 --history_max 20 --encoder BERT4Rec \
        --num_neg 1 --ctc_temp 1 --ccc_temp 0.2 --batch_size 4096 --gamma 1 --dataset Grocery_and_Gourmet_Food
A history is encoded by two TransformerLayers with a key-padding mask and forward position ids (BERT4RecEncoder, :250-276):
rechorus_amd.nn.bert4rec_encode_layers strings the shape-generic sequence kernels together (rc_seq_embed_fwdpos_fwd, the fp32
MFMA GEMMs, rc_seq_attention_fwd/_bwd with causal = 0, rc_seq_add_layernorm_*).  Training encodes the history and its two
augmented views (Dataset.augment, :106-138: mask or reorder a Beta-distributed span) in ONE pass over 3 B sequences.  The loss
is the context-target term (:99-101, softmax cross-entropy of candidate column 0 at temperature ctc_temp, on the list-loss
kernel) plus gamma times the context-context term (:142-193), a supervised-contrastive loss over the 2 B x 2 B similarity
matrix of the two views that rc_contra_loss_fwd/_bwd computes on fp32 MFMA without storing the matrix
(rechorus_amd.nn.contra_loss).  --encoder GRU4Rec / Caser and shapes outside the kernels' envelopes are refused at construction,
nothing is rerouted.

The context-context labels are candidate column 0 AS THE FORWARD SEES IT, exactly as in the reference (:94): this class does
NOT declare `candidate_permutation_equivariant`, so BaseRunner.fit shuffles the candidate columns on the host before every
forward, as the reference's runner does, and the dense training step runs eagerly (it is not replayed from a hipGraph).
"""
from models.contrarec_model import BERT4RecEncoder, ContraRec   # the class bodies; see that module's docstring for why they live there

__all__ = ['ContraRec', 'BERT4RecEncoder']
