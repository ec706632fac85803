""" KDA on the HIP engine
Reference: "Toward Dynamic User Intention: Temporal Evolutionary Effects of Item Relations in Sequential Recommendation",
Wang et al., TOIS 2021.
Counterpart of the reference's models/sequential/KDA.py (same class / flag / state_dict names), e.g.
    python main.py --model_name KDA --emb_size 64 --include_attr 1 --freq_rand 0 --lr 1e-3 --l2 1e-6 --num_heads 4 \
        --history_max 20 --dataset Grocery_and_Gourmet_Food
For every candidate and every relation r of the item knowledge graph (relation 0 is a virtual "any two items" relation; helpers/
KDAReader.py on helpers/KGReader.py) the history is summarised by a softmax attention whose query is the candidate seen through
the relation, (rel[r] + value) * candidate, each history item damped by a temporal kernel of the time gap that is LEARNED IN THE
FREQUENCY DOMAIN: a Fourier series per relation, initialised with the DFT of the relation's observed interval distribution and
clamped to [0, 1].  The R relational summaries pass num_layers rounds of self-attention across relations (MultiHeadAttention
without bias, W1, W2, dropout, LayerNorm), are pooled (average / max / attention by the user), added to the user vector and
scored against the candidate plus an item bias; a DistMult loss on sampled triplets is added with weight gamma.
Here the first level -- attention, softmax over the history, decay, weighted sum -- is ONE autograd node on csrc/kda.hip
(rechorus_amd.nn.kda_aggregate): one launch forward, the backward recomputes instead of keeping anything of size B C L R, no
atomics, and no tensor larger than the [B, C, R, V] output exists (the torch composition materialises two [B, C, L, R, V]
products).  user_embeddings, entity_embeddings and item_bias are HipEmbeddings; the layers over the R relations, the poolings,
kg_forward and the reference's own loss (no clamp) are torch ops.  The Dataset is built on the host (DataLoader path).  Unlike
the reference's runner, which shuffles the columns of `item_id` but not those of `item_val`, training here keeps every value
row with its candidate.  A row without a valid history position gives a zero context (the reference: NaN).
--emb_size outside {16, 32, 64, 128}, --history_max outside [1, 64], more than 8 relations or --n_dft above 256 (or below 2) is
refused at construction.  Chorus, of the same family, is not built.
"""
from models.kda_model import KDA, RelationalDynamicAggregation   # the class bodies; see that module's docstring

__all__ = ['KDA', 'RelationalDynamicAggregation']
