""" CFKG on the HIP engine
Reference: "Learning over Knowledge-Base Embeddings for Recommendation", Zhang et al., SIGIR'2018.
Counterpart of the reference's models/general/CFKG.py (same class / flag / state_dict names), e.g.
    python main.py --model_name CFKG --emb_size 64 --margin 1 --include_attr 1 --lr 1e-4 --l2 1e-6 --dataset Grocery_and_Gourmet_Food
A knowledge-graph embedding model: users and the other entities (items, and with --include_attr 1 attribute values) share ONE table,
users first; relation 0 is "buy", the others are the `r_*` (and `i_*`) columns of item_meta.csv read by helpers/KGReader.py.
    prediction[b, c] = -|| e[head] + r[relation] - e[tail] ||^2
trained with a margin hinge on (h, r, t) against (h, r, t') and against (h', r, t).  The head is one kernel (rc_cfkg_scores;
rechorus_amd.nn.cfkg_scores with a HIP backward to two dense gradients); `--engine rowwise` runs the whole iteration on
rc_cfkg_fwd_bwd, rc_sort_ids, rc_segmented_update and rc_dense_update (engine.CfkgTrainer): the entity table row-wise, the
relation table (at most 8 rows) densely.  The Dataset samples corrupted heads and tails on the host in the reference's draw order,
so the model takes the DataLoader path.  Unlike the reference, whose runner reads `item_id` from a feed that has none and stops in
the first step, this model trains.  An `--emb_size` outside {16, 32, 64, 128} or more than 8 relations is refused at
construction.
"""
from models.cfkg_model import CFKG   # the class body; see that module's docstring for why it lives there

__all__ = ['CFKG']
