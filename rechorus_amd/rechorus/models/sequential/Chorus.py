""" Chorus on the HIP engine
Reference: "Make It a Chorus: Knowledge- and Time-aware Item Modeling for Sequential Recommendation", Wang et al., SIGIR'2020.
Counterpart of the reference's models/sequential/Chorus.py (same class / flag / state_dict names), in two stages:
    python main.py --model_name Chorus --emb_size 64 --margin 1 --lr 5e-4 --l2 1e-5 --epoch 50 --early_stop 0 \
        --batch_size 512 --dataset Grocery_and_Gourmet_Food --stage 1
    python main.py --model_name Chorus --emb_size 64 --margin 1 --lr_scale 0.1 --lr 1e-3 --l2 0 \
        --dataset Grocery_and_Gourmet_Food --base_method BPR --stage 2
Stage 1 pre-trains i_embeddings / r_embeddings with TransE on the item-item graph read by helpers/KGReader.py (the launch sequence
of CFKG: rc_cfkg_scores / rc_cfkg_fwd_bwd, with the feed's two pairs exchanged) and saves them under the reference's path and key
names; stage 2 loads that file (a missing one is a ValueError) and scores a candidate by its embedding plus its relational
embeddings, each weighted by a temporal kernel of the time since the user's most recent related history item,
    z = (1 + sum_r decay_r) i + sum_r decay_r rel_r,    prediction = <u, z> + user_bias + item_bias    (GMF: <w o u, z>),
with an exponential kernel for relation 0, a normal one for 'complement' columns and a difference of normals for 'substitute'
columns, their parameters read from three [category_num, relation_num] tables.  The head is one kernel (rc_chorus_scores;
rechorus_amd.nn.chorus_scores with a HIP backward to every dense gradient); `--engine rowwise` runs the whole iteration on
rc_chorus_fwd_bwd, rc_segmented_update, rc_slrc_user_bias_update, rc_chorus_category_update and rc_dense_update
(engine.ChorusTrainer) with the three learning-rate / weight-decay groups of customize_parameters.  The Dataset builds
`category_id` and `relational_interval` on the host, so the model takes the DataLoader path.  Unlike the reference's runner, which
shuffles the columns of `item_id` but not those of `category_id` and `relational_interval`, training here keeps every category and
interval with its candidate -- on purpose.  Refused at construction, with the flag named: an `--emb_size` outside
{16, 32, 64, 128}, more than seven item relations, a `--base_method` other than BPR / GMF, and a corpus read with `--include_attr 1`.
"""
from models.chorus_model import Chorus   # the class body; see that module's docstring for why it lives there

__all__ = ['Chorus']
