""" SLRC+ on the HIP engine
Reference: "Modeling Item-specific Temporal Dynamics of Repeat Consumption for Recommender Systems", Wang et al., TheWebConf'2019.
Counterpart of the reference's models/sequential/SLRCPlus.py (same class / flag / state_dict names), e.g.
    python main.py --model_name SLRCPlus --emb_size 64 --lr 5e-4 --l2 1e-5 --dataset Grocery_and_Gourmet_Food
Biased matrix factorisation plus a Hawkes excitation per candidate: for each relation r (0: the item itself, r >= 1: the r-th
`r_*` column of item_meta.csv, read by helpers/KGReader.py) the time since the most recent related history event excites the
candidate through a mixture of an exponential and a Gaussian kernel with per-item parameters,
    prediction[b, c] = <u, i> + user_bias[u] + item_bias[i] + sum_r alpha_r (pi_r Exp(beta_r)(dt_r) + (1 - pi_r) N(mu_r, sigma_r)(dt_r)) [dt_r known].
The head is one kernel (rc_slrc_scores; rechorus_amd.nn.slrc_scores with a HIP backward to ten dense gradients); `--engine rowwise`
runs the whole iteration on rc_slrc_fwd_bwd, rc_slrc_item_update, rc_segmented_update, rc_slrc_user_bias_update and rc_dense_update
(engine.SlrcTrainer), touching only the rows of the batch.  The Dataset builds `relational_interval` on the host, so the model takes
the DataLoader path.  Unlike the reference's runner, which shuffles the columns of `item_id` but not those of
`relational_interval`, training here keeps every interval with its candidate.  An `--emb_size` outside
{16, 32, 64, 128} or more than seven item relations is refused at construction.
"""
from models.slrcplus_model import SLRCPlus   # the class body; see that module's docstring for why it lives there

__all__ = ['SLRCPlus']
