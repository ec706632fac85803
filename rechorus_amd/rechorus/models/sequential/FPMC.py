""" FPMC on the HIP engine
Reference: "Factorizing Personalized Markov Chains for Next-Basket Recommendation", Rendle et al., WWW'2010.
Counterpart of the reference's models/sequential/FPMC.py (same class / flag / state_dict names), e.g.
    python main.py --model_name FPMC --emb_size 64 --lr 1e-3 --l2 1e-6 --history_max 20 --dataset Grocery_and_Gourmet_Food
Four tables and two terms: a candidate is scored by the user's taste and by the transition from the last item of the history,
    prediction[b, c] = <ui[user], iu[item_bc]> + <li[last item], il[item_bc]>            (FPMC.py:44-56).
Both candidate rows are read once by one lane-group (rc_fpmc_scores; rechorus_amd.nn.fpmc_scores with a HIP backward to four
dense gradients); `--engine rowwise` runs the whole iteration on rc_fpmc_fwd_bwd, rc_fpmc_item_update and two
rc_segmented_update calls (engine.FpmcTrainer), touching only the rows of the batch.  `--test_all 1` scores the whole catalogue
through the same head (C = n_items): the two-term score is not one [B, d] x [n, d] product, so there is no
`full_catalogue_vectors`.  An `--emb_size` outside {16, 32, 64, 128} is refused at construction.
"""
from models.fpmc_model import FPMC   # the class body; see that module's docstring for why it lives there

__all__ = ['FPMC']
