""" BUIR on the HIP engine
Reference: "Bootstrapping User and Item Representations for One-Class Collaborative Filtering", Lee et al., SIGIR'2021.
Counterpart of the reference's models/general/BUIR.py (same class / flag / state_dict names), e.g.
    python main.py --model_name BUIR --emb_size 64 --lr 1e-3 --l2 1e-6 --dataset Grocery_and_Gourmet_Food
Two online tables, two target tables of the same shape and a d x d predictor.  A training row is a (user, positive item) pair:
the predictor's image of the online user row is pulled towards the item's target row and the other way round, both after
normalisation; no negatives are drawn, so the device pipeline assembles the batches without a sampler launch.  The whole step up
to the loss -- four row gathers, the predictor on both sides, four normalisations, two dots -- and its backward are one autograd
node on rc_buir_fwd / _bwd (rechorus_amd.nn.buir_loss).  Evaluation scores <P(i), u> + <P(u), i> as <q, i> + c with one query
vector per user (rc_buir_query, rc_buir_scores); --test_all ranks the catalogue with that query vector.  After every optimizer
step BUIRRunner moves the target tables towards the online ones (`_update_target`, one launch on both tables, bit-equal to the
reference's expression).  Shapes outside the kernels' envelope are refused at construction, nothing is rerouted.
"""
from models.buir_model import BUIR   # the class body; see that module's docstring for why it lives there

__all__ = ['BUIR']
