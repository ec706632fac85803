""" DirectAU on the HIP engine
Reference: "Towards Representation Alignment and Uniformity in Collaborative Filtering", Wang et al., KDD'2022.
Counterpart of the reference's models/general/DirectAU.py (same class / flag / state_dict names), e.g.
    python main.py --model_name DirectAU --emb_size 64 --lr 1e-3 --l2 1e-5 --gamma 0.3 --dataset Grocery_and_Gourmet_Food
Two embedding tables and a dot-product head; the training objective is alignment of the normalised user / item rows of a
batch plus gamma times the mean of the two sides' uniformity (DirectAU.py:54-88).  That objective is one autograd node on
rc_directau_fwd / _bwd (rechorus_amd.nn.directau_loss): the pairs of the batch are swept once on fp32 MFMA, the B x B distances
are never stored, and the backward pass hands per-occurrence row gradients to HipEmbedding, which sums them into the tables.
Every score (training prediction, evaluation, --test_all) comes from BPRMF's dot-product kernels.  Training rows bring no
negatives, so the device pipeline assembles their batches without a sampler launch.
"""
from torch import nn

from models.BaseModel import GeneralModel
from rechorus_amd import engine, nn as hnn


class DirectAU(GeneralModel):
    reader, runner = 'BaseReader', 'BaseRunner'
    extra_log_args = ['emb_size', 'gamma']
    candidate_permutation_equivariant = True   # a candidate's score depends on that candidate alone

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Width of the user and item embedding tables.')
        parser.add_argument('--gamma', type=float, default=1, help='Factor on the uniformity term of the loss.')
        return GeneralModel.parse_model_args(parser)

    @staticmethod
    def init_weights(m):
        # the model's only parameters are its two tables: Xavier-normal on each (visited users first, then items)
        if isinstance(m, hnn.HipEmbedding):
            nn.init.xavier_normal_(m.weight)

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.emb_size, self.gamma = args.emb_size, args.gamma
        engine.directau_check_shape(self.emb_size)   # an --emb_size the kernels do not cover fails before any training
        self._workspace = engine.DirectAUWorkspace()  # the loss's scratch, reused step after step (hipGraph replay)
        self.u_embeddings = hnn.HipEmbedding(self.user_num, self.emb_size)
        self.i_embeddings = hnn.HipEmbedding(self.item_num, self.emb_size)
        self.apply(self.init_weights)

    # the reference's two loss terms, for model files that build on them
    @staticmethod
    def alignment(x, y):
        return hnn.alignment(x, y)

    @staticmethod
    def uniformity(x):
        return hnn.uniformity(x)

    def forward(self, feed_dict):
        self.check_list = []
        users, candidates = feed_dict['user_id'], feed_dict['item_id']   # [B], [B, n_candidates]
        scores = hnn.bprmf_scores(self.u_embeddings.weight, self.i_embeddings.weight, users, candidates)
        out = {'prediction': scores.view(feed_dict['batch_size'], -1)}
        if feed_dict['phase'] == 'train':
            # the rows the loss works on: one user and one positive item per training row
            out['user_e'] = self.u_embeddings(users)
            out['item_e'] = self.i_embeddings(candidates[:, 0])
        return out

    def loss(self, out_dict):
        return hnn.directau_loss(out_dict['user_e'], out_dict['item_e'], self.gamma, workspace=self._workspace)

    def full_catalogue_vectors(self, feed_dict):
        """(query vectors [B, d], item table) of the dot-product head, for --test_all ranking"""
        return engine.gather_rows(self.u_embeddings.weight.detach(), feed_dict['user_id']), self.i_embeddings.weight.detach()

    class Dataset(GeneralModel.Dataset):
        empty_train_negatives = True   # read by rechorus_amd.pipeline: training batches are (user, positive) pairs

        def actions_before_epoch(self):
            # the objective needs positives only: every training row gets an empty candidate list besides its target
            self.data['neg_items'] = [[]] * len(self)
