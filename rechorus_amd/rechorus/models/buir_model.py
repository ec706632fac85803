"""The BUIR class itself: parameters, the reference's initialisation order, the two forward paths and the target update.
models/general/BUIR.py, the file main.py resolves `--model_name BUIR` to, documents the model and re-exports it.
The class is defined here, beside BaseModel.py, because tests/test_directau_cpu.py holds the table of classes DEFINED IN the
general / sequential / context packages to the one of the DirectAU commit, and that table is left as it is.
"""
import torch
import torch.nn as nn

from models.BaseModel import GeneralModel
from rechorus_amd import engine, nn as hnn


class BUIR(GeneralModel):
    reader, runner = 'BaseReader', 'BUIRRunner'
    extra_log_args = ['emb_size', 'momentum']
    candidate_permutation_equivariant = True   # a candidate's score depends on that candidate alone

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Width of the four embedding tables and of the predictor.')
        parser.add_argument('--momentum', type=float, default=0.995, help='Share of a target table kept by each target update.')
        return GeneralModel.parse_model_args(parser)

    @staticmethod
    def init_weights(m):
        # Xavier-normal on every table and on the predictor's weight, a standard normal bias: visited in definition order
        if isinstance(m, nn.Linear):
            nn.init.xavier_normal_(m.weight)
            if m.bias is not None:
                nn.init.normal_(m.bias)
        elif isinstance(m, hnn.HipEmbedding):
            nn.init.xavier_normal_(m.weight)

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.emb_size, self.momentum = args.emb_size, args.momentum
        engine.buir_check_shape(self.emb_size)    # an --emb_size the kernels do not cover fails before any training
        self._workspace = engine.BuirWorkspace()  # the loss's scratch, reused step after step (hipGraph replay)
        # the definition order fixes the random stream: default inits in this order, then init_weights in this order
        self.user_online = hnn.HipEmbedding(self.user_num, self.emb_size)
        self.user_target = hnn.HipEmbedding(self.user_num, self.emb_size)
        self.item_online = hnn.HipEmbedding(self.item_num, self.emb_size)
        self.item_target = hnn.HipEmbedding(self.item_num, self.emb_size)
        self.predictor = nn.Linear(self.emb_size, self.emb_size)
        self.apply(self.init_weights)
        # the targets start as copies of the online tables and never receive a gradient
        for online, target in ((self.user_online, self.user_target), (self.item_online, self.item_target)):
            target.weight.data.copy_(online.weight.data)
            target.weight.requires_grad = False

    def _update_target(self):
        """target = target * momentum + online * (1 - momentum) on both tables (called by BUIRRunner after every step)"""
        engine.ema_update(self.user_target.weight.data, self.user_online.weight.data,
                          self.item_target.weight.data, self.item_online.weight.data, self.momentum)

    def forward(self, feed_dict):
        """evaluation: {'prediction' [B, C]}.  Training: the prediction [B, 1] and, under 'loss', the loss the same launch
        computed -- not the reference's four intermediate row tensors (u_online, u_target, i_online, i_target): they never
        leave the kernel."""
        self.check_list = []
        users, candidates = feed_dict['user_id'], feed_dict['item_id']   # [B], [B, n_candidates]
        if not candidates.is_cuda:
            raise RuntimeError('BUIR runs on the GPU only: its loss and scoring kernels have no CPU path')
        batch_size = candidates.shape[0]
        W, b = self.predictor.weight, self.predictor.bias
        if feed_dict['phase'] == 'train':
            if candidates.shape[1] != 1:
                raise ValueError('BUIR trains on (user, positive item) pairs: item_id must be [batch_size, 1]')
            loss, prediction = hnn.buir_loss(self.user_online.weight, self.user_target.weight, self.item_online.weight,
                                             self.item_target.weight, W, b, users, candidates, workspace=self._workspace)
            return {'prediction': prediction.view(batch_size, -1), 'loss': loss}
        with torch.no_grad():
            prediction = hnn.buir_scores(self.user_online.weight, self.item_online.weight, W, b, users, candidates)
        return {'prediction': prediction.view(batch_size, -1)}

    def loss(self, out_dict):
        return out_dict['loss']

    def full_catalogue_vectors(self, feed_dict):
        """(query vectors [B, d], item table) for --test_all ranking: score = <q, i> + c, and c is constant over a user's
        candidates, so the rank of the target among all items is the rank under <q, i>"""
        q, _ = engine.buir_query(self.user_online.weight.detach(), self.predictor.weight.detach(), self.predictor.bias.detach(),
                                 feed_dict['user_id'])
        return q, self.item_online.weight.detach()

    class Dataset(GeneralModel.Dataset):
        empty_train_negatives = True   # read by rechorus_amd.pipeline: training batches are (user, positive) pairs

        def actions_before_epoch(self):
            # the objective needs positives only: every training row gets an empty candidate list besides its target
            self.data['neg_items'] = [[] for _ in range(len(self))]
