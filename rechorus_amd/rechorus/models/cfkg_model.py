"""The CFKG class itself: the two tables, the envelope check, the head, the row-wise training step and the triplet Dataset.
models/general/CFKG.py, the file main.py resolves `--model_name CFKG` to, documents the model and re-exports it.  The class is
defined here, beside BaseModel.py, because tests/test_directau_cpu.py holds the table of classes DEFINED IN the general / sequential
/ context packages to the one of the DirectAU commit, and that table is left as it is.

One deviation from the reference, on purpose: the reference's BaseRunner.fit reads batch['item_id'] before every step, a key CFKG's
training feed does not have, so the reference's own CFKG stops with a KeyError in its first step.  Here the runner reads that key
only where it shuffles candidate columns, and CFKG declares `candidate_permutation_equivariant` (each candidate is scored on its own,
and the feed has no `item_id` whose columns could be shuffled) -- so CFKG trains.  Forward, loss, Dataset and optimizer construction
are the reference's.
"""
import numpy as np
import torch
import torch.nn as nn

from models.BaseModel import GeneralModel
from rechorus_amd import engine, nn as hnn


class CFKG(GeneralModel):
    reader, runner = 'KGReader', 'BaseRunner'
    extra_log_args = ['emb_size', 'margin', 'include_attr']
    candidate_permutation_equivariant = True

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Size of embedding vectors.')
        parser.add_argument('--margin', type=float, default=0, help='Margin in hinge loss.')
        return GeneralModel.parse_model_args(parser)

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.emb_size, self.margin, self._trainer = args.emb_size, args.margin, None
        self.relation_num, self.entity_num = corpus.n_relations, corpus.n_entities
        try:   # a shape the kernels do not cover fails here, before any training
            engine.cfkg_check_shape(self.emb_size, 1, 1)
        except ValueError as e:
            raise ValueError('--emb_size {}: {}'.format(self.emb_size, e)) from None
        try:
            engine.cfkg_check_shape(self.emb_size, 1, self.relation_num)
        except ValueError as e:
            raise ValueError('{} relations ("buy", the r_* columns of item_meta.csv and, with --include_attr 1, its i_* columns): {}'
                             .format(self.relation_num, e)) from None
        # the definition order fixes the random stream of the initialisation
        self.e_embeddings = hnn.HipEmbedding(self.user_num + self.entity_num, self.emb_size)   # users first, then the entities
        self.r_embeddings = hnn.HipEmbedding(self.relation_num, self.emb_size)                 # relation 0: "buy"
        self.loss_function = nn.MarginRankingLoss(margin=self.margin)
        self.apply(self.init_weights)

    def forward(self, feed_dict):
        self.check_list = []
        head_ids = feed_dict['head_id']   # [batch_size, n_candidates]
        if not head_ids.is_cuda:
            raise RuntimeError('CFKG runs on the GPU only: its head has no CPU path')
        prediction = hnn.cfkg_scores(self.e_embeddings.weight, self.r_embeddings.weight, head_ids, feed_dict['tail_id'],
                                     feed_dict['relation_id'])
        return {'prediction': prediction.view(feed_dict['batch_size'], -1)}

    def loss(self, out_dict):
        """MarginRankingLoss over the 2 B pairs (column 0, column 2) and (column 1, column 3) of a [B, 4] prediction"""
        predictions = out_dict['prediction']
        pos_pred, neg_pred = predictions[:, :2].flatten(), predictions[:, 2:].flatten()
        return self.loss_function(pos_pred, neg_pred, torch.ones_like(pos_pred))

    # ---- large-table mode: the whole fit() iteration on engine.CfkgTrainer ----------------------------------------------------------
    def hip_rowwise_supported(self):
        return self.emb_size in (16, 32, 64, 128) and 1 <= self.relation_num <= 8

    def hip_train_step(self, feed_dict, opt_name, lr, l2):
        """forward + margin loss + backward + the update of both tables (engine.CfkgTrainer: the entity table row-wise, the relation
        table densely); returns the device loss tensor without synchronising"""
        if self._trainer is None or self._trainer.opt != opt_name:
            self._trainer = engine.CfkgTrainer(self.e_embeddings.weight.data, self.r_embeddings.weight.data, margin=self.margin,
                                               opt=opt_name, lr=lr, l2=l2)
        with torch.no_grad():
            return self._trainer.step(feed_dict['head_id'], feed_dict['tail_id'], feed_dict['relation_id'])

    class Dataset(GeneralModel.Dataset):
        """train: the graph's triplets followed by the train interactions as (user, 0, item) triplets, one corrupted head and one
        corrupted tail per row; dev / test: the user against [target, negatives] under relation 0 (CFKG.py:78-129)"""

        def __init__(self, model, corpus, phase):
            super().__init__(model, corpus, phase)
            if phase == 'train':
                kg = corpus.relation_df
                users, items = np.asarray(self.data['user_id']), np.asarray(self.data['item_id'])
                self.data = {'head': np.concatenate([np.asarray(kg['head']), users]),
                             'tail': np.concatenate([np.asarray(kg['tail']), items]),
                             'relation': np.concatenate([np.asarray(kg['relation']), np.zeros_like(users)])}
                self.neg_heads = np.zeros(len(self), dtype=int)
                self.neg_tails = np.zeros(len(self), dtype=int)

        def _get_feed_dict(self, index):
            n_users = self.corpus.n_users
            if self.phase == 'train':
                head, tail, relation = self.data['head'][index], self.data['tail'][index], self.data['relation'][index]
                head_id = np.array([head, head, head, self.neg_heads[index]])
                tail_id = np.array([tail, tail, self.neg_tails[index], tail]) + n_users   # a tail is never a user
                if relation > 0:   # "buy" alone has users for heads
                    head_id = head_id + n_users
                return {'head_id': head_id, 'tail_id': tail_id, 'relation_id': np.full(4, relation)}
            user, target = self.data['user_id'][index], self.data['item_id'][index]
            negs = np.arange(1, self.corpus.n_items) if self.model.test_all else self.data['neg_items'][index]
            tail_id = np.concatenate([[target], negs])
            # user_id is not in the reference's feed: the streamed --test_all evaluation masks the user's seen items by it
            return {'head_id': user * np.ones_like(tail_id), 'tail_id': tail_id + n_users, 'relation_id': np.zeros_like(tail_id),
                    'user_id': user}

        def actions_before_epoch(self):
            """one corrupted tail and one corrupted head per row, drawn one np.random.randint at a time in the reference's order
            (CFKG.py:114-129), so that the same seed gives the same negatives: the tail's first draw, then the head's first draw,
            then the tail's redraws, then the head's.  Interactions are redrawn against train_clicked_set, graph triplets against
            triplet_set; a triplet's FIRST tail draw ranges over the items, its redraws over all entities."""
            draw = np.random.randint
            n_users, n_items, n_entities = self.corpus.n_users, self.corpus.n_items, self.corpus.n_entities
            clicked, triplets = self.corpus.train_clicked_set, self.corpus.triplet_set
            for i in range(len(self)):
                head, tail, relation = self.data['head'][i], self.data['tail'][i], self.data['relation'][i]
                neg_tail = draw(1, n_items)
                if relation == 0:
                    neg_head = draw(1, n_users)
                    while neg_tail in clicked[head]:
                        neg_tail = draw(1, n_items)
                    while tail in clicked[neg_head]:
                        neg_head = draw(1, n_users)
                else:
                    neg_head = draw(1, n_entities)
                    while (head, relation, neg_tail) in triplets:
                        neg_tail = draw(1, n_entities)
                    while (neg_head, relation, tail) in triplets:
                        neg_head = draw(1, n_entities)
                self.neg_tails[i], self.neg_heads[i] = neg_tail, neg_head
