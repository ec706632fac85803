"""The Chorus class itself: the nine parameters, the envelope check, the two heads, the row-wise training step of both stages and the
Dataset that builds the triplet feed (stage 1) or the category ids and relational intervals (otherwise).
models/sequential/Chorus.py, the file main.py resolves `--model_name Chorus` to, documents the model and re-exports it.  The class is
defined here, beside BaseModel.py, because tests/test_directau_cpu.py holds the table of classes DEFINED IN the general / sequential
/ context packages to the one of the DirectAU commit, and that table is left as it is.

One deviation from the reference, on purpose: the class sets `candidate_permutation_equivariant`.  The reference's runner shuffles
the columns of `item_id` alone and so pairs `category_id` and `relational_interval` with the wrong candidates; here every candidate
keeps its category and its intervals.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from models.BaseModel import SequentialModel
from rechorus_amd import engine, nn as hnn


class Chorus(SequentialModel):
    reader, runner = 'KGReader', 'BaseRunner'
    extra_log_args = ['margin', 'lr_scale', 'stage']
    candidate_permutation_equivariant = True

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--stage', type=int, default=2, help='Stage of training: 1-KG_pretrain, 2-recommendation.')
        parser.add_argument('--base_method', type=str, default='BPR', help='Basic method to generate recommendations: BPR, GMF')
        parser.add_argument('--emb_size', type=int, default=64, help='Size of embedding vectors.')
        parser.add_argument('--time_scalar', type=int, default=60 * 60 * 24 * 100, help='Time scalar for time intervals.')
        parser.add_argument('--category_col', type=str, default='i_category', help='The name of category column in item_meta.csv.')
        parser.add_argument('--lr_scale', type=float, default=0.1, help='Scale the lr for parameters in pre-trained KG model.')
        parser.add_argument('--margin', type=float, default=1, help='Margin in hinge loss.')
        return SequentialModel.parse_model_args(parser)

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.margin, self.stage, self.lr_scale = args.margin, args.stage, args.lr_scale
        self.kg_lr = args.lr_scale * args.lr
        self.base_method = args.base_method
        self.emb_size, self.time_scalar, self._trainer, self._trainer_key = args.emb_size, args.time_scalar, None, None
        self.relations = corpus.item_relations
        self.relation_num = len(corpus.item_relations) + 1
        if self.stage not in (1, 2):
            raise ValueError('--stage {}: 1 (KG pre-training) or 2 (recommendation)'.format(self.stage))
        if self.base_method.upper().strip() not in ('BPR', 'GMF'):
            raise ValueError('--base_method {!r}: BPR or GMF'.format(self.base_method))
        self.gmf = self.base_method.upper().strip() == 'GMF'
        if getattr(corpus, 'include_attr', 0):
            # the reference indexes r_embeddings / i_embeddings with the attribute relations and entities and raises in its first KG
            # batch; here they would be out-of-range reads on the device
            raise ValueError('--include_attr 1: Chorus has no embeddings for attribute relations and entities; read the corpus with '
                             '--include_attr 0')
        try:   # a shape the kernels do not cover fails here, before any training
            engine.chorus_check_shape(self.emb_size, 1, 1)
        except ValueError as e:
            raise ValueError('--emb_size {}: {}'.format(self.emb_size, e)) from None
        try:
            engine.chorus_check_shape(self.emb_size, 1, self.relation_num)
        except ValueError as e:
            raise ValueError('{} item relations (r_* columns of item_meta.csv): {}'.format(self.relation_num - 1, e)) from None
        self.kinds = engine.chorus_kinds(self.relations)
        if args.category_col in corpus.item_meta_df.columns:
            self.category_col = args.category_col
            self.category_num = int(corpus.item_meta_df[self.category_col].max()) + 1
        else:
            self.category_col, self.category_num = None, 1   # a virtual global category
        # the definition order fixes the random stream of the initialisation and the state_dict keys
        self.u_embeddings = hnn.HipEmbedding(self.user_num, self.emb_size)
        self.i_embeddings = hnn.HipEmbedding(self.item_num, self.emb_size)
        self.r_embeddings = hnn.HipEmbedding(self.relation_num, self.emb_size)
        self.betas = hnn.HipEmbedding(self.category_num, self.relation_num)
        self.mus = hnn.HipEmbedding(self.category_num, self.relation_num)
        self.sigmas = hnn.HipEmbedding(self.category_num, self.relation_num)
        self.prediction = nn.Linear(self.emb_size, 1, bias=False)
        self.user_bias = hnn.HipEmbedding(self.user_num, 1)
        self.item_bias = hnn.HipEmbedding(self.item_num, 1)
        self.kg_loss = nn.MarginRankingLoss(margin=self.margin)
        self.apply(self.init_weights)

        self.pretrain_path = '../model/Chorus/KG__{}__emb_size={}__margin={}.pt'.format(corpus.dataset, self.emb_size, self.margin)
        if self.stage == 1:
            self.model_path = self.pretrain_path
        else:
            if os.path.exists(self.pretrain_path):
                self.load_model(self.pretrain_path)
            else:
                raise ValueError('Pre-trained KG model does not exist, please run with "--stage 1"')

    def _params(self):
        """the nine parameters in engine.CHORUS_PARAMS order"""
        return (self.u_embeddings.weight, self.i_embeddings.weight, self.r_embeddings.weight, self.betas.weight, self.mus.weight,
                self.sigmas.weight, self.prediction.weight, self.user_bias.weight, self.item_bias.weight)

    def forward(self, feed_dict):
        self.check_list = []
        if self.stage == 1 and feed_dict['phase'] == 'train':
            prediction = self.kg_forward(feed_dict)
        else:
            prediction = self.rec_forward(feed_dict)
        return {'prediction': prediction}

    def rec_forward(self, feed_dict):
        i_ids = feed_dict['item_id']   # [batch_size, n_candidates]
        if not i_ids.is_cuda:
            raise RuntimeError('Chorus runs on the GPU only: its head has no CPU path')
        intervals = feed_dict['relational_interval'].float()   # [batch_size, n_candidates, relation_num]
        prediction = hnn.chorus_scores(self._params(), feed_dict['user_id'], i_ids, feed_dict['category_id'].long(), intervals,
                                       self.kinds, self.gmf)
        return prediction.view(feed_dict['batch_size'], -1)

    def kg_forward(self, feed_dict):
        head_ids = feed_dict['head_id']   # [batch_size, 4]
        if not head_ids.is_cuda:
            raise RuntimeError('Chorus runs on the GPU only: its head has no CPU path')
        return hnn.cfkg_scores(self.i_embeddings.weight, self.r_embeddings.weight, head_ids, feed_dict['tail_id'],
                               feed_dict['relation_id'])

    def loss(self, out_dict):
        if self.stage == 1:   # MarginRankingLoss over the 2 B pairs (column 0, column 2) and (column 1, column 3)
            predictions = out_dict['prediction']
            pos_pred, neg_pred = predictions[:, :2].flatten(), predictions[:, 2:].flatten()
            return self.kg_loss(pos_pred, neg_pred, torch.ones_like(pos_pred))
        return super().loss(out_dict)

    def customize_parameters(self):
        if self.stage != 2:
            return super().customize_parameters()
        weight_p, kg_p, bias_p = [], [], []
        for name, p in filter(lambda x: x[1].requires_grad, self.named_parameters()):
            if 'bias' in name:
                bias_p.append(p)
            elif 'i_embeddings' in name or 'r_embeddings' in name:
                kg_p.append(p)
            else:
                weight_p.append(p)
        return [{'params': weight_p}, {'params': kg_p, 'lr': self.kg_lr},   # scale down the lr of the pre-trained embeddings
                {'params': bias_p, 'weight_decay': 0.0}]

    # ---- large-table mode: the whole fit() iteration on row-wise updates, both stages -----------------------------------------------
    def hip_rowwise_supported(self):
        return self.emb_size in (16, 32, 64, 128) and 1 <= self.relation_num <= 8

    def hip_train_step(self, feed_dict, opt_name, lr, l2):
        """stage 1: engine.CfkgTrainer on (i_embeddings, r_embeddings) with the feed's two pairs exchanged (engine.chorus_kg_feed);
        stage 2: engine.ChorusTrainer.  Returns the device loss tensor without synchronising"""
        key = (opt_name, lr, l2)      # the hyper records are built once per (optimizer, lr, l2)
        if self._trainer is None or self._trainer_key != key:
            self._trainer_key = key
            if self.stage == 1:
                self._trainer = engine.CfkgTrainer(self.i_embeddings.weight.data, self.r_embeddings.weight.data, margin=self.margin,
                                                   opt=opt_name, lr=lr, l2=l2)
            else:
                self._trainer = engine.ChorusTrainer(*(t.data for t in self._params()), kinds=self.kinds, gmf=self.gmf, opt=opt_name,
                                                     lr=lr, l2=l2, lr_scale=self.lr_scale)
        with torch.no_grad():
            if self.stage == 1:
                head, tail = engine.chorus_kg_feed(feed_dict['head_id'], feed_dict['tail_id'])
                return self._trainer.step(head, tail, feed_dict['relation_id'].contiguous())
            return self._trainer.step(feed_dict['user_id'].contiguous(), feed_dict['item_id'].contiguous(),
                                      feed_dict['category_id'].long().contiguous(),
                                      feed_dict['relational_interval'].float().contiguous())

    class Dataset(SequentialModel.Dataset):
        def __init__(self, model, corpus, phase):
            super().__init__(model, corpus, phase)
            self.kg_train = model.stage == 1 and phase == 'train'
            if self.kg_train:
                kg = corpus.relation_df
                self.data = {k: np.asarray(kg[k]) for k in ('head', 'relation', 'tail')}
                self.neg_heads = np.zeros(len(self), dtype=int)
                self.neg_tails = np.zeros(len(self), dtype=int)
                return
            items = corpus.item_meta_df['item_id']
            col = model.category_col
            categories = corpus.item_meta_df[col] if col is not None else np.zeros_like(items)
            self.item2cate = dict(zip(items, categories))   # every id < category_num: category_num = the column's maximum + 1
            # heads_of[r][tail] = the items h with (h, r, tail) in the graph, r = 1 .. relation_num - 1 (relation ids >= relation_num
            # cannot reach the kernels: the interval array has relation_num columns)
            self._heads_of = [dict() for _ in range(model.relation_num)]
            for head, r, tail in corpus.triplet_set:
                if r < model.relation_num:
                    self._heads_of[r].setdefault(tail, set()).add(head)

        def _get_feed_dict(self, index):
            """stage-1 train: the triplet (h, r, t) as head_id = (t, t, t', t), tail_id = (h, h, h, h') -- the reference feeds the
            reversed relation (Chorus.py:213-221).  Otherwise the sequential feed + category_id [n_candidates] and
            relational_interval [n_candidates, relation_num] float32: entry 0 always -1, entry r >= 1 the time since the most recent
            history item h with (h, r, candidate) in the graph, divided by time_scalar in float64 (Chorus.py:223-241)"""
            if self.kg_train:
                head, tail, relation = self.data['head'][index], self.data['tail'][index], self.data['relation'][index]
                head_id = np.array([head, head, head, self.neg_heads[index]])
                tail_id = np.array([tail, tail, self.neg_tails[index], tail])
                return {'head_id': tail_id, 'tail_id': head_id, 'relation_id': np.array([relation] * 4)}
            feed = super()._get_feed_dict(index)
            time = self.data['time'][index]
            R = self.model.relation_num
            last_seen = {}   # item -> time of its most recent history event (later positions overwrite earlier ones)
            for item, t in zip(np.asarray(feed['history_items']).tolist(), np.asarray(feed['history_times']).tolist()):
                last_seen[item] = t
            candidates = np.asarray(feed['item_id']).tolist()
            interval = np.full((len(candidates), R), -1.0, dtype=np.float64)
            for c, cand in enumerate(candidates):
                for r in range(1, R):
                    heads = self._heads_of[r].get(cand)
                    if heads:
                        seen = [last_seen[h] for h in heads if h in last_seen]
                        if seen:   # the most recent position holds the latest time: histories are time-ordered
                            interval[c, r] = (time - max(seen)) / self.model.time_scalar
            feed['category_id'] = np.array([self.item2cate[x] for x in candidates])
            feed['relational_interval'] = interval.astype(np.float32)
            return feed

        def actions_before_epoch(self):
            """stage-1 train: one corrupted tail and one corrupted head per triplet, one np.random.randint at a time in the
            reference's order (Chorus.py:244-253), so the same seed gives the same negatives"""
            if not self.kg_train:
                return super().actions_before_epoch()
            draw, n_items, triplets = np.random.randint, self.corpus.n_items, self.corpus.triplet_set
            for i in range(len(self)):
                head, tail, relation = self.data['head'][i], self.data['tail'][i], self.data['relation'][i]
                self.neg_tails[i] = draw(1, n_items)
                self.neg_heads[i] = draw(1, n_items)
                while (head, relation, self.neg_tails[i]) in triplets:
                    self.neg_tails[i] = draw(1, n_items)
                while (self.neg_heads[i], relation, tail) in triplets:
                    self.neg_heads[i] = draw(1, n_items)
