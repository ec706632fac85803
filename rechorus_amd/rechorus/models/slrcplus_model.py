"""The SLRCPlus class itself: the ten parameters, the envelope check, the head, the row-wise training step and the Dataset that
builds the relational intervals.  models/sequential/SLRCPlus.py, the file main.py resolves `--model_name SLRCPlus` to, documents the
model and re-exports it.  The class is defined here, beside BaseModel.py, because tests/test_directau_cpu.py holds the table of
classes DEFINED IN the general / sequential / context packages to the one of the DirectAU commit, and that table is left as it is.
"""
import numpy as np
import torch
import torch.nn as nn

from models.BaseModel import SequentialModel
from rechorus_amd import engine, nn as hnn


class SLRCPlus(SequentialModel):
    reader, runner = 'KGReader', 'BaseRunner'
    extra_log_args = ['emb_size']
    # every candidate is scored on its own, so the runner does not shuffle the candidate columns -- a shuffle of `item_id` alone
    # would pair the columns of `relational_interval` with the wrong candidates
    candidate_permutation_equivariant = True

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Size of embedding vectors.')
        parser.add_argument('--time_scalar', type=int, default=60 * 60 * 24 * 100, help='Time scalar for time intervals.')
        return SequentialModel.parse_model_args(parser)

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.emb_size, self.time_scalar, self._trainer = args.emb_size, args.time_scalar, None
        self.relation_num = len(corpus.item_relations) + 1
        try:   # a shape the kernels do not cover fails here, before any training
            engine.slrc_check_shape(self.emb_size, 1, 1)
        except ValueError as e:
            raise ValueError('--emb_size {}: {}'.format(self.emb_size, e)) from None
        try:
            engine.slrc_check_shape(self.emb_size, 1, self.relation_num)
        except ValueError as e:
            raise ValueError('{} item relations (r_* columns of item_meta.csv): {}'.format(self.relation_num - 1, e)) from None
        # the definition order fixes the random stream of the initialisation
        self.u_embeddings = hnn.HipEmbedding(self.user_num, self.emb_size)
        self.i_embeddings = hnn.HipEmbedding(self.item_num, self.emb_size)
        self.user_bias = hnn.HipEmbedding(self.user_num, 1)
        self.item_bias = hnn.HipEmbedding(self.item_num, 1)
        self.global_alpha = nn.Parameter(torch.tensor(0.))
        self.alphas = hnn.HipEmbedding(self.item_num, self.relation_num)
        self.pis = hnn.HipEmbedding(self.item_num, self.relation_num)
        self.betas = hnn.HipEmbedding(self.item_num, self.relation_num)
        self.sigmas = hnn.HipEmbedding(self.item_num, self.relation_num)
        self.mus = hnn.HipEmbedding(self.item_num, self.relation_num)
        self.apply(self.init_weights)

    def _params(self):
        """the ten parameters in engine.SLRC_PARAMS order"""
        return (self.u_embeddings.weight, self.i_embeddings.weight, self.user_bias.weight, self.item_bias.weight, self.global_alpha,
                self.alphas.weight, self.pis.weight, self.betas.weight, self.sigmas.weight, self.mus.weight)

    def forward(self, feed_dict):
        self.check_list = []
        i_ids = feed_dict['item_id']   # [batch_size, n_candidates]
        if not i_ids.is_cuda:
            raise RuntimeError('SLRCPlus runs on the GPU only: its head has no CPU path')
        intervals = feed_dict['relational_interval'].float()   # [batch_size, n_candidates, relation_num]
        prediction = hnn.slrc_scores(self._params(), feed_dict['user_id'], i_ids, intervals)
        return {'prediction': prediction.view(feed_dict['batch_size'], -1)}

    # ---- large-table mode: the whole fit() iteration on row-wise updates ---------------------------------------------------------
    def hip_rowwise_supported(self):
        return self.emb_size in (16, 32, 64, 128) and 1 <= self.relation_num <= 8

    def hip_train_step(self, feed_dict, opt_name, lr, l2):
        """forward + BPR loss + backward + row-wise optimizer update of the ten parameters (engine.SlrcTrainer); returns the device
        loss tensor without synchronising"""
        if self._trainer is None or self._trainer.opt != opt_name:
            self._trainer = engine.SlrcTrainer(*(t.data for t in self._params()), opt=opt_name, lr=lr, l2=l2)
        with torch.no_grad():
            return self._trainer.step(feed_dict['user_id'].contiguous(), feed_dict['item_id'].contiguous(),
                                      feed_dict['relational_interval'].float().contiguous())

    class Dataset(SequentialModel.Dataset):
        def __init__(self, model, corpus, phase):
            super().__init__(model, corpus, phase)
            # heads_of[r][tail] = the items h with (h, r, tail) in the graph, r = 1 .. relation_num - 1
            self._heads_of = [dict() for _ in range(model.relation_num)]
            for head, r, tail in corpus.triplet_set:
                if r < model.relation_num:
                    self._heads_of[r].setdefault(tail, set()).add(head)

        def _get_feed_dict(self, index):
            """the sequential feed dict + relational_interval [n_candidates, relation_num] float32: entry 0 the time since the most
            recent history event of the candidate itself, entry r >= 1 since the most recent history item h with (h, r, candidate)
            in the graph, both divided by time_scalar in float64; -1 where there is none (SLRCPlus.py:91-116)"""
            feed = super()._get_feed_dict(index)
            time = self.data['time'][index]
            R = self.model.relation_num
            last_seen = {}   # item -> time of its most recent history event (later positions overwrite earlier ones)
            for item, t in zip(feed['history_items'].tolist(), feed['history_times'].tolist()):
                last_seen[item] = t
            candidates = feed['item_id'].tolist()
            interval = np.full((len(candidates), R), -1.0, dtype=np.float64)
            for c, cand in enumerate(candidates):
                t = last_seen.get(cand)
                if t is not None:
                    interval[c, 0] = (time - t) / self.model.time_scalar
                for r in range(1, R):
                    heads = self._heads_of[r].get(cand)
                    if heads:
                        seen = [last_seen[h] for h in heads if h in last_seen]
                        if seen:   # the most recent position holds the latest time: histories are time-ordered
                            interval[c, r] = (time - max(seen)) / self.model.time_scalar
            feed['relational_interval'] = interval.astype(np.float32)
            return feed
