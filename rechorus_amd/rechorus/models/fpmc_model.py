"""The FPMC class itself: the four tables, the envelope check, the two-term head and the row-wise training step.
models/sequential/FPMC.py, the file main.py resolves `--model_name FPMC` to, documents the model and re-exports it.
The class is defined here, beside BaseModel.py, because tests/test_directau_cpu.py holds the table of classes DEFINED IN the
general / sequential / context packages to the one of the DirectAU commit, and that table is left as it is.
"""
import numpy as np
import torch

from models.BaseModel import SequentialModel
from rechorus_amd import engine, nn as hnn


class FPMC(SequentialModel):
    reader, runner = 'SeqReader', 'BaseRunner'
    extra_log_args = ['emb_size']
    candidate_permutation_equivariant = True   # every candidate is scored on its own

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Size of embedding vectors.')
        return SequentialModel.parse_model_args(parser)

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.emb_size, self._trainer = args.emb_size, None
        try:   # a width the kernels do not cover fails here, before any training
            engine.fpmc_check_shape(self.emb_size)
        except ValueError as e:
            raise ValueError('--emb_size {}: {}'.format(self.emb_size, e)) from None
        self.ui_embeddings = hnn.HipEmbedding(self.user_num, self.emb_size)
        self.iu_embeddings = hnn.HipEmbedding(self.item_num, self.emb_size)
        self.li_embeddings = hnn.HipEmbedding(self.item_num, self.emb_size)
        self.il_embeddings = hnn.HipEmbedding(self.item_num, self.emb_size)
        self.apply(self.init_weights)

    def _tables(self):
        return self.ui_embeddings.weight, self.li_embeddings.weight, self.iu_embeddings.weight, self.il_embeddings.weight

    def forward(self, feed_dict):
        self.check_list = []
        i_ids = feed_dict['item_id']   # [batch_size, n_candidates]
        if not i_ids.is_cuda:
            raise RuntimeError('FPMC runs on the GPU only: its two-term head has no CPU path')
        prediction = hnn.fpmc_scores(*self._tables(), feed_dict['user_id'], feed_dict['last_item_id'], i_ids)
        return {'prediction': prediction.view(feed_dict['batch_size'], -1)}

    # ---- large-table mode: the whole fit() iteration on row-wise updates ---------------------------------------------------------
    def hip_rowwise_supported(self):
        return self.emb_size in (16, 32, 64, 128)

    def hip_train_step(self, feed_dict, opt_name, lr, l2):
        """forward + BPR loss + backward + row-wise optimizer update of the four tables (engine.FpmcTrainer); returns the device
        loss tensor without synchronising"""
        if self._trainer is None or self._trainer.opt != opt_name:
            self._trainer = engine.FpmcTrainer(*(t.data for t in self._tables()), opt=opt_name, lr=lr, l2=l2)
        with torch.no_grad():
            return self._trainer.step(feed_dict['user_id'].contiguous(), feed_dict['last_item_id'].contiguous(),
                                      feed_dict['item_id'].contiguous())

    class Dataset(SequentialModel.Dataset):
        last_item_feed = True   # read by rechorus_amd.pipeline: the feed dict is {user_id, item_id, last_item_id}

        def _get_feed_dict(self, index):
            user_id, target_item = self.data['user_id'][index], self.data['item_id'][index]
            if self.phase != 'train' and self.model.test_all:
                neg_items = np.arange(1, self.corpus.n_items)
            else:
                neg_items = self.data['neg_items'][index]
            position = self.data['position'][index]
            return {'user_id': user_id,
                    'item_id': np.concatenate([[target_item], neg_items]).astype(int),
                    'last_item_id': self.corpus.user_his[user_id][position - 1][0]}
