"""The ComiRec class itself: parameters, the envelope check and the two forward paths.
models/sequential/ComiRec.py, the file main.py resolves `--model_name ComiRec` to, documents the model and re-exports it.
The class is defined here, beside BaseModel.py, because tests/test_directau_cpu.py holds the table of classes DEFINED IN the
general / sequential / context packages to the one of the DirectAU commit, and that table is left as it is.
"""
import torch
import torch.nn as nn

from models.BaseModel import SequentialModel
from rechorus_amd import engine, nn as hnn


class ComiRec(SequentialModel):
    reader, runner = 'SeqReader', 'BaseRunner'
    extra_log_args = ['emb_size', 'attn_size', 'K']

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Width of the item and position embedding tables.')
        parser.add_argument('--attn_size', type=int, default=8, help='Hidden width of the interest attention.')
        parser.add_argument('--K', type=int, default=2, help='Number of interest vectors per sequence.')
        parser.add_argument('--add_pos', type=int, default=1, help='1: position rows are added to the attention input.')
        return SequentialModel.parse_model_args(parser)

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.emb_size, self.attn_size, self.K = args.emb_size, args.attn_size, args.K
        self.add_pos, self.max_his = args.add_pos, args.history_max
        # a flag combination the kernels do not cover fails here, before any training
        engine.comirec_check_shape(self.emb_size, self.attn_size, self.K, self.max_his)
        self._workspace = engine.ComiRecWorkspace()   # the backward's scratch, reused step after step
        self.i_embeddings = hnn.HipEmbedding(self.item_num, self.emb_size)
        if self.add_pos:
            self.p_embeddings = hnn.HipEmbedding(self.max_his + 1, self.emb_size)
        self.W1 = nn.Linear(self.emb_size, self.attn_size)
        self.W2 = nn.Linear(self.attn_size, self.K)
        self.apply(self.init_weights)

    def _tensors(self):
        pos = self.p_embeddings.weight if self.add_pos else None
        return self.i_embeddings.weight, pos, self.W1.weight, self.W1.bias, self.W2.weight, self.W2.bias

    def forward(self, feed_dict):
        self.check_list = []
        candidates = feed_dict['item_id']        # [batch_size, n_candidates]
        history = feed_dict['history_items']     # [batch_size, <= history_max], right padded with 0
        lengths = feed_dict['lengths']           # [batch_size]
        batch_size = candidates.shape[0]
        if not candidates.is_cuda:
            raise RuntimeError('ComiRec runs on the GPU only: its interest extraction has no CPU path')
        if feed_dict['phase'] == 'train':
            user = hnn.comirec_user_vector(*self._tensors(), history, lengths, candidates[:, 0], workspace=self._workspace)
            rows = torch.arange(batch_size, device=candidates.device)
            prediction = hnn.bprmf_scores(user, self.i_embeddings.weight, rows, candidates)
        else:
            with torch.no_grad():
                prediction = hnn.comirec_scores(*self._tensors(), history, lengths, candidates)
        return {'prediction': prediction.view(batch_size, -1)}
