"""The ContraRec classes themselves: parameters, the refusals, the two forward paths, the loss and the augmenting Dataset.
models/sequential/ContraRec.py, the file main.py resolves `--model_name ContraRec` to, documents the model and re-exports it.
The classes are defined here, beside BaseModel.py, because tests/test_directau_cpu.py holds the table of classes DEFINED IN the
general / sequential / context packages to the one of the DirectAU commit, and that table is left as it is.
"""
import numpy as np
import torch
import torch.nn as nn

from models.BaseModel import SequentialModel
from rechorus_amd import engine, nn as hnn
from utils import layers

_SOFTMAX_CE = engine.LIST_KINDS['softmaxCE']


class BERT4RecEncoder(nn.Module):
    """the parameters of the reference's BERT4RecEncoder under its names (p_embeddings, transformer_block); the computation is
    rechorus_amd.nn.bert4rec_encode_layers"""
    num_layers, num_heads = 2, 2

    def __init__(self, emb_size, max_his):
        super().__init__()
        self.p_embeddings = hnn.HipEmbedding(max_his + 1, emb_size)
        self.transformer_block = nn.ModuleList([
            layers.TransformerLayer(d_model=emb_size, d_ff=emb_size, n_heads=self.num_heads) for _ in range(self.num_layers)])

    def forward(self, item_emb, history, lengths):
        return hnn.bert4rec_encode_layers(item_emb, self.p_embeddings.weight, self.transformer_block, self.num_heads, history, lengths)


class ContraRec(SequentialModel):
    reader, runner = 'SeqReader', 'BaseRunner'
    extra_log_args = ['gamma', 'num_neg', 'batch_size', 'ctc_temp', 'ccc_temp', 'encoder']

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Width of the item and position embedding tables.')
        parser.add_argument('--gamma', type=float, default=1, help='Weight of the context-context term in the loss.')
        parser.add_argument('--beta_a', type=int, default=3, help='First shape parameter of the Beta draw behind an augmentation span.')
        parser.add_argument('--beta_b', type=int, default=3, help='Second shape parameter of the Beta draw behind an augmentation span.')
        parser.add_argument('--ctc_temp', type=float, default=1, help='Temperature of the context-target term.')
        parser.add_argument('--ccc_temp', type=float, default=0.2, help='Temperature of the context-context term.')
        parser.add_argument('--encoder', type=str, default='BERT4Rec',
                            help='Sequence encoder: BERT4Rec (GRU4Rec and Caser have no kernels and are refused).')
        return SequentialModel.parse_model_args(parser)

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.emb_size, self.max_his = args.emb_size, args.history_max
        self.gamma, self.beta_a, self.beta_b = args.gamma, args.beta_a, args.beta_b
        self.ctc_temp, self.ccc_temp = args.ctc_temp, args.ccc_temp
        self.encoder_name = args.encoder
        self.mask_token = corpus.n_items
        # a flag combination the kernels do not cover fails here, before any training; nothing is rerouted
        if self.encoder_name in ('GRU4Rec', 'Caser'):
            raise ValueError('ContraRec on the HIP engine: --encoder {} has no kernels; only --encoder BERT4Rec is '
                             'implemented'.format(self.encoder_name))
        if self.encoder_name != 'BERT4Rec':
            raise ValueError('Invalid sequence encoder.')
        if not hnn.sasrec_layers_supported(self.emb_size, BERT4RecEncoder.num_heads, self.max_his):
            raise ValueError('ContraRec on the HIP engine: --emb_size {} / --history_max {} is outside the encoder kernels (emb_size '
                             'a multiple of 4 up to 1024 that the 2 heads divide, history in [1, 1024])'.format(self.emb_size, self.max_his))
        try:
            engine.contra_check_shape(self.emb_size, getattr(args, 'batch_size', 1))
        except ValueError as e:
            raise ValueError('{} (--emb_size / --batch_size)'.format(e)) from None
        self._workspace = engine.ContraWorkspace()   # the loss kernels' scratch, reused step after step
        self._targets = {}
        self.i_embeddings = hnn.HipEmbedding(self.item_num + 1, self.emb_size)   # the last row is the mask token's
        self.encoder = BERT4RecEncoder(self.emb_size, self.max_his)
        self.apply(self.init_weights)

    def forward(self, feed_dict):
        self.check_list = []
        i_ids = feed_dict['item_id']             # [batch_size, n_candidates]
        history = feed_dict['history_items']     # [batch_size, <= history_max], right padded with 0
        lengths = feed_dict['lengths']           # [batch_size]
        batch_size = i_ids.shape[0]
        if not i_ids.is_cuda:
            raise RuntimeError('ContraRec runs on the GPU only: its encoder and losses have no CPU path')
        rows = torch.arange(batch_size, device=i_ids.device)
        if feed_dict['phase'] != 'train':
            with torch.no_grad():
                his_vector = self.encoder(self.i_embeddings.weight, history, lengths)
                prediction = hnn.bprmf_scores(his_vector, self.i_embeddings.weight, rows, i_ids)
            return {'prediction': prediction.view(batch_size, -1)}
        # the original history and its two augmented views share `lengths`: ONE encoder pass over 3 B sequences (the encoder is
        # per sequence and has no dropout, so this is the reference's three passes)
        stacked = torch.cat([history, feed_dict['history_items_a'], feed_dict['history_items_b']], dim=0)
        vectors = self.encoder(self.i_embeddings.weight, stacked, lengths.repeat(3))
        his_vector, view_a, view_b = vectors[:batch_size], vectors[batch_size:2 * batch_size], vectors[2 * batch_size:]
        prediction = hnn.bprmf_scores(his_vector, self.i_embeddings.weight, rows, i_ids)
        # 'views': the two views' encoder outputs, un-normalised (the reference's F.normalize is part of the loss kernels)
        return {'prediction': prediction.view(batch_size, -1), 'views': (view_a, view_b), 'labels': i_ids[:, 0]}

    def _target(self, pred):
        key = (tuple(pred.shape), pred.device)
        t = self._targets.get(key)
        if t is None:
            t = torch.zeros(pred.shape, dtype=torch.int64, device=pred.device)
            t[:, 0] = 1
            self._targets[key] = t
        return t

    def ctc_loss(self, out_dict):
        """context-target term (ContraRec.py:99-101): softmax cross-entropy of column 0 at temperature ctc_temp, on the engine's
        list-loss kernel (the reference's subtraction of the global maximum is a shift of every row)"""
        pred = out_dict['prediction']
        return self.ctc_temp * hnn.list_loss(pred / self.ctc_temp, self._target(pred), 1, _SOFTMAX_CE)

    def ccc_loss(self, out_dict):
        """context-context term (ContraRec.py:102,142-193) of the two augmented views"""
        view_a, view_b = out_dict['views']
        return hnn.contra_loss(view_a, view_b, out_dict['labels'], self.ccc_temp, workspace=self._workspace)

    def loss(self, out_dict):
        return self.ctc_loss(out_dict) + self.gamma * self.ccc_loss(out_dict)

    class Dataset(SequentialModel.Dataset):
        """the reference's augmentations (ContraRec.py:106-138) in numpy, drawing from np.random in its call order: the same seed
        gives the same views"""

        def _span(self, n):
            """how many of n positions an augmentation touches: one Beta(beta_a, beta_b) draw, rounded down"""
            return int(n * np.random.beta(a=self.model.beta_a, b=self.model.beta_b))

        def reorder_op(self, seq):
            """a window of the drawn span, at a uniformly drawn start, is permuted in place (draws: beta, randint, shuffle)"""
            n = len(seq)
            span = self._span(n)
            first = np.random.randint(0, n - span + 1)
            order = np.arange(n)
            np.random.shuffle(order[first:first + span])    # (a view: the window of `order` itself is shuffled)
            return seq[order]

        def mask_op(self, seq):
            """the drawn span of positions, chosen by shuffling a flag vector, becomes the mask token (draws: beta, shuffle)"""
            hit = np.arange(len(seq)) < self._span(len(seq))
            np.random.shuffle(hit)
            seq[hit] = self.model.mask_token
            return seq

        def augment(self, seq):
            """one uniform draw picks the operation: above 0.5 masking, else reordering; the input is left as it is"""
            view = np.array(seq).copy()
            return self.mask_op(view) if np.random.rand() > 0.5 else self.reorder_op(view)

        def _get_feed_dict(self, index):
            feed = super()._get_feed_dict(index)
            if self.phase == 'train':
                for suffix in ('a', 'b'):      # view a is drawn before view b
                    feed['history_items_' + suffix] = self.augment(feed['history_items'])
            return feed
