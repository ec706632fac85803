"""SetRank's class bodies (models/reranker/SetRank.py, SetRankGeneral.py and SetRankSequential.py re-export them; reference
models/reranker/SetRank.py:58-188).

x_i = rFF0([i_emb | u_v | i_v]) + ordinal_position_embedding[position] over the slots of an impression list (the position is added
AFTER rFF0, so its table has width num_hidden_unit: SetRank.py:104, :118, :144-145), `n_blocks` permutation-aware blocks under the
key-padding mask, rFF1 to one score per slot.  --setrank_type MSAB: a block is one post-norm self-attention block, ONE autograd node on
the list-encoder kernels (rechorus_amd.nn.list_encoder_block, as PRM's).  --setrank_type IMSAB (the default): a block is
h = MAB1(I, x, x; mask), x' = MAB2(x, h, h) with I [20, num_hidden_unit] learned inducing points shared by every list, TWO nodes on the
set-attention kernels (rechorus_amd.nn.induced_set_block).  The MabParams / MsabParams / ImsabParams modules hold the parameters under
the reference's state_dict keys (encoder.{k}.MAB1.attn.in_proj_weight, ..., encoder.{k}.I) and are never called.
"""
import torch
import torch.nn as nn

from models.BaseRerankerModel import RerankModel, RerankSeqModel
from rechorus_amd import engine, nn as hnn

FEED_FORWARD = 128      # the reference hard-codes d_feedforward=128 (SetRank.py:121, :123)
M_CLUSTERS = 20         # and m_clusters=20 (SetRank.py:123)
SETRANK_TYPES = ('MSAB', 'IMSAB')


class MabParams(nn.Module):
    """the parameters of one MAB, created in the reference's order (SetRank.py:32-38); never called"""

    def __init__(self, d_model, nhead, d_feedforward):
        super().__init__()
        self.attn = nn.MultiheadAttention(embed_dim=d_model, num_heads=nhead, dropout=0.0)
        self.linear1 = nn.Linear(d_model, d_feedforward)
        self.linear2 = nn.Linear(d_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)

    def weights(self):
        """the twelve tensors in engine.LISTENC_WEIGHTS order"""
        a = self.attn
        return [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, self.norm1.weight, self.norm1.bias,
                self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias, self.norm2.weight, self.norm2.bias]


class MsabParams(nn.Module):
    def __init__(self, d_model, nhead, d_feedforward):
        super().__init__()
        self.MAB1 = MabParams(d_model, nhead, d_feedforward)


class ImsabParams(nn.Module):
    def __init__(self, d_model, nhead, d_feedforward, m_clusters):
        super().__init__()
        self.MAB1 = MabParams(d_model, nhead, d_feedforward)
        self.MAB2 = MabParams(d_model, nhead, d_feedforward)
        # drawn here, inside the constructor, after both blocks (SetRank.py:72-73); init_weights leaves it alone (neither a Linear
        # nor an Embedding)
        self.I = nn.Parameter(torch.empty(m_clusters, d_model))
        nn.init.normal_(self.I, mean=0.0, std=0.01)


class SetRankBase(object):
    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Size of item embedding vectors.')
        parser.add_argument('--n_blocks', type=int, default=4, help='num of blocks of MSAB/IMSAB')
        parser.add_argument('--num_heads', type=int, default=4, help='Number of attention heads.')
        parser.add_argument('--num_hidden_unit', type=int, default=64, help='Number of hidden units in Transformer layer.')
        parser.add_argument('--setrank_type', type=str, default='IMSAB', help='MSAB or IMSAB')
        return parser

    def _base_init(self, args, corpus):
        self.args = args
        self.emb_size, self.n_blocks = args.emb_size, args.n_blocks
        self.num_heads, self.num_hidden_unit = args.num_heads, args.num_hidden_unit
        self.setrank_type = args.setrank_type
        self.list_len = self.train_max_pos_item + self.train_max_neg_item
        if self.setrank_type not in SETRANK_TYPES:
            raise ValueError('SetRank: --setrank_type must be MSAB or IMSAB, got {!r}'.format(self.setrank_type))
        if float(self.dropout) > 0:
            raise ValueError('SetRank on the HIP engine: --dropout {} is not supported (every attention block has four dropout sites '
                             'and no mask stream is built for them); use --dropout 0'.format(self.dropout))
        if self.n_blocks < 1:
            raise ValueError('SetRank: --n_blocks must be at least 1, got {}'.format(self.n_blocks))
        d, H, n = self.num_hidden_unit, self.num_heads, self.list_len      # ValueError with the library's reason
        if self.setrank_type == 'MSAB':
            engine.listenc_check_shape(n, d, H, FEED_FORWARD)
            self._workspace = engine.ListEncWorkspace()
        else:
            engine.setmab_check_shape(M_CLUSTERS, n, d, H, FEED_FORWARD)
            engine.setmab_check_shape(n, M_CLUSTERS, d, H, FEED_FORWARD)
            self._workspace = engine.SetMabWorkspace()
        self.corpus = corpus
        self._base_define_params()
        self.apply(self.init_weights)      # (reaches the ranker too, as in the reference: its checkpoint is loaded again below)
        self.restore_ranker()

    def _base_define_params(self):
        d = self.num_hidden_unit
        self.i_embeddings = hnn.HipEmbedding(self.item_num, self.emb_size)
        self.ordinal_position_embedding = hnn.HipEmbedding(self.list_len, d)
        self.rFF0 = nn.Linear(self.emb_size + 2 * self.ranker_emb_size, d, bias=True)
        if self.setrank_type == 'MSAB':
            self.encoder = nn.ModuleList([MsabParams(d, self.num_heads, FEED_FORWARD) for _ in range(self.n_blocks)])
        else:
            self.encoder = nn.ModuleList([ImsabParams(d, self.num_heads, FEED_FORWARD, M_CLUSTERS) for _ in range(self.n_blocks)])
        self.rFF1 = nn.Linear(d, 1, bias=True)

    def _block(self, blk, x, pad, grad):
        H = self.num_heads
        if self.setrank_type == 'MSAB':
            w = blk.MAB1.weights()
            return hnn.list_encoder_block(x, pad, w, H, self._workspace) if grad else hnn.list_encoder_block_eval(x, pad, w, H)
        w1, w2 = blk.MAB1.weights(), blk.MAB2.weights()
        return (hnn.induced_set_block(x, pad, blk.I, w1, w2, H, self._workspace) if grad
                else hnn.induced_set_block_eval(x, pad, blk.I, w1, w2, H))

    def encode(self, feed_dict):
        """[x_0, x_1, ..., x_n_blocks], each [batch, slots, num_hidden_unit]: the input stage's output and every block's"""
        i_ids = feed_dict['item_id']
        if i_ids.shape[1] != self.list_len:
            raise ValueError('SetRank: lists of {} slots, the model was built for {}'.format(i_ids.shape[1], self.list_len))
        di = torch.cat((self.i_embeddings(i_ids), feed_dict['u_v'], feed_dict['i_v']), dim=2)
        xi = hnn.linear(di, self.rFF0.weight, self.rFF0.bias).view(i_ids.shape[0], self.list_len, -1)
        xs, pad = [xi + self.ordinal_position_embedding(feed_dict['position'])], feed_dict['padding_mask']
        grad = torch.is_grad_enabled()
        for blk in self.encoder:
            xs.append(self._block(blk, xs[-1], pad, grad))
        return xs

    def forward(self, feed_dict):
        self.check_list = []
        batch_size = feed_dict['item_id'].shape[0]
        prediction = hnn.linear(self.encode(feed_dict)[-1], self.rFF1.weight, self.rFF1.bias)
        return {'prediction': prediction.view(batch_size, -1)}


def _variant(name, task_base, reader, doc):
    def parse_model_args(parser):
        return task_base.parse_model_args(SetRankBase.parse_model_args(parser))

    def __init__(self, args, corpus):
        task_base.__init__(self, args, corpus)
        self._base_init(args, corpus)

    def forward(self, feed_dict):
        return SetRankBase.forward(self, feed_dict)
    body = dict(reader=reader, runner='ImpressionRunner', extra_log_args=['tuneranker', 'setrank_type'], __init__=__init__,
                forward=forward, parse_model_args=staticmethod(parse_model_args), __module__=__name__, __doc__=doc)
    return type(name, (task_base, SetRankBase), body)


SetRankGeneral = _variant('SetRankGeneral', RerankModel, 'ImpressionReader', 'SetRank over the lists of a general base ranker (BPRMF)')
SetRankSequential = _variant('SetRankSequential', RerankSeqModel, 'ImpressionSeqReader',
                             'SetRank over the lists of a sequential base ranker (SASRec)')
