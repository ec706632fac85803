"""PRM's class bodies (models/reranker/PRM.py re-exports them; reference models/reranker/PRM.py:31-128).

x_i = rFF0([i_emb | u_v | i_v] + ordinal_position_embedding[position]) over the slots of an impression list, `n_blocks` post-norm
encoder blocks under the key-padding mask, rFF1 to one score per slot.  Each block is ONE autograd node on the list-encoder kernels
(rechorus_amd.nn.list_encoder_block: one forward launch; the backward recomputes the block and keeps the weight-gradient partials on
chip at the default width).  The nn.TransformerEncoderLayer modules hold the parameters under the reference's state_dict keys and
are never called.  The input stage (two HipEmbedding gathers, torch cat and +, rFF0) and rFF1 are composed from the existing nodes.
"""
import torch
import torch.nn as nn

from models.BaseRerankerModel import RerankModel, RerankSeqModel
from rechorus_amd import engine, nn as hnn

FEED_FORWARD = 128      # the reference hard-codes dim_feedforward=128 (PRM.py:64)


def block_weights(layer):
    """the twelve tensors of one nn.TransformerEncoderLayer in engine.LISTENC_WEIGHTS order"""
    a = layer.self_attn
    return [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, layer.norm1.weight, layer.norm1.bias,
            layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, layer.norm2.weight, layer.norm2.bias]


class PRMBase(object):
    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Size of item embedding vectors.')
        parser.add_argument('--n_blocks', type=int, default=4, help='num of blocks of MSAB/IMSAB')
        parser.add_argument('--num_heads', type=int, default=4, help='Number of attention heads.')
        parser.add_argument('--num_hidden_unit', type=int, default=64, help='Number of hidden units in Transformer layer.')
        return parser

    def _base_init(self, args, corpus):
        self.args = args
        self.emb_size, self.n_blocks = args.emb_size, args.n_blocks
        self.num_heads, self.num_hidden_unit = args.num_heads, args.num_hidden_unit
        self.list_len = self.train_max_pos_item + self.train_max_neg_item
        if float(self.dropout) > 0:
            raise ValueError('PRM on the HIP engine: --dropout {} is not supported (the encoder block has four dropout sites and no '
                             'mask stream is built for them); use --dropout 0'.format(self.dropout))
        if self.n_blocks < 1:
            raise ValueError('PRM: --n_blocks must be at least 1, got {}'.format(self.n_blocks))
        engine.listenc_check_shape(self.list_len, self.num_hidden_unit, self.num_heads, FEED_FORWARD)      # ValueError with the reason
        self.corpus = corpus
        self._workspace = engine.ListEncWorkspace()
        self._base_define_params()
        self.apply(self.init_weights)      # (reaches the ranker too, as in the reference: its checkpoint is loaded again below)
        self.restore_ranker()

    def _base_define_params(self):
        width = self.emb_size + 2 * self.ranker_emb_size
        self.i_embeddings = hnn.HipEmbedding(self.item_num, self.emb_size)
        self.ordinal_position_embedding = hnn.HipEmbedding(self.list_len, width)
        self.rFF0 = nn.Linear(width, self.num_hidden_unit, bias=True)
        self.encoder = nn.ModuleList([nn.TransformerEncoderLayer(d_model=self.num_hidden_unit, nhead=self.num_heads,
                                                                 dim_feedforward=FEED_FORWARD, dropout=0.0)
                                      for _ in range(self.n_blocks)])
        self.rFF1 = nn.Linear(self.num_hidden_unit, 1, bias=True)

    def encode(self, feed_dict):
        """[x_0, x_1, ..., x_n_blocks], each [batch, slots, num_hidden_unit]: rFF0's output and every block's"""
        i_ids = feed_dict['item_id']
        if i_ids.shape[1] != self.list_len:
            raise ValueError('PRM: lists of {} slots, the model was built for {}'.format(i_ids.shape[1], self.list_len))
        di = torch.cat((self.i_embeddings(i_ids), feed_dict['u_v'], feed_dict['i_v']), dim=2)
        xi = hnn.linear(di + self.ordinal_position_embedding(feed_dict['position']), self.rFF0.weight, self.rFF0.bias)
        xs, pad = [xi.view(i_ids.shape[0], self.list_len, -1)], feed_dict['padding_mask']
        grad = torch.is_grad_enabled()
        for layer in self.encoder:
            w = block_weights(layer)
            xs.append(hnn.list_encoder_block(xs[-1], pad, w, self.num_heads, self._workspace) if grad
                      else hnn.list_encoder_block_eval(xs[-1], pad, w, self.num_heads))
        return xs

    def forward(self, feed_dict):
        self.check_list = []
        batch_size = feed_dict['item_id'].shape[0]
        prediction = hnn.linear(self.encode(feed_dict)[-1], self.rFF1.weight, self.rFF1.bias)
        return {'prediction': prediction.view(batch_size, -1)}


def _variant(name, task_base, reader, doc):
    def parse_model_args(parser):
        return task_base.parse_model_args(PRMBase.parse_model_args(parser))

    def __init__(self, args, corpus):
        task_base.__init__(self, args, corpus)
        self._base_init(args, corpus)

    def forward(self, feed_dict):
        return PRMBase.forward(self, feed_dict)
    body = dict(reader=reader, runner='ImpressionRunner', extra_log_args=['tuneranker'], __init__=__init__, forward=forward,
                parse_model_args=staticmethod(parse_model_args), __module__=__name__, __doc__=doc)
    return type(name, (task_base, PRMBase), body)


PRMGeneral = _variant('PRMGeneral', RerankModel, 'ImpressionReader', 'PRM over the lists of a general base ranker (BPRMF)')
PRMSequential = _variant('PRMSequential', RerankSeqModel, 'ImpressionSeqReader', 'PRM over the lists of a sequential base ranker (SASRec)')
