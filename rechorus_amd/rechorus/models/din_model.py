"""The DIN classes themselves: parameters, the envelope check and the forward.
models/context_seq/DIN.py, the file main.py resolves `--model_name DIN` to, documents the model and re-exports them.
The classes are defined here, beside BaseModel.py, because tests/test_directau_cpu.py holds the table of classes DEFINED IN the
model packages to the one of the DirectAU commit, and that table is left as it is (as models/cfkg_model.py).
"""
import torch
import torch.nn as nn

from models.BaseContextModel import ContextSeqCTRModel, ContextSeqModel
from models.BaseModel import task_variant
from models.context.FM import is_categorical
from rechorus_amd import engine, nn as hnn
from utils.layers import MLP_Block


class DINBase(object):
    @staticmethod
    def parse_model_args_din(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Size of embedding vectors.')
        parser.add_argument('--att_layers', type=str, default='[64]', help="Size of each layer in the attention module.")
        parser.add_argument('--dnn_layers', type=str, default='[64]', help="Size of each layer in the MLP module.")
        return parser

    parse_model_args = parse_model_args_din

    def _base_init(self, args, corpus):
        self._define_init(args, corpus)

    def _define_init(self, args, corpus):
        self.user_context = ['user_id'] + corpus.user_feature_names
        self.item_context = ['item_id'] + corpus.item_feature_names
        self.situation_context = corpus.situation_feature_names
        self.item_feature_num = len(self.item_context)
        self.user_feature_num = len(self.user_context)
        self.situation_feature_num = len(corpus.situation_feature_names) if self.add_historical_situations else 0
        self.vec_size = args.emb_size
        self.att_layers = eval(args.att_layers)
        self.dnn_layers = eval(args.dnn_layers)
        # a flag combination the attention kernels do not cover fails here, before any training; nothing is rerouted
        if not 1 <= self.history_max <= 64:
            raise ValueError('DIN on the HIP engine: --history_max {} outside [1, 64]'.format(self.history_max))
        self.att_width = (self.item_feature_num + self.situation_feature_num) * self.vec_size
        try:
            engine.din_check_shape(self.att_width, self.history_max, self.att_layers, self.dropout)
        except ValueError as e:
            raise ValueError('{} (--emb_size {} x {} attended fields, --att_layers {}, --dropout {})'.format(
                e, self.vec_size, self.item_feature_num + self.situation_feature_num, args.att_layers, self.dropout)) from None
        self._define_params_DIN()
        self.apply(self.init_weights)

    def _define_params_DIN(self):
        # creation order as in the reference (:47-61): the same torch.manual_seed gives the same initial parameters
        self.embedding_dict = nn.ModuleDict()
        for f in self.user_context + self.item_context + self.situation_context:
            self.embedding_dict[f] = (hnn.HipEmbedding(self.feature_max[f], self.vec_size) if is_categorical(f)
                                      else nn.Linear(1, self.vec_size, bias=False))
        self.att_mlp_layers = MLP_Block(input_dim=4 * self.att_width, hidden_units=self.att_layers, output_dim=1,
                                        hidden_activations='Sigmoid', dropout_rates=self.dropout, batch_norm=False)
        pre_size = (2 * (self.item_feature_num + self.situation_feature_num) + self.item_feature_num
                    + len(self.situation_context) + self.user_feature_num) * self.vec_size
        self.dnn_mlp_layers = MLP_Block(input_dim=pre_size, hidden_units=self.dnn_layers, output_dim=1,
                                        hidden_activations='Dice', dropout_rates=self.dropout, batch_norm=True,
                                        norm_before_activation=True)
        if self.dropout > 0:      # key of the attention's dropout mask stream; not a parameter and not in the state_dict
            self.register_buffer('att_drop_seed', hnn.fresh_drop_seed(), persistent=False)

    def _fields(self, names, feed_dict, n_cand, prefix=''):
        """[B, n_cand, len(names), d]: ONE gather launch for the named fields, numeric ones included (ids [B] are broadcast over
        the candidate slot; the history is a gather with L in that slot)"""
        ids = [feed_dict[prefix + f] for f in names]
        kinds = [engine.FIELD_IDS if is_categorical(f) else engine.field_kind(x) for f, x in zip(names, ids)]
        return hnn.gather_fields_kinds([self.embedding_dict[f].weight for f in names], ids, n_cand, kinds)

    def attention_params(self):
        """[(W_1, b_1), ..., (w_out, b_out)]: the Linear layers of att_mlp_layers in order"""
        return [(m.weight, m.bias) for m in self.att_mlp_layers.mlp if isinstance(m, nn.Linear)]

    def attention(self, current, history, lengths, n_cand):
        """DIN.py:63-95 for q [B * C, H] over keys [B, L, H] as one node (rechorus_amd.nn.din_attention) -> (out, weights)"""
        p, seed = (self.dropout, self.att_drop_seed) if (self.training and self.dropout > 0) else (0.0, None)
        if seed is not None:
            engine.step_increment(seed)      # a new mask for this forward; the node keeps the value for its backward
        return hnn.din_attention(current, history, lengths, n_cand, self.attention_params(), p, seed)

    def forward(self, feed_dict):
        if not self.dnn_mlp_layers.mlp[0].weight.is_cuda:
            raise RuntimeError('DIN runs on the GPU only (the attention has no CPU path)')
        B, C = feed_dict['item_id'].shape
        L = feed_dict['history_item_id'].shape[1]
        attended = self.item_context + (self.situation_context if self.situation_feature_num else [])
        history = self._fields(attended, feed_dict, L, prefix='history_')                   # [B, L, Fa, d]
        all_context = self._fields(self.item_context + self.user_context + self.situation_context, feed_dict, C)
        if self.situation_feature_num:
            current = self._fields(attended, feed_dict, C)                                   # [B, C, Fa, d]
        else:
            current = all_context[:, :, :self.item_feature_num]
        q = current.reshape(B * C, self.att_width)
        out, _ = self.attention(q, history.reshape(B, L, self.att_width), feed_dict['lengths'], C)
        din_output = torch.cat([out, out * q, all_context.reshape(B * C, -1)], dim=-1)      # [B * C, .]: rows of instances only
        return {'prediction': self.dnn_mlp_layers(din_output).squeeze(dim=-1).view(B, C)}


def din_ctr_forward(self, feed_dict, head_forward):
    """one candidate per row, probability out, label passed through (reference :177-181)"""
    out = head_forward(self, feed_dict)
    out['prediction'] = out['prediction'].view(-1).sigmoid()
    out['label'] = feed_dict['label'].view(-1)
    return out


_LOG = ['emb_size', 'att_layers', 'add_historical_situations']
_M = 'models.din_model'
DINCTR = task_variant('DINCTR', ContextSeqCTRModel, DINBase, 'ContextSeqReader', 'CTRRunner', _LOG, _M, forward=din_ctr_forward)
DINTopK = task_variant('DINTopK', ContextSeqModel, DINBase, 'ContextSeqReader', 'BaseRunner', _LOG, _M)
DINCTR.candidate_permutation_equivariant = True  # one candidate per row: nothing to shuffle in fit()
