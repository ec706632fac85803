"""The AutoInt classes themselves: parameters, the envelope check and the two forward paths.
models/context/AutoInt.py, the file main.py resolves `--model_name AutoInt` to, documents the model and re-exports them.
The classes are defined here, beside BaseModel.py, because tests/test_directau_cpu.py holds the table of classes DEFINED IN the
general / sequential / context packages to the one of the DirectAU commit, and that table is left as it is.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from models.BaseContextModel import ContextCTRModel, ContextModel
from models.BaseModel import task_variant
from models.context.FM import FMBase, ctr_forward, is_categorical
from rechorus_amd import engine, nn as hnn
from utils.layers import MLP_Block, MultiHeadAttention


class AutoIntBase(FMBase):
    fm_term = False      # the head adds the tower's term only; the gather forms no pairwise term

    @staticmethod
    def parse_model_args_AutoInt(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Size of embedding vectors.')
        parser.add_argument('--attention_size', type=int, default=32, help='Size of attention hidden space.')
        parser.add_argument('--num_heads', type=int, default=1, help='Number of attention heads.')
        parser.add_argument('--num_layers', type=int, default=1, help='Number of self-attention layers.')
        parser.add_argument('--layers', type=str, default='[64]', help="Size of each layer.")
        return parser

    parse_model_args = parse_model_args_AutoInt

    def _base_init(self, args, corpus):
        self._define_init(args, corpus)

    def _define_init(self, args, corpus):
        self.vec_size = args.emb_size
        self.layers = eval(args.layers)
        self.num_heads, self.num_layers, self.attention_size = args.num_heads, args.num_layers, args.attention_size
        # a flag combination the kernels do not cover fails here, before any training; nothing is rerouted
        width = self.vec_size
        for _ in range(self.num_layers):
            engine.autoint_check_shape(len(self.context_features), width, self.attention_size, self.num_heads)
            width = self.attention_size
        self._workspace = engine.AutoIntWorkspace()   # the backward's scratch, shared by the layers and reused step after step
        self._define_params_AutoInt()
        self.apply(self.init_weights)

    def _define_params_AutoInt(self):
        # creation order as in the reference (:49-66): the same torch.manual_seed gives the same initial parameters
        self._define_params_FM()
        att_input = self.vec_size
        attentions, residuals = [], []
        for _ in range(self.num_layers):
            attentions.append(MultiHeadAttention(d_model=att_input, n_heads=self.num_heads, kq_same=False, bias=False,
                                                 attention_d=self.attention_size))
            residuals.append(nn.Linear(att_input, self.attention_size))
            att_input = self.attention_size
        self.autoint_attentions = nn.ModuleList(attentions)
        self.residual_embeddings = nn.ModuleList(residuals)
        pre_size = len(self.feature_max) * self.attention_size      # the reference's expression (:64): = F * A for ContextReader
        self.deep_layers = MLP_Block(pre_size, self.layers, hidden_activations="ReLU", dropout_rates=self.dropout, output_dim=1)

    def _early_seed(self):
        # as WideDeep: the tower's dropout seed is bumped by the gather's launch inside a whole training step
        return getattr(self.deep_layers, 'drop_seed', None) if (self.training and self._rows_opt() is not None) else None

    def _lookup(self, tables, feed_dict, n_cand):
        """FMBase._lookup with a torch lookup where the tables are not on the GPU (HipEmbedding has no CPU forward)"""
        out = []
        for f in self.context_features:
            x = feed_dict[f]
            if is_categorical(f):
                v = tables[f](x) if tables[f].weight.is_cuda else F.embedding(x, tables[f].weight)
            else:
                v = tables[f](x.float().unsqueeze(-1))
            out.append(v if v.dim() == 3 else v.unsqueeze(-2).expand(-1, n_cand, -1))
        return out

    def interacting_layers(self, x):
        """[B, C, F, d] -> the outputs of every layer, [B, C, F, A] each (:72-75)"""
        outs = []
        fused = hnn.autoint_layer if torch.is_grad_enabled() else hnn.autoint_layer_eval
        for att, res in zip(self.autoint_attentions, self.residual_embeddings):
            if x.is_cuda:
                args = (x, att.q_linear.weight, att.k_linear.weight, att.v_linear.weight, res.weight, res.bias, self.num_heads)
                x = fused(*args, self._workspace) if fused is hnn.autoint_layer else fused(*args)
            else:
                x = (att(x, x, x) + res(x)).relu()
            outs.append(x)
        return outs

    def _deep(self, field_vectors):
        x = self.interacting_layers(field_vectors)[-1] if self.num_layers > 0 else field_vectors
        return self.deep_layers(x.flatten(start_dim=-2)).squeeze(dim=-1)

    def _head_terms(self, field_vectors, fm=None):
        return [self._deep(field_vectors)]

    def _predict(self, feed_dict):
        field_vectors, first_order = self._get_embeddings_FM(feed_dict)
        return {'prediction': first_order + self._deep(field_vectors)}

    def forward(self, feed_dict):
        if self.overall_bias.is_cuda and not self.training:
            with torch.no_grad():      # the evaluation forward: the forward-only layer entry, no autograd graph
                return self._predict(feed_dict)
        return self._predict(feed_dict)


_LOG = ['emb_size', 'layers', 'num_layers', 'num_heads', 'loss_n']
_M = 'models.autoint_model'
# the reference's AutoIntCTR chains ContextCTRModel's parser (:86-89), so --loss_n defaults to 'BCE' here (WideDeepCTR / DeepFMCTR
# chain ContextModel's and default to 'BPR': that quirk is theirs alone)
AutoIntCTR = task_variant('AutoIntCTR', ContextCTRModel, AutoIntBase, 'ContextReader', 'CTRRunner', _LOG, _M, forward=ctr_forward)
AutoIntTopK = task_variant('AutoIntTopK', ContextModel, AutoIntBase, 'ContextReader', 'BaseRunner', _LOG, _M)
AutoIntCTR.candidate_permutation_equivariant = True  # one candidate per row: nothing to shuffle in fit()
