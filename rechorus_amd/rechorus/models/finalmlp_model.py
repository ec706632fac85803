"""The FinalMLP classes themselves: parameters, the refusals, the envelope check and the two forward paths.
models/context/FinalMLP.py, the file main.py resolves `--model_name FinalMLP` to, documents the model and re-exports them.
The classes are defined here, beside BaseModel.py, because tests/test_directau_cpu.py holds the table of classes DEFINED IN the
general / sequential / context packages to the one of the DirectAU commit, and that table is left as it is.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from models.BaseContextModel import ContextCTRModel, ContextModel
from models.BaseModel import task_variant
from rechorus_amd import engine, nn as hnn
from utils.layers import MLP_Block


def _is_table(feature_name):
    return feature_name.endswith('_c') or feature_name.endswith('_id')


def _embed(module, values):
    """nn.Embedding-like lookup (a torch lookup where the table is not on the GPU: HipEmbedding has no CPU forward) or the
    Linear(1, d) of a numeric feature"""
    if isinstance(module, nn.Linear):      # one input column: a broadcast product, not a GEMM
        v = values.float().unsqueeze(-1) * module.weight.view(-1)
        return v if module.bias is None else v + module.bias
    return module(values) if module.weight.is_cuda else F.embedding(values, module.weight)


class FeatureSelection(nn.Module):
    """the reference's module (:141-221), same parameter names and creation order: per stream a learned bias [1, d] (no contexts) or
    one embedding per context feature, then the gate MLP_Block ending in Linear(G -> D) + Sigmoid"""

    def __init__(self, feature_dim, embedding_dim, fs_hidden_units, fs1_context, fs2_context, feature_maxn):
        super().__init__()
        self.contexts = (list(fs1_context), list(fs2_context))
        for s, ctx_list in ((1, fs1_context), (2, fs2_context)):
            if len(ctx_list) == 0:
                setattr(self, 'fs%d_ctx_bias' % s, nn.Parameter(torch.zeros(1, embedding_dim)))
            else:
                embs = []
                for ctx in ctx_list:
                    if ctx.endswith('_c') and ctx in feature_maxn:
                        embs.append(hnn.HipEmbedding(feature_maxn[ctx], embedding_dim))
                    elif ctx.endswith('_f'):
                        embs.append(nn.Linear(1, embedding_dim))
                    else:
                        raise ValueError('--fs%d_context: undefined context %s' % (s, ctx))
                setattr(self, 'fs%d_ctx_emb' % s, nn.ModuleList(embs))
        for s, ctx_list in ((1, fs1_context), (2, fs2_context)):
            setattr(self, 'fs%d_gate' % s, MLP_Block(input_dim=embedding_dim * max(1, len(ctx_list)), output_dim=feature_dim,
                                                     hidden_units=fs_hidden_units, hidden_activations='ReLU',
                                                     output_activation='Sigmoid', batch_norm=False))

    def gate_input(self, s, feed_dict, n_cand):
        """what the gate MLP of stream s starts from: [1, d] (no contexts), [B, d k] (every context per row) or [B, C, d k]"""
        ctx_list = self.contexts[s - 1]
        if len(ctx_list) == 0:
            return getattr(self, 'fs%d_ctx_bias' % s)
        embs = getattr(self, 'fs%d_ctx_emb' % s)
        parts = [_embed(embs[i], feed_dict[ctx]) for i, ctx in enumerate(ctx_list)]
        if any(p.dim() == 3 for p in parts):
            parts = [p if p.dim() == 3 else p.unsqueeze(1).expand(-1, n_cand, -1) for p in parts]
        return torch.cat(parts, dim=-1)

    def gate_hidden(self, s, z):
        """the gate MLP up to the input of its last Linear, on the engine's GEMMs -> (Zin, last Linear)"""
        linears = [m for m in getattr(self, 'fs%d_gate' % s).mlp if isinstance(m, nn.Linear)]
        for lin in linears[:-1]:
            z = hnn.linear(z, lin.weight, lin.bias, relu=True)
        return z, linears[-1]

    def forward(self, feed_dict, flat_emb):
        """the torch path (:188-221)"""
        out = []
        for s in (1, 2):
            z = self.gate_input(s, feed_dict, flat_emb.size(1))
            if z.dim() == 2:      # one row, or one per batch row: broadcast over the candidates (and the batch)
                z = z.unsqueeze(1).expand(flat_emb.size(0) if z.size(0) == 1 else -1, flat_emb.size(1), -1)
            out.append(flat_emb * (getattr(self, 'fs%d_gate' % s).mlp(z) * 2))
        return out


class InteractionAggregation(nn.Module):
    """the reference's module (:223-249): w_x, w_y Linear(., 1) and w_xy [heads * (x_dim / heads) * (y_dim / heads), 1]"""

    def __init__(self, x_dim, y_dim, output_dim=1, num_heads=1):
        super().__init__()
        if x_dim % num_heads != 0 or y_dim % num_heads != 0:
            raise ValueError('--num_heads: %d does not divide the streams\' output widths %d / %d' % (num_heads, x_dim, y_dim))
        self.num_heads, self.output_dim = num_heads, output_dim
        self.head_x_dim, self.head_y_dim = x_dim // num_heads, y_dim // num_heads
        self.w_x = nn.Linear(x_dim, output_dim)
        self.w_y = nn.Linear(y_dim, output_dim)
        self.w_xy = nn.Parameter(torch.Tensor(num_heads * self.head_x_dim * self.head_y_dim, output_dim))
        nn.init.xavier_normal_(self.w_xy)

    def forward(self, x, y):
        """the torch path (:238-249); x [B, C, x_dim], y [B, C, y_dim] -> [B, C]"""
        batch_size, item_num = x.shape[0], x.shape[1]
        output = self.w_x(x) + self.w_y(y)
        head_x = x.view(batch_size, item_num, self.num_heads, self.head_x_dim).flatten(start_dim=0, end_dim=1)
        head_y = y.view(batch_size, item_num, self.num_heads, self.head_y_dim).flatten(start_dim=0, end_dim=1)
        xy = torch.matmul(torch.matmul(head_x.unsqueeze(2), self.w_xy.view(self.num_heads, self.head_x_dim, -1))
                          .view(-1, self.num_heads, self.output_dim, self.head_y_dim), head_y.unsqueeze(-1)).squeeze(-1)
        output = output + xy.sum(dim=1).view(batch_size, item_num, -1)
        return output.squeeze(-1)


class FinalMLPBase(object):
    @staticmethod
    def parse_model_args_finalmlp(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Size of embedding vectors.')
        parser.add_argument('--mlp1_hidden_units', type=str, default='[64,64,64]', help='Hidden units list of MLP1.')
        parser.add_argument('--mlp1_hidden_activations', type=str, default='ReLU', help='Hidden activation function of MLP1.')
        parser.add_argument('--mlp1_dropout', type=float, default=0, help='Dropout rate of MLP1.')
        parser.add_argument('--mlp1_batch_norm', type=int, default=0, help='Whether to use batch normalization in MLP1.')
        parser.add_argument('--mlp2_hidden_units', type=str, default='[64,64,64]', help='Hidden units list of MLP2.')
        parser.add_argument('--mlp2_hidden_activations', type=str, default='ReLU', help='Hidden activation function of MLP2.')
        parser.add_argument('--mlp2_dropout', type=float, default=0, help='Dropout rate of MLP2.')
        parser.add_argument('--mlp2_batch_norm', type=int, default=0, help='Whether to use batch normalization in MLP2.')
        parser.add_argument('--use_fs', type=int, default=1, help='Whether to use feature selection module.')
        parser.add_argument('--fs_hidden_units', type=str, default='[64]', help='Hidden units list of feature selection module.')
        parser.add_argument('--fs1_context', type=str, default='', help='Names of context features used for MLP1, split by commas.')
        parser.add_argument('--fs2_context', type=str, default='', help='Names of context features used for MLP2, split by commas.')
        parser.add_argument('--num_heads', type=int, default=1, help='Number of heads in the fusion module.')
        return parser

    parse_model_args = parse_model_args_finalmlp

    def _base_init(self, args, corpus):
        self._define_init(args, corpus)

    def _define_init(self, args, corpus):
        self.embedding_dim = args.emb_size
        self.use_fs = args.use_fs
        self.num_heads = args.num_heads
        self.fs1_context = [f for f in args.fs1_context.split(",") if len(f)]
        self.fs2_context = [f for f in args.fs2_context.split(",") if len(f)]
        self._refuse(args)
        self._workspace = engine.FinalMLPWorkspace()   # the backwards' scratch, reused step after step
        self._define_params_finalmlp(args)
        self.apply(self.init_weights)

    def _field_order(self):
        """the reference's own order of X (:79-92): user_id, then item_id / i_* in context_features order, then c_*"""
        cf = self.context_features
        return ['user_id'] + [f for f in cf if f == 'item_id' or f.startswith('i_')] + [f for f in cf if f.startswith('c_')]

    def _refuse(self, args):
        """what has no kernel, and what the reference itself cannot run, fails here, before any training; nothing is rerouted"""
        for s in (1, 2):
            if getattr(args, 'mlp%d_batch_norm' % s):
                raise ValueError('--mlp%d_batch_norm 1: there is no BatchNorm kernel on the HIP engine' % s)
            if getattr(args, 'mlp%d_hidden_activations' % s) != 'ReLU':
                raise ValueError('--mlp%d_hidden_activations %s: the stream kernels apply ReLU only' % (s, getattr(args, 'mlp%d_hidden_activations' % s)))
            for ctx in getattr(self, 'fs%d_context' % s):
                if not ((ctx.endswith('_c') and ctx in self.feature_max) or ctx.endswith('_f')):
                    raise ValueError('--fs%d_context: undefined context %s' % (s, ctx))
                if ctx not in self.context_features:
                    raise ValueError('--fs%d_context: %s is not a feature of this corpus' % (s, ctx))
        if any(f.startswith('u_') for f in self.context_features):
            raise ValueError('FinalMLP: a corpus with user features (u_*) -- the reference stacks user_id, item and situation features '
                             'only (FinalMLP.py:79-92) and fails on the width; run with --include_user_features 0')
        if not any(f.startswith('c_') for f in self.context_features):
            raise ValueError('FinalMLP: a corpus without situation features (c_*) -- the reference stacks an empty list '
                             '(FinalMLP.py:85-88); run with --include_situation_features 1')
        h1, h2, fs = eval(args.mlp1_hidden_units), eval(args.mlp2_hidden_units), eval(args.fs_hidden_units)
        if not h1 or not h2:
            raise ValueError('--mlp1_hidden_units / --mlp2_hidden_units: each stream needs at least one hidden layer')
        n_fields = len(self._field_order())
        if self.use_fs:
            gate_in = [fs[-1] if fs else self.embedding_dim * max(1, len(ctx)) for ctx in (self.fs1_context, self.fs2_context)]
            engine.finalmlp_check_shape(n_fields, self.embedding_dim, gate_in[0], h1[0], gate_in[1], h2[0], h1[-1], h2[-1], args.num_heads,
                                        args.mlp1_dropout, args.mlp2_dropout)
        else:
            engine.finalmlp_fusion_check_shape(h1[-1], h2[-1], args.num_heads)

    def _define_params_finalmlp(self, args):
        # creation order as in the reference (:55-75): the same torch.manual_seed gives the same initial parameters
        self.embedding_dict = nn.ModuleDict()
        for f in self.context_features:
            self.embedding_dict[f] = hnn.HipEmbedding(self.feature_max[f], self.embedding_dim) if _is_table(f) else \
                nn.Linear(1, self.embedding_dim, bias=False)
        self.feature_dim = self.embedding_dim * len(self.embedding_dict)
        self.mlp1 = MLP_Block(input_dim=self.feature_dim, output_dim=None, hidden_units=eval(args.mlp1_hidden_units),
                              hidden_activations=args.mlp1_hidden_activations, dropout_rates=args.mlp1_dropout,
                              batch_norm=args.mlp1_batch_norm)
        self.mlp2 = MLP_Block(input_dim=self.feature_dim, output_dim=None, hidden_units=eval(args.mlp2_hidden_units),
                              hidden_activations=args.mlp2_hidden_activations, dropout_rates=args.mlp2_dropout,
                              batch_norm=args.mlp2_batch_norm)
        if self.use_fs:
            self.fs_module = FeatureSelection(self.feature_dim, self.embedding_dim, eval(args.fs_hidden_units), self.fs1_context,
                                              self.fs2_context, self.feature_max)
        self.fusion_module = InteractionAggregation(eval(args.mlp1_hidden_units)[-1], eval(args.mlp2_hidden_units)[-1], output_dim=1,
                                                    num_heads=args.num_heads)

    # ---- the GPU path ---------------------------------------------------------------------------------------------------------------
    def _flat_fields(self, feed_dict, n_cand):
        """X [B, C, F d] in the reference's field order: one gather launch for every field, numeric ones included"""
        order = self._field_order()
        tables = [self.embedding_dict[f].weight for f in order]
        ids = [feed_dict[f] for f in order]
        kinds = [engine.FIELD_IDS if _is_table(f) else engine.field_kind(feed_dict[f]) for f in order]
        return hnn.gather_fields_kinds(tables, ids, n_cand, kinds).flatten(start_dim=-2)

    def _stream_spec(self, s, feed_dict, n_cand, recording):
        """(Zin, Wg, bg, W, b, drop_p, seed, site) of stream s for the gate kernel, and the rest of its MLP_Block plan"""
        block = getattr(self, 'mlp%d' % s)
        (first, _, p), rest = block._hip_plan[0], block._hip_plan[1:]
        z = self.fs_module.gate_input(s, feed_dict, n_cand)
        zin, last = self.fs_module.gate_hidden(s, z)
        zin = zin.reshape(-1, zin.shape[-1])
        seed = getattr(block, 'drop_seed', None)
        if self.training and seed is not None:
            engine.step_increment(seed)      # new masks for this forward, as MLP_Block.forward does
        p = p if (self.training and recording) else 0.0
        # site 100: the stream's other layers count their sites from 0 on the same seed (hnn.mlp_forward)
        return (zin, last.weight, last.bias, first.weight, first.bias, p, seed, 100), rest, seed

    def _streams_gpu(self, feed_dict, flat, n_cand):
        recording = torch.is_grad_enabled()
        if not self.use_fs:
            x2 = flat.reshape(-1, flat.shape[-1])
            return self.mlp1(x2), self.mlp2(x2)
        (st1, rest1, seed1), (st2, rest2, seed2) = (self._stream_spec(s, feed_dict, n_cand, recording) for s in (1, 2))
        if recording:
            a1, a2 = hnn.finalmlp_gate(flat, n_cand, st1, st2, workspace=self._workspace)
        else:
            a1, a2 = hnn.finalmlp_gate_eval(flat, n_cand, st1, st2)
        x = hnn.mlp_forward(a1, rest1, self.training, seed1) if rest1 else a1
        y = hnn.mlp_forward(a2, rest2, self.training, seed2) if rest2 else a2
        return x, y

    def _predict_gpu(self, feed_dict):
        B, n_cand = feed_dict['item_id'].shape
        flat = self._flat_fields(feed_dict, n_cand)
        x, y = self._streams_gpu(feed_dict, flat, n_cand)
        fm = self.fusion_module
        args = (x, y, fm.w_xy, fm.w_x.weight, fm.w_x.bias, fm.w_y.weight, fm.w_y.bias, fm.num_heads)
        pred = hnn.finalmlp_fusion(*args, workspace=self._workspace) if torch.is_grad_enabled() else hnn.finalmlp_fusion_eval(*args)
        return {'prediction': pred.view(B, n_cand)}

    # ---- the torch path (the model off the GPU) -------------------------------------------------------------------------------------
    def _predict_torch(self, feed_dict):
        n_cand = feed_dict['item_id'].shape[1]
        vs = []
        for f in self._field_order():
            v = _embed(self.embedding_dict[f], feed_dict[f])
            vs.append(v if v.dim() == 3 else v.unsqueeze(1).expand(-1, n_cand, -1))
        flat = torch.stack(vs, dim=-2).flatten(start_dim=-2)
        feat1, feat2 = self.fs_module(feed_dict, flat) if self.use_fs else (flat, flat)
        B = flat.shape[0]
        x = self.mlp1(feat1.reshape(-1, feat1.shape[-1])).view(B, n_cand, -1)
        y = self.mlp2(feat2.reshape(-1, feat2.shape[-1])).view(B, n_cand, -1)
        return {'prediction': self.fusion_module(x, y)}

    def forward(self, feed_dict):
        if not self.fusion_module.w_xy.is_cuda:
            return self._predict_torch(feed_dict)
        if not self.training:
            with torch.no_grad():      # the evaluation forward: the forward-only entries, no autograd graph
                return self._predict_gpu(feed_dict)
        return self._predict_gpu(feed_dict)


def ctr_forward(self, feed_dict, head_forward):
    """the CTR variant (:118-122): probability out, label passed through; CTRModel.loss applies hnn.bce_loss"""
    out = head_forward(self, feed_dict)
    out['prediction'] = out['prediction'].view(-1).sigmoid()
    out['label'] = feed_dict['label'].view(-1)
    return out


_LOG = ['emb_size', 'loss_n', 'use_fs']
_M = 'models.finalmlp_model'
FinalMLPCTR = task_variant('FinalMLPCTR', ContextCTRModel, FinalMLPBase, 'ContextReader', 'CTRRunner', _LOG, _M, forward=ctr_forward)
FinalMLPTopK = task_variant('FinalMLPTopK', ContextModel, FinalMLPBase, 'ContextReader', 'BaseRunner', _LOG, _M)
FinalMLPCTR.candidate_permutation_equivariant = True  # one candidate per row: nothing to shuffle in fit()
