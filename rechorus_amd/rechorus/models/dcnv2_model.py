"""The DCNv2 classes themselves: parameters, the envelope check, the two cross networks and the forward.
models/context/DCNv2.py, the file main.py resolves `--model_name DCNv2` to, documents the model and re-exports them.
The classes are defined here, beside BaseModel.py, because tests/test_directau_cpu.py holds the table of classes DEFINED IN the
general / sequential / context packages to the one of the DirectAU commit, and that table is left as it is (as models/autoint_model.py).
"""
import torch
import torch.nn as nn

from models.BaseContextModel import ContextCTRModel, ContextModel
from models.BaseModel import task_variant
from models.context.FM import is_categorical
from rechorus_amd import engine, nn as hnn
from utils.layers import MLP_Block


class DCNv2Base(object):
    @staticmethod
    def parse_model_args_DCNv2Base(parser):
        # the DCN parser (reference models/context/DCN.py:23-32) ...
        parser.add_argument('--emb_size', type=int, default=64, help='Size of embedding vectors.')
        parser.add_argument('--layers', type=str, default='[64]', help="Size of each deep layer.")
        parser.add_argument('--cross_layer_num', type=int, default=6, help="Number of cross layers.")
        parser.add_argument('--reg_weight', type=float, default=2.0,
                            help="Regularization weight for cross-layer weights. In DCNv2, it is only used for mixed version")
        # ... plus DCNv2's own flags (DCNv2.py:26-33)
        parser.add_argument('--mixed', type=int, default=1, help="Wether user mixed cross network or not.")
        parser.add_argument('--structure', type=str, default='parallel', help="cross network and DNN is 'parallel' or 'stacked'")
        parser.add_argument('--low_rank', type=int, default=64, help="Size for the low-rank architecture when mixed==1.")
        parser.add_argument('--expert_num', type=int, default=2,
                            help="Number of experts to calculate in each cross layer when mixed==1.")
        return parser

    parse_model_args = parse_model_args_DCNv2Base

    def _base_init(self, args, corpus):
        self._define_init(args, corpus)

    def _define_init(self, args, corpus):
        self.vec_size = args.emb_size
        self.reg_weight = args.reg_weight
        self.layers = eval(args.layers)
        self.cross_layer_num = args.cross_layer_num
        self.mixed, self.structure = args.mixed, args.structure
        self.expert_num, self.low_rank = args.expert_num, args.low_rank
        # what the kernels do not cover fails here, before any training; nothing is rerouted.  (The reference leaves predict_layer
        # undefined for any other --structure and fails in its first forward.)
        if self.structure not in ('parallel', 'stacked'):
            raise ValueError("DCNv2: --structure must be 'parallel' or 'stacked', got {!r}".format(self.structure))
        self.cross_width = len(self.feature_max) * self.vec_size
        if self.mixed:
            try:
                engine.dcnv2_check_shape(self.cross_width, self.low_rank, self.expert_num)
            except ValueError as e:
                raise ValueError('{} (--emb_size {} x {} fields, --low_rank {}, --expert_num {})'.format(
                    e, self.vec_size, len(self.feature_max), self.low_rank, self.expert_num)) from None
        self._workspace = engine.DCNv2Workspace()   # the backward's scratch, shared by the layers and reused step after step
        self._define_params_DCNv2()
        self.apply(self.init_weights)

    def _define_params_DCNv2(self):
        # creation order as in the reference (:46-77): the same torch.manual_seed gives the same initial parameters
        self.context_embedding = nn.ModuleDict()
        for f in self.context_features:
            self.context_embedding[f] = (hnn.HipEmbedding(self.feature_max[f], self.vec_size) if is_categorical(f)
                                         else nn.Linear(1, self.vec_size, bias=False))
        pre_size = self.cross_width
        n = self.cross_layer_num
        if self.mixed:
            self.cross_layer_u = nn.ParameterList(nn.Parameter(torch.randn(self.expert_num, pre_size, self.low_rank)) for _ in range(n))
            self.cross_layer_v = nn.ParameterList(nn.Parameter(torch.randn(self.expert_num, pre_size, self.low_rank)) for _ in range(n))
            self.cross_layer_c = nn.ParameterList(nn.Parameter(torch.randn(self.expert_num, self.low_rank, self.low_rank))
                                                  for _ in range(n))
            self.gating = nn.ModuleList(nn.Linear(pre_size, 1) for _ in range(self.expert_num))
        else:
            self.cross_layer_w2 = nn.ParameterList(nn.Parameter(torch.randn(pre_size, pre_size)) for _ in range(n))
        self.bias = nn.ParameterList(nn.Parameter(torch.zeros(pre_size, 1)) for _ in range(n))
        self.deep_layers = MLP_Block(pre_size, self.layers, hidden_activations="ReLU", batch_norm=True, norm_before_activation=True,
                                     dropout_rates=self.dropout, output_dim=None)
        if self.structure == 'parallel':
            self.predict_layer = nn.Linear(pre_size + self.layers[-1], 1)
        else:
            self.predict_layer = nn.Linear(self.layers[-1], 1)

    def _fields(self, feed_dict, n_cand):
        """[B, n_cand, F, d]: ONE gather launch for every field, numeric ones included (as models/din_model.py:_fields)"""
        names = self.context_features
        ids = [feed_dict[f] for f in names]
        kinds = [engine.FIELD_IDS if is_categorical(f) else engine.field_kind(x) for f, x in zip(names, ids)]
        return hnn.gather_fields_kinds([self.context_embedding[f].weight for f in names], ids, n_cand, kinds)

    def gate_params(self):
        """(Wg [E, D], bg [E]): the experts' gating Linears stacked; ONE gate serves every layer (:62)"""
        return (torch.cat([m.weight for m in self.gating], dim=0), torch.cat([m.bias for m in self.gating], dim=0))

    def cross_layers(self, x_0):
        """[N, D] -> every layer's x_l, [N, D] each"""
        outs, x_l = [], x_0
        if self.mixed:      # cross_net_mix (:96-144): one node per layer
            Wg, bg = self.gate_params()
            for l in range(self.cross_layer_num):
                args = (x_0, x_l, self.cross_layer_u[l], self.cross_layer_v[l], self.cross_layer_c[l], self.bias[l], Wg, bg)
                x_l = hnn.dcnv2_mix_layer(*args, self._workspace) if torch.is_grad_enabled() else hnn.dcnv2_mix_layer_eval(*args)
                outs.append(x_l)
        else:               # cross_net_2 (:79-94): W_l x_l + b_l on the fp32 MFMA dense layer, the rest in torch ops
            for l in range(self.cross_layer_num):
                x_l = x_0 * hnn.linear(x_l, self.cross_layer_w2[l], self.bias[l].view(-1)) + x_l
                outs.append(x_l)
        return outs

    def forward(self, feed_dict):
        if not self.predict_layer.weight.is_cuda:
            raise RuntimeError('DCNv2 runs on the GPU only (the cross network has no CPU path)')
        if not self.training:
            with torch.no_grad():      # the evaluation forward: the forward-only layer entry, no autograd graph
                return self._predict(feed_dict)
        return self._predict(feed_dict)

    def _predict(self, feed_dict):
        B, C = feed_dict['item_id'].shape
        x_0 = self._fields(feed_dict, C).reshape(B * C, self.cross_width)
        cross = self.cross_layers(x_0)[-1] if self.cross_layer_num > 0 else x_0
        if self.structure == 'parallel':
            out = self.predict_layer(torch.cat([cross, self.deep_layers(x_0)], dim=-1))
        else:
            out = self.predict_layer(self.deep_layers(cross))
        return {'prediction': out.view(B, C)}


def dcnv2_ctr_forward(self, feed_dict, head_forward):
    """one candidate per row, probability out, label passed through (reference :186-190)"""
    out = head_forward(self, feed_dict)
    out['prediction'] = out['prediction'].view(-1).sigmoid()
    out['label'] = feed_dict['label'].view(-1)
    return out


def _loss_with_reg(task_base):
    def loss(self, out_dict):
        """the task's loss; with --mixed 0 plus reg_weight * sum_l ||W_l||_2 -- the norm, not its square (:192-198, DCN.py:99-111)"""
        ls = task_base.loss(self, out_dict)
        if not self.mixed:
            reg = None
            for W in self.cross_layer_w2:
                reg = W.norm(2) if reg is None else reg + W.norm(2)
            ls = ls + self.reg_weight * reg
        return ls
    return loss


_LOG = ['emb_size', 'loss_n', 'cross_layer_num']
_M = 'models.dcnv2_model'
# the reference's DCNv2CTR chains ContextCTRModel's parser (:177-180), so --loss_n defaults to 'BCE' there
DCNv2CTR = task_variant('DCNv2CTR', ContextCTRModel, DCNv2Base, 'ContextReader', 'CTRRunner', _LOG, _M, forward=dcnv2_ctr_forward)
DCNv2TopK = task_variant('DCNv2TopK', ContextModel, DCNv2Base, 'ContextReader', 'BaseRunner', _LOG, _M)
DCNv2CTR.loss = _loss_with_reg(ContextCTRModel)
DCNv2TopK.loss = _loss_with_reg(ContextModel)
DCNv2CTR.candidate_permutation_equivariant = True  # one candidate per row: nothing to shuffle in fit()
