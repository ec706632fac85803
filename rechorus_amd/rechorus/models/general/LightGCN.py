""" LightGCN on the HIP engine
Reference: "LightGCN: Simplifying and Powering Graph Convolution Network for Recommendation", He et al., SIGIR'2020.
Counterpart of the reference's models/general/LightGCN.py (same class / flag / state_dict names), e.g.
    python main.py --model_name LightGCN --emb_size 64 --n_layers 3 --lr 1e-3 --l2 1e-8 --dataset Grocery_and_Gourmet_Food
    python main.py --model_name LightGCN --model_mode Impression --loss_n BPR --dataset MINDCTR ...
The normalised adjacency (:23-53) is built once with vectorised numpy as CSR and a propagation plan (rechorus_amd/lgcn.py), kept
as non-persistent buffers, so checkpoints interchange with the reference's.  The encoder's propagation (:137-151: torch.cat,
L sparse-dense products, stack, mean) is rc_lgcn_propagate_fwd, its autograd rc_lgcn_propagate_bwd; scores and loss are BPRMF's
kernels on the propagated tables.  In evaluation the propagated tables are computed once per pass and reused by every batch
(the reference recomputes the whole graph for each one; the numbers are the same).
"""
import torch
import torch.nn as nn

from models.BaseImpressionModel import ImpressionModel
from models.BaseModel import GeneralModel, task_variant
from rechorus_amd import engine, lgcn, nn as hnn


class LightGCNBase(object):
    """the graph encoder and the dot-product head, shared by the task variants below"""
    candidate_permutation_equivariant = True  # every candidate is scored on its own

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--emb_size', type=int, default=64, help='Size of embedding vectors.')
        parser.add_argument('--n_layers', type=int, default=3, help='Number of LightGCN layers.')
        return parser

    @staticmethod
    def build_adjmat(user_count, item_count, train_mat, selfloop_flag=False):
        """the reference's normalised adjacency (D^-1/2 A D^-1/2, no self loops) as CSR arrays (indptr, indices, data)"""
        if selfloop_flag:
            raise ValueError('LightGCN: selfloop_flag=True is not built (the reference never sets it)')
        return lgcn.build_norm_adj(user_count, item_count, train_mat)

    def _base_init(self, args, corpus):
        self.emb_size, self.n_layers = args.emb_size, args.n_layers
        engine.lgcn_check_shape(self.emb_size, self.n_layers)          # before the adjacency is built
        self.norm_adj = self.build_adjmat(corpus.n_users, corpus.n_items, corpus.train_clicked_set)
        engine.lgcn_check_shape(self.emb_size, self.n_layers, self.user_num + self.item_num, self.norm_adj[1].size)
        self._base_define_params()
        self.apply(self.init_weights)

    def _base_define_params(self):
        self.encoder = LGCNEncoder(self.user_num, self.item_num, self.emb_size, self.norm_adj, self.n_layers)

    def forward(self, feed_dict):
        self.check_list = []
        user, items = feed_dict['user_id'], feed_dict['item_id']   # [B], [B, n_candidates]
        u_all, i_all = self.encoder.tables()
        prediction = hnn.bprmf_scores(u_all, i_all, user, items)
        out = {'prediction': prediction.view(feed_dict['batch_size'], -1)}
        if isinstance(self, ImpressionModel):
            # LightGCNImpression hands back the base's whole dict (LightGCN.py:65-74,107-108): rerankers built on it read u_v / i_v
            out['u_v'] = hnn.table_rows(u_all, user)[:, None, :].expand(-1, items.shape[1], -1)
            out['i_v'] = hnn.table_rows(i_all, items)
        return out

    def full_catalogue_vectors(self, feed_dict):
        """(propagated user rows [B, d], propagated item table) of the dot-product head, for --test_all ranking"""
        u_all, i_all = self.encoder.tables()
        return engine.gather_rows(u_all.detach(), feed_dict['user_id']), i_all.detach()


class LGCNEncoder(nn.Module):
    """the two raw tables (state_dict keys embedding_dict.user_emb / item_emb, xavier_uniform like LightGCN.py:122-128) and the
    propagation over the normalised adjacency.  The CSR and its plan are non-persistent buffers (they follow .to(device));
    `chunk` sets the plan's split length (None: rechorus_amd.lgcn.default_chunk)."""

    def __init__(self, user_count, item_count, emb_size, norm_adj, n_layers=3, chunk=None):
        super().__init__()
        self.user_count, self.item_count, self.emb_size, self.n_layers = user_count, item_count, emb_size, n_layers
        self.layers = [emb_size] * n_layers
        initializer = nn.init.xavier_uniform_
        self.embedding_dict = nn.ParameterDict({
            'user_emb': nn.Parameter(initializer(torch.empty(user_count, emb_size))),
            'item_emb': nn.Parameter(initializer(torch.empty(item_count, emb_size))),
        })
        self._csr = norm_adj
        self._graph = None
        self._eval_tables = None
        self.set_chunk(chunk)

    def set_chunk(self, chunk):
        """(re)build the propagation plan with another chunk length; the buffers stay on the device they were on"""
        arrays, self.chunk, self.n_parts = lgcn.graph_arrays(self.user_count, self.item_count, *self._csr, chunk=chunk)
        dev = getattr(self, 'adj_indptr', torch.empty(0)).device
        for k, v in arrays.items():
            self.register_buffer('adj_' + k, torch.from_numpy(v).to(dev), persistent=False)
        self._graph, self._eval_tables = None, None

    def graph(self):
        t = {k: getattr(self, 'adj_' + k) for k in lgcn.GRAPH_KEYS}
        g = self._graph
        if g is None or g.tensors['indptr'] is not t['indptr']:      # first use, or the module moved
            if not t['indptr'].is_cuda:
                raise RuntimeError('LightGCN runs on the GPU only (move the model to cuda)')
            g = self._graph = lgcn.LgcnGraph(self.user_count, self.item_count, t, self.chunk, self.n_parts)
        return g

    def tables(self):
        """(propagated user table, propagated item table).  Training (or any forward that records gradients): one propagation per
        call, as the reference.  Evaluation without gradients: computed once and reused until the module is switched between
        train / eval, loaded from a state_dict, or either table's version changes."""
        U, I = self.embedding_dict['user_emb'], self.embedding_dict['item_emb']
        if self.training or torch.is_grad_enabled():
            return hnn.lgcn_propagate(U, I, self.graph(), self.n_layers)
        key = (U._version, I._version, U.data_ptr(), I.data_ptr())
        if self._eval_tables is None or self._eval_tables[0] != key:
            out = engine.lgcn_propagate_fwd(self.graph(), U.detach(), I.detach(), self.n_layers)
            self._eval_tables = (key, out[:self.user_count], out[self.user_count:])
        return self._eval_tables[1], self._eval_tables[2]

    def forward(self, users, items):
        """LGCNEncoder.forward of the reference: the propagated rows of `users` and `items`"""
        u_all, i_all = self.tables()
        return hnn.table_rows(u_all, users), hnn.table_rows(i_all, items)

    def train(self, mode=True):
        self._eval_tables = None
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self._eval_tables = None
        return super()._load_from_state_dict(*args, **kwargs)


_LOG = ['emb_size', 'n_layers', 'batch_size']
LightGCN = task_variant('LightGCN', GeneralModel, LightGCNBase, 'BaseReader', 'BaseRunner', _LOG, __name__,
                        doc='top-k recommendation with sampled negatives (BPR loss) on graph-propagated embeddings')
LightGCNImpression = task_variant('LightGCNImpression', ImpressionModel, LightGCNBase, 'ImpressionReader', 'ImpressionRunner', _LOG,
                                  __name__, doc='ranking inside impression lists on graph-propagated embeddings')
