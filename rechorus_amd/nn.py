"""torch.nn-shaped front of the HIP engine: what a ReChorus model file touches.

`HipEmbedding` is a drop-in for `nn.Embedding` (same `.weight` Parameter, same state_dict key)
whose forward and backward run in librechorus_hip.so; `bprmf_scores` / `bpr_loss` are the fused
head and loss as autograd Functions, so the reference's call order
`model(batch) -> model.loss(out) -> loss.backward() -> optimizer.step()`
(helpers/BaseRunner.py:193-206) keeps working unchanged while every FLOP is HIP.

Gradients reaching a table are DENSE `[n_rows, d]` tensors like autograd's
(aten::embedding_dense_backward semantics), built by sort + segmented sum (no atomics), so any
torch optimizer or `HipOptimizer` (rc_dense_update, exact torch.optim maths) can consume them.
The large-table row-wise path bypasses autograd entirely (`engine.BprmfTrainer`).
"""
import os

import torch
import torch.nn as nn

from . import engine


class _EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, ids):
        ctx.save_for_backward(ids)
        ctx.n_rows = weight.shape[0]
        return engine.gather_rows(weight.detach(), ids)

    @staticmethod
    def backward(ctx, grad_out):
        (ids,) = ctx.saved_tensors
        # a [B] or [B, <= 2] id tensor is a user / candidate list (the reference's default --num_neg 1): a row repeats only by
        # popularity, the two-launch small route fits.  A wider one may be a padded history window, whose padding id collects
        # thousands of occurrences: those keep the plan / sort routes
        route = "small" if (ids.dim() <= 1 or ids.shape[-1] <= 2) else None
        g = engine.embedding_dense_backward(grad_out.contiguous(), ids, ctx.n_rows, route=route)
        return g, None


class HipEmbedding(nn.Module):
    """nn.Embedding(num_embeddings, embedding_dim) on the HIP engine (reference call sites:
    models/general/BPRMF.py:31-32,39-40 and the 88 other `nn.Embedding` definitions)."""

    def __init__(self, num_embeddings, embedding_dim):
        super().__init__()
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        self.weight = nn.Parameter(torch.empty(num_embeddings, embedding_dim))
        nn.init.normal_(self.weight)  # nn.Embedding's default; models re-init via init_weights

    def forward(self, ids):
        if not self.weight.is_cuda:
            raise RuntimeError("HipEmbedding runs on the GPU only (move the model to cuda)")
        return _EmbeddingFn.apply(self.weight, ids.contiguous())

    def extra_repr(self):
        return f"{self.num_embeddings}, {self.embedding_dim} [HIP]"


_DROP_SEED_GEN = None


def fresh_drop_seed():
    """int64 [1] seed for a module's counter-based dropout masks, drawn from a generator of its OWN (seeded from torch's
    initial seed, so runs with the same --random_seed repeat) -- the global RNG stream that initialises the parameters is
    left exactly as the reference leaves it."""
    global _DROP_SEED_GEN
    if _DROP_SEED_GEN is None:
        _DROP_SEED_GEN = torch.Generator()
        _DROP_SEED_GEN.manual_seed((torch.initial_seed() * 6364136223846793005 + 1442695040888963407) % (2 ** 63))
    return torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=_DROP_SEED_GEN)


def adopt_embeddings(model):
    """Make an unmodified ReChorus model file run its table lookups on the HIP engine: every plain `nn.Embedding`
    submodule (the reference defines all 88 of its tables that way, sparse=False, no padding_idx / max_norm) is
    replaced by a `HipEmbedding` that SHARES its `weight` Parameter -- state_dict keys, init_weights, optimizer
    parameter groups and checkpoints stay what the model file expects.  Returns the number of tables adopted;
    embeddings with options HipEmbedding does not implement are left on torch."""
    n = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if type(child) is not nn.Embedding:
                continue
            if child.sparse or child.padding_idx is not None or child.max_norm is not None or child.scale_grad_by_freq:
                continue
            hip = HipEmbedding.__new__(HipEmbedding)
            nn.Module.__init__(hip)
            hip.num_embeddings, hip.embedding_dim = child.num_embeddings, child.embedding_dim
            hip.weight = child.weight
            setattr(parent, name, hip)
            n += 1
    return n


class _BprmfScoreFn(torch.autograd.Function):
    """prediction[b,c] = <U[uid[b]], I[iid[b,c]]>  (models/general/BPRMF.py:39-42)."""

    @staticmethod
    def forward(ctx, U, I, uid, iid):
        ctx.save_for_backward(U, I, uid, iid)
        return engine.gather_dot(U.detach(), I.detach(), uid, iid)

    @staticmethod
    def backward(ctx, gpred):
        U, I, uid, iid = ctx.saved_tensors
        Ud, Id = U.detach(), I.detach()
        gpred = gpred.contiguous()
        C = iid.shape[1]
        # dL/dI[r] = sum_{(b,c): iid[b,c]=r} g[b,c] * U[uid[b]]  (rows rebuilt on the fly)
        keys, perm = engine.sort_ids(iid, I.shape[0])
        GI = torch.zeros_like(Id)
        engine.segmented_update(keys, perm, Ud, coef=gpred.reshape(-1), src_index=uid, div=C,
                                dense_grad=GI)
        # dL/dU[r] = sum_{b: uid[b]=r} sum_c g[b,c] * I[iid[b,c]]
        ug = engine.weighted_row_sum(Id, iid, gpred)
        GU = engine.embedding_dense_backward(ug, uid, U.shape[0])
        return GU, GI, None, None


def bprmf_scores(U, I, uid, iid):
    return _BprmfScoreFn.apply(U, I, uid.contiguous(), iid.contiguous())


class _FpmcScoreFn(torch.autograd.Function):
    """prediction[b,c] = <UI[uid[b]], IU[iid[b,c]]> + <LI[lid[b]], IL[iid[b,c]]>  (models/sequential/FPMC.py:44-56)."""

    @staticmethod
    def forward(ctx, UI, LI, IU, IL, uid, lid, iid):
        ctx.save_for_backward(UI, LI, IU, IL, uid, lid, iid)
        return engine.fpmc_scores(UI.detach(), LI.detach(), IU.detach(), IL.detach(), uid, lid, iid)

    @staticmethod
    def backward(ctx, gpred):
        UI, LI, IU, IL, uid, lid, iid = (t.detach() for t in ctx.saved_tensors)
        gpred = gpred.contiguous()
        # item side: dL/dIU[r] = sum_{(b,c): iid[b,c]=r} g[b,c] * UI[uid[b]], dL/dIL[r] likewise from LI[lid[b]] -- one pass
        keys, perm = engine.sort_ids(iid, IU.shape[0])
        _, heads, n_heads = engine.segment_heads(keys, perm, want_single=False)
        GIU, GIL = torch.zeros_like(IU), torch.zeros_like(IL)
        engine.fpmc_item_update(keys, perm, heads, n_heads, gpred, UI, LI, uid, lid, dense_grad=(GIU, GIL))
        # query side: per-tuple rows sum_c g[b,c] * IU / IL[iid[b,c]], summed per user / per last item
        GUI, GLI = torch.zeros_like(UI), torch.zeros_like(LI)
        for G, table, ids in ((GUI, IU, uid), (GLI, IL, lid)):
            rows = engine.weighted_row_sum(table, iid, gpred)
            k, p = engine.sort_ids(ids, G.shape[0])
            engine.segmented_update(k, p, rows, dense_grad=G)
        return GUI, GLI, GIU, GIL, None, None, None


def fpmc_scores(UI, LI, IU, IL, uid, lid, iid):
    """FPMC's two-term head as one autograd node: dense gradients for the four tables from an arbitrary loss on the scores"""
    return _FpmcScoreFn.apply(UI, LI, IU, IL, uid.contiguous(), lid.contiguous(), iid.contiguous())


class _SlrcScoreFn(torch.autograd.Function):
    """SLRC+'s prediction (models/sequential/SLRCPlus.py:62-89) with dense gradients for its ten parameters; none for the ids or the
    intervals.  The backward runs on the saved inputs: per-candidate excitation derivatives are recomputed by rc_slrc_fwd_bwd's
    arithmetic through engine.slrc_excitation_grads."""

    @staticmethod
    def forward(ctx, uid, iid, intervals, *params):
        ctx.save_for_backward(uid, iid, intervals, *params)
        return engine.slrc_scores([p.detach() for p in params], uid, iid, intervals)

    @staticmethod
    def backward(ctx, gpred):
        uid, iid, intervals, *params = (t.detach() for t in ctx.saved_tensors)
        U, I, ub, ib, ga = params[:5]
        gpred = gpred.contiguous()
        # the per-occurrence Hawkes rows and the per-tuple partials, scaled by the incoming gradient
        hgrad, ubgrad, gagrad = engine.slrc_excitation_grads(params, uid, iid, intervals, gpred)
        keys, perm = engine.sort_ids(iid, I.shape[0])
        _, heads, n_heads = engine.segment_heads(keys, perm, want_single=False)
        dense = [torch.zeros_like(params[k]) for k in (1, 3, 5, 6, 7, 8, 9)]
        engine.slrc_item_update(keys, perm, heads, n_heads, gpred, hgrad, U, uid, dense_grad=dense)
        GI, Gib, *GH = dense
        # user side: per-tuple rows sum_c g[b,c] * I[iid[b,c]] and sum_c g[b,c], summed per user
        GU, Gub = torch.zeros_like(U), torch.zeros_like(ub)
        k, p = engine.sort_ids(uid, U.shape[0])
        engine.segmented_update(k, p, engine.weighted_row_sum(I, iid, gpred), dense_grad=GU)
        engine.slrc_user_bias_update(k, p, ubgrad, dense_grad=Gub)
        Gga = engine.reduce_sum(gagrad).reshape(ga.shape)
        return (None, None, None, GU, GI, Gub, Gib, Gga, *GH)


def slrc_scores(params, uid, iid, intervals):
    """SLRC+'s head as one autograd node: dense gradients for the ten parameters (engine.SLRC_PARAMS order) from an arbitrary loss
    on the scores; the intervals take no gradient"""
    return _SlrcScoreFn.apply(uid.contiguous(), iid.contiguous(), intervals.contiguous(), *params)


class _CfkgScoreFn(torch.autograd.Function):
    """prediction[b,c] = -|E[head[b,c]] + R[rel[b,c]] - E[tail[b,c]]|^2  (models/general/CFKG.py:57-68), dense gradients for E, R."""

    @staticmethod
    def forward(ctx, E, R, head, tail, rel):
        ctx.save_for_backward(E, R, head, tail, rel)
        return engine.cfkg_scores(E.detach(), R.detach(), head, tail, rel)

    @staticmethod
    def backward(ctx, gpred):
        E, R, head, tail, rel = (t.detach() for t in ctx.saved_tensors)
        n = head.numel()
        # one row per (b, c): the head's gradient; the tail's is its negative, the relation's equals it
        G = engine.cfkg_scores_grads(E, R, head, tail, rel, gpred.contiguous())
        # E serves heads and tails alike: ONE sort over both id lists, occurrence o and o + n both read row o of G (coef +1 / -1)
        keys, perm = engine.sort_ids(torch.cat((head.reshape(-1), tail.reshape(-1))), E.shape[0])
        coef = torch.ones(2 * n, dtype=torch.float32, device=G.device)
        coef[n:] = -1.0
        src_index = torch.arange(n, dtype=torch.int64, device=G.device).repeat(2)
        GE = torch.zeros_like(E)
        engine.segmented_update(keys, perm, G, coef=coef, src_index=src_index, dense_grad=GE)
        GR = engine.embedding_dense_backward(G, rel, R.shape[0], route="sort")
        return GE, GR, None, None, None


def cfkg_scores(E, R, head, tail, rel):
    """CFKG's translation-distance head as one autograd node: dense gradients for the entity and the relation table from an
    arbitrary loss on the scores"""
    return _CfkgScoreFn.apply(E, R, head.contiguous(), tail.contiguous(), rel.contiguous())


class _ChorusScoreFn(torch.autograd.Function):
    """Chorus's stage-2 prediction (models/sequential/Chorus.py:122-153) with dense gradients for its nine parameters; none for the
    ids or the intervals.  The backward runs on the saved inputs through engine.chorus_scores_grads (rc_chorus_scores_bwd) and the
    row updates' dense-gradient forms.  A parameter the head does not read (prediction.weight under BPR, the biases under GMF, sigmas
    and mus without a 'substitute' relation) gets no gradient, as in the reference."""

    @staticmethod
    def forward(ctx, uid, iid, cid, intervals, kinds, gmf, *params):
        ctx.save_for_backward(uid, iid, cid, intervals, *params)
        ctx.kinds, ctx.gmf = list(kinds), bool(gmf)
        return engine.chorus_scores([p.detach() for p in params], uid, iid, cid, intervals, ctx.kinds, ctx.gmf)

    @staticmethod
    def backward(ctx, gpred):
        uid, iid, cid, intervals, *params = (t.detach() for t in ctx.saved_tensors)
        U, I, Rel, betas, mus, sigmas, w, ub, ib = params
        gmf, Cn = ctx.gmf, iid.shape[1]
        gpred = gpred.contiguous()
        out = engine.chorus_scores_grads(params, uid, iid, cid, intervals, ctx.kinds, gpred, gmf)
        ikeys, iperm = engine.sort_ids(iid, I.shape[0])
        GI = torch.zeros_like(I)
        if gmf:
            engine.segmented_update(ikeys, iperm, out["uprime"], coef=out["coef"], div=Cn, dense_grad=GI)
        else:
            engine.segmented_update(ikeys, iperm, U, coef=out["coef"], src_index=uid, div=Cn, dense_grad=GI)
        ckeys, cperm = engine.sort_ids(cid, betas.shape[0])
        _, heads, n_heads = engine.segment_heads(ckeys, cperm, want_single=False)
        Gb, Gs, Gm = torch.zeros_like(betas), torch.zeros_like(sigmas), torch.zeros_like(mus)
        engine.chorus_category_update(ckeys, cperm, heads, n_heads, out["kgrad"], betas.shape[0], dense_grad=[Gb, Gs, Gm])
        ukeys, uperm = engine.sort_ids(uid, U.shape[0])
        GU = torch.zeros_like(U)
        engine.segmented_update(ukeys, uperm, out["ugrad"], dense_grad=GU)
        if 2 not in ctx.kinds:      # sigmas and mus are read by the 'substitute' kernel alone
            Gs = Gm = None
        Gw = Gub = Gib = None
        if gmf:
            Gw = out["gw"].view_as(w)
        else:
            Gub, Gib = torch.zeros_like(ub), torch.zeros_like(ib)
            engine.slrc_user_bias_update(ukeys, uperm, out["ubgrad"], dense_grad=Gub)
            engine.slrc_user_bias_update(ikeys, iperm, gpred, dense_grad=Gib)
        return (None, None, None, None, None, None, GU, GI, out["GRel"], Gb, Gm, Gs, Gw, Gub, Gib)


def chorus_scores(params, uid, iid, cid, intervals, kinds, gmf=False):
    """Chorus's stage-2 head as one autograd node: dense gradients for the nine parameters (engine.CHORUS_PARAMS order) from an
    arbitrary loss on the scores; kinds: engine.chorus_kinds(item_relations).  The stage-1 forward is cfkg_scores on (i_embeddings,
    r_embeddings)."""
    return _ChorusScoreFn.apply(uid.contiguous(), iid.contiguous(), cid.contiguous(), intervals.contiguous(), kinds, gmf, *params)


class _DinAttentionFn(torch.autograd.Function):
    """DIN.attention (models/context_seq/DIN.py:63-95) for instance n = b C + c over the history of row b, as ONE node: the forward
    keeps q, keys and the flat parameters; the backward recomputes everything from them (same dropout seed and site)."""

    @staticmethod
    def forward(ctx, q, keys, lengths, flat, n_cand, widths, drop_p, seed, site0):
        q, keys, flat = q.detach().contiguous(), keys.detach().contiguous(), flat.detach().contiguous()
        # the seed's VALUE at the forward: the caller may bump the device counter before the backward recomputes the mask
        seed = seed.clone() if (drop_p and seed is not None) else None
        ctx.save_for_backward(q, keys, lengths, flat, seed)
        ctx.args = (n_cand, widths, drop_p, site0)
        out, att = engine.din_attention_fwd(q, keys, lengths, flat, n_cand, widths, drop_p, seed, site0, want_att=True)
        ctx.mark_non_differentiable(att)
        return out, att

    @staticmethod
    def backward(ctx, d_out, _d_att):
        q, keys, lengths, flat, seed = ctx.saved_tensors
        n_cand, widths, drop_p, site0 = ctx.args
        dq, dkeys, dflat = engine.din_attention_bwd(q, keys, lengths, flat, d_out.contiguous(), n_cand, widths, drop_p, seed, site0)
        return dq, dkeys, None, dflat, None, None, None, None, None


def din_attention(q, keys, lengths, n_cand, params, drop_p=0.0, seed=None, site0=0):
    """DIN's target attention as one autograd node.  q [B * n_cand, H], keys [B, L, H], lengths int64 [B];
    params = [(W_1, b_1), ..., (W_k, b_k), (w_out, b_out)]: the Linear layers of att_mlp_layers in order (Sigmoid and Dropout(drop_p)
    behind every hidden one).  Returns (out [N, H], att [N, L]): the weighted key sum and the masked, scaled weights (the reference's
    return_seq_weight; no gradient flows through att).  drop_p > 0 (training): `seed` int64 [1] on the device, layers use sites
    site0, site0 + 1, ...  The parameters travel as one flat buffer (a torch.cat of a few thousand floats, whose autograd hands every
    layer its slice of the flat gradient); nothing of N * L rows exists outside the kernels."""
    widths = tuple(int(W.shape[0]) for W, _ in params[:-1])
    flat = torch.cat([t.reshape(-1) for pair in params for t in pair])
    return _DinAttentionFn.apply(q, keys, lengths.contiguous(), flat, int(n_cand), widths, float(drop_p), seed if drop_p else None, int(site0))


class _KdaAggregateFn(torch.autograd.Function):
    """RelationalDynamicAggregation.forward (models/sequential/KDA.py:265-303) as ONE node: the forward keeps its inputs, the backward
    recomputes everything from them (nothing of size B C L R is kept)."""

    @staticmethod
    def forward(ctx, seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val):
        seq, target, rel = seq.detach().contiguous(), target.detach().contiguous(), rel.detach().contiguous()
        value = value.detach().contiguous() if include_val else None
        freq_real, freq_imag = freq_real.detach().contiguous(), freq_imag.detach().contiguous()
        ctx.include_val = include_val
        ctx.save_for_backward(seq, hist, delta_t, target, value, rel, freq_real, freq_imag)
        return engine.kda_aggregate_fwd(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val)

    @staticmethod
    def backward(ctx, d_context):
        dseq, dtarget, dvalue, drel, dfr, dfi = engine.kda_aggregate_bwd(*ctx.saved_tensors, d_context.contiguous(), ctx.include_val)
        return dseq, None, None, dtarget, dvalue, drel, dfr, dfi, None


def kda_aggregate(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val=True):
    """KDA's relational dynamic aggregation as one autograd node.  seq [B, L, V] history rows, hist int64 [B, L] (valid iff > 0, anywhere
    in the row), delta_t fp32 [B, L], target [B, C, V], value [B, C, R, V] (read only with include_val; may be None without), rel [R, V],
    freq_real / freq_imag [R, F].  Returns context [B, C, R, V]; gradients flow to seq, target, value, rel and both frequency tables.
    A row without a valid position gives a zero context and zero gradients."""
    return _KdaAggregateFn.apply(seq, hist.contiguous(), delta_t.float().contiguous(), target, value if include_val else None, rel,
                                 freq_real, freq_imag, bool(include_val))


def table_rows(W, ids):
    """W[ids] with an autograd that sums the rows' gradients into a dense [n_rows, d] tensor (HipEmbedding's lookup on a table
    that is not a module's Parameter, e.g. LightGCN's propagated tables)"""
    return _EmbeddingFn.apply(W, ids.contiguous())


class _LgcnPropagateFn(torch.autograd.Function):
    """LGCNEncoder.forward's propagation (models/general/LightGCN.py:137-151): mean(E_0, A E_0, ..., A^L E_0), E_0 = the two
    tables; backward sum_l A^l G / (L+1) (A symmetric).  Both directions are rc_lgcn_propagate_fwd/bwd on the graph's plan."""

    @staticmethod
    def forward(ctx, user_emb, item_emb, graph, n_layers):
        ctx.graph, ctx.n_layers = graph, n_layers
        # the graph's persistent output buffer: a captured training step replays on the same memory
        out = engine.lgcn_propagate_fwd(graph, user_emb.detach(), item_emb.detach(), n_layers, out="persistent")
        return out[:graph.n_users], out[graph.n_users:]

    @staticmethod
    def backward(ctx, g_user, g_item):
        graph = ctx.graph
        if g_user is None and g_item is None:
            return None, None, None, None
        ref = g_user if g_user is not None else g_item
        dim = ref.shape[1]
        if g_user is None:
            g_user = torch.zeros((graph.n_users, dim), dtype=torch.float32, device=ref.device)
        if g_item is None:
            g_item = torch.zeros((graph.n_items, dim), dtype=torch.float32, device=ref.device)
        gu, gi = engine.lgcn_propagate_bwd(graph, g_user.contiguous(), g_item.contiguous(), ctx.n_layers)
        return gu, gi, None, None


def lgcn_propagate(user_emb, item_emb, graph, n_layers):
    """(propagated user table, propagated item table): the two halves of one [N, d] buffer, each a contiguous view"""
    return _LgcnPropagateFn.apply(user_emb, item_emb, graph, int(n_layers))


class _DirectAUFn(torch.autograd.Function):
    """DirectAU's loss terms (models/general/DirectAU.py:54-88) on rc_directau_fwd / _bwd.  term "loss": align + gamma (unif(U) +
    unif(I)) / 2; "align": alignment(x, y); "unif": uniformity(x) (x passed as both inputs, the item half not computed).  Backward:
    the two [B, d] per-occurrence row gradients."""

    _TERMS = {"loss": (3, 0), "align": (0, 1), "unif": (1, 2)}   # term -> (uniformity sets computed, slot of out[4])

    @staticmethod
    def forward(ctx, user_e, item_e, gamma, term, workspace):
        sets, slot = _DirectAUFn._TERMS[term]
        ws = workspace if workspace is not None else engine.DirectAUWorkspace()
        out, _, buf, gen = engine.directau_fwd(user_e.detach(), item_e.detach(), gamma, sets=sets, workspace=ws)
        ctx.buf, ctx.gen, ctx.workspace = buf, gen, ws
        ctx.batch, ctx.d, ctx.term = user_e.shape[0], user_e.shape[1], term
        ctx.coef = {"loss": (1.0, gamma / 2.0, gamma / 2.0), "align": (1.0, 0.0, 0.0), "unif": (0.0, 1.0, 0.0)}[term]
        return out[slot]

    @staticmethod
    def backward(ctx, g):
        if ctx.workspace.generation != ctx.gen:
            raise RuntimeError("DirectAU loss: another DirectAU forward ran on this workspace before this backward; give each "
                               "pending loss a workspace of its own (rechorus_amd.engine.DirectAUWorkspace)")
        unif = ctx.term == "unif"
        gu, gi = engine.directau_bwd(g, ctx.batch, ctx.d, ctx.coef, ctx.buf, want_user=True, want_item=not unif)
        return gu, gi, None, None, None


def directau_loss(user_e, item_e, gamma, workspace=None):
    """DirectAU.loss (models/general/DirectAU.py:80-86) on the rows [B, d] of one batch, as ONE autograd node; workspace: the
    model's engine.DirectAUWorkspace, reused step after step (None: a fresh one for this call)"""
    return _DirectAUFn.apply(user_e.contiguous(), item_e.contiguous(), float(gamma), "loss", workspace)


def alignment(x, y, workspace=None):
    """DirectAU.alignment (:54-57): mean_b |normalize(x_b) - normalize(y_b)|^2"""
    return _DirectAUFn.apply(x.contiguous(), y.contiguous(), 0.0, "align", workspace)


def uniformity(x, workspace=None):
    """DirectAU.uniformity (:59-62): log mean_{i<j} exp(-2 |normalize(x_i) - normalize(x_j)|^2), without torch.pdist"""
    x = x.contiguous()
    return _DirectAUFn.apply(x, x, 0.0, "unif", workspace)


class _ComiRecFn(torch.autograd.Function):
    """ComiRec's multi-interest extraction with the hard selection of training (models/sequential/ComiRec.py:64-87) on
    rc_comirec_fwd / _bwd -> (user [B, d], interests [B, K, d], sel [B]); only `user` carries gradient, none flows through the
    selection.  Backward: dense gradients of the item table (engine.embedding_dense_backward over the history occurrences), the
    position table (the SASRec position rule) and the four weight tensors."""

    @staticmethod
    def forward(ctx, item_w, pos_w, W1, b1, W2, b2, hist, lengths, targets, workspace):
        det = [t.detach().contiguous() if t is not None else None for t in (item_w, pos_w, W1, b1, W2, b2)]
        interests, attn, sel, user = engine.comirec_fwd(*det, hist, lengths, targets=targets)
        ctx.save_for_backward(*[t for t in det[:5] if t is not None], hist, lengths, attn, sel, user)
        ctx.has_pos, ctx.workspace = pos_w is not None, workspace
        ctx.n_items, ctx.n_pos = item_w.shape[0], (pos_w.shape[0] if pos_w is not None else 0)
        ctx.mark_non_differentiable(interests, sel)
        return user, interests, sel

    @staticmethod
    def backward(ctx, d_user, _gi, _gs):
        saved = list(ctx.saved_tensors)
        item_w = saved.pop(0)
        pos_w = saved.pop(0) if ctx.has_pos else None
        W1, b1, W2, hist, lengths, attn, sel, user = saved
        g_hist, g_x, dW1, db1, dW2, db2 = engine.comirec_bwd(item_w, pos_w, W1, b1, W2, hist, lengths, attn, sel, user,
                                                             d_user.contiguous(), workspace=ctx.workspace)
        G_item = engine.embedding_dense_backward(g_hist, hist, ctx.n_items)
        G_pos = None
        if ctx.has_pos:
            if g_x.shape[2] in (32, 64):
                G_pos = engine.sasrec_pos_grad(g_x, lengths, ctx.n_pos)
            else:
                B, L, d = g_x.shape
                G_pos = engine.seq_pos_grad(g_x.view(B * L, d), lengths, B, L, ctx.n_pos)
        return G_item, G_pos, dW1, db1, dW2, db2, None, None, None, None


def comirec_user_vector(item_w, pos_w, W1, b1, W2, b2, hist, lengths, targets, workspace=None, details=False):
    """the training path of ComiRec.py:64-87: user [B, d] = the interest of each sequence that scores its target item highest
    (pos_w None: --add_pos 0).  Its output goes into bprmf_scores(user, item_w, arange(B), item_id), which adds the candidates'
    gradient to the item table.  details=True: (user, interests [B, K, d], sel int32 [B]) -- the latter two carry no gradient."""
    out = _ComiRecFn.apply(item_w, pos_w, W1, b1, W2, b2, hist.contiguous(), lengths.contiguous(), targets.contiguous(), workspace)
    return out if details else out[0]


def comirec_scores(item_w, pos_w, W1, b1, W2, b2, hist, lengths, item_id):
    """the evaluation path of ComiRec.py:64-80,90-91: prediction [B, C] = max_k <interest[b, k], item_w[item_id[b, c]]>; forward
    only (rc_comirec_score_max has no backward): raises when autograd is recording"""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (item_w, pos_w, W1, b1, W2, b2)):
        raise RuntimeError("comirec_scores is the evaluation path and has no backward: call it under torch.no_grad() "
                           "(training goes through comirec_user_vector)")
    det = [t.detach().contiguous() if t is not None else None for t in (item_w, pos_w, W1, b1, W2, b2)]
    interests, _, _, _ = engine.comirec_fwd(*det, hist.contiguous(), lengths.contiguous(), want_attn=False)
    return engine.comirec_score_max(interests, det[0], item_id.contiguous())


class _AutoIntLayerFn(torch.autograd.Function):
    """One AutoInt interacting layer (models/context/AutoInt.py:72-75) on rc_autoint_layer_fwd / _bwd.  Saves X and Y only: the
    backward recomputes Q, K, V and the softmax.  No host synchronisation and no data-dependent allocation: capture-safe."""

    @staticmethod
    def forward(ctx, X, Wq, Wk, Wv, Wr, br, heads, workspace):
        det = [t.detach().contiguous() for t in (X, Wq, Wk, Wv, Wr, br)]
        Y = engine.autoint_layer_fwd(*det, heads)
        ctx.save_for_backward(*det[:5], Y)
        ctx.heads, ctx.workspace = heads, workspace
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, Wq, Wk, Wv, Wr, Y = ctx.saved_tensors
        dX, dWq, dWk, dWv, dWr, dbr = engine.autoint_layer_bwd(X, Wq, Wk, Wv, Wr, Y, dY.contiguous(), ctx.heads,
                                                               workspace=ctx.workspace)
        return dX, dWq, dWk, dWv, dWr, dbr, None, None


def autoint_layer(X, Wq, Wk, Wv, Wr, br, heads, workspace=None):
    """relu(MultiHeadAttention(X, X, X) + Linear(X)) over the fields of each instance (models/context/AutoInt.py:72-75): X [..., F,
    Din], Wq / Wk / Wv / Wr [A, Din], br [A] -> [..., F, A], as ONE autograd node (one forward launch, one backward launch plus the
    fixed-order reduce); workspace: the model's engine.AutoIntWorkspace, reused step after step"""
    return _AutoIntLayerFn.apply(X, Wq, Wk, Wv, Wr, br, int(heads), workspace)


def autoint_layer_eval(X, Wq, Wk, Wv, Wr, br, heads):
    """the same layer on the evaluation path: forward only, raises when autograd is recording"""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (X, Wq, Wk, Wv, Wr, br)):
        raise RuntimeError("autoint_layer_eval is the evaluation path and has no backward: call it under torch.no_grad() "
                           "(training goes through autoint_layer)")
    return engine.autoint_layer_fwd(*[t.detach().contiguous() for t in (X, Wq, Wk, Wv, Wr, br)], int(heads))


class _Dcnv2MixLayerFn(torch.autograd.Function):
    """One mixed cross layer of DCNv2 (models/context/DCNv2.py:119-141) on rc_dcnv2_mix_layer_fwd / _bwd.  Saves its inputs only:
    the backward recomputes both tanh stages and the gate.  No host synchronisation and no data-dependent allocation: capture-safe."""

    @staticmethod
    def forward(ctx, X0, Xl, U, V, C, bias, Wg, bg, workspace):
        det = [t.detach().contiguous() for t in (X0, Xl, U, V, C, bias, Wg, bg)]
        Xnext = engine.dcnv2_mix_layer_fwd(*det)
        ctx.save_for_backward(*det)
        ctx.workspace = workspace
        return Xnext

    @staticmethod
    def backward(ctx, dXnext):
        dXl, dX0, dU, dV, dC, dbias, dWg, dbg = engine.dcnv2_mix_layer_bwd(dXnext.contiguous(), *ctx.saved_tensors,
                                                                           workspace=ctx.workspace)
        return dX0, dXl, dU, dV, dC, dbias, dWg, dbg, None


def dcnv2_mix_layer(X0, Xl, U, V, C, bias, Wg, bg, workspace=None):
    """x_l + x_0 * sum_e softmax(gate)_e (U_e tanh(C_e tanh(V_e^T x_l)) + bias) (models/context/DCNv2.py:119-141): X0, Xl [..., D],
    U, V [E, D, r], C [E, r, r], bias [D] or [D, 1], the gate Wg [E, D], bg [E] -> [..., D], as ONE autograd node (one forward launch,
    one backward launch plus the fixed-order reduce).  X0's gradient is this layer's share; autograd sums the layers'.
    workspace: the model's engine.DCNv2Workspace, reused step after step"""
    return _Dcnv2MixLayerFn.apply(X0, Xl, U, V, C, bias, Wg, bg, workspace)


def dcnv2_mix_layer_eval(X0, Xl, U, V, C, bias, Wg, bg):
    """the same layer on the evaluation path: forward only, raises when autograd is recording"""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (X0, Xl, U, V, C, bias, Wg, bg)):
        raise RuntimeError("dcnv2_mix_layer_eval is the evaluation path and has no backward: call it under torch.no_grad() "
                           "(training goes through dcnv2_mix_layer)")
    return engine.dcnv2_mix_layer_fwd(*[t.detach().contiguous() for t in (X0, Xl, U, V, C, bias, Wg, bg)])


class _ListEncoderBlockFn(torch.autograd.Function):
    """One post-norm encoder block over candidate lists (models/reranker/PRM.py:64,90-92) on rc_listenc_block_fwd / _bwd.  Saves X,
    the mask and the weights only: the backward recomputes the block.  No host synchronisation and no data-dependent allocation:
    capture-safe."""

    @staticmethod
    def forward(ctx, X, pad, heads, workspace, *weights):
        det = [t.detach().contiguous() for t in (X, *weights)]
        pad = pad.detach().to(torch.uint8).contiguous()
        Y = engine.listenc_block_fwd(det[0], pad, det[1:], heads)
        ctx.save_for_backward(pad, *det)
        ctx.heads, ctx.workspace = heads, workspace
        return Y

    @staticmethod
    def backward(ctx, dY):
        pad, X, *weights = ctx.saved_tensors
        dX, grads = engine.listenc_block_bwd(dY.contiguous(), X, pad, weights, ctx.heads, workspace=ctx.workspace)
        return (dX, None, None, None, *grads)


def list_encoder_block(X, pad, weights, heads, workspace=None):
    """nn.TransformerEncoderLayer(d, heads, d_ff, dropout=0) (post-norm, ReLU, eps 1e-5) over lists X [B, n, d] under the key-padding
    mask pad [B, n] (true / 1 = padded slot) (models/reranker/PRM.py:64,90-92) -> [B, n, d], as ONE autograd node (one forward launch,
    one backward launch plus the fixed-order reduce).  weights: in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias,
    norm1.weight, norm1.bias, linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm2.weight, norm2.bias
    (engine.LISTENC_WEIGHTS order).  workspace: the model's engine.ListEncWorkspace, reused step after step"""
    return _ListEncoderBlockFn.apply(X, pad, int(heads), workspace, *weights)


def list_encoder_block_eval(X, pad, weights, heads):
    """the same block on the evaluation path: forward only, raises when autograd is recording"""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (X, *weights)):
        raise RuntimeError("list_encoder_block_eval is the evaluation path and has no backward: call it under torch.no_grad() "
                           "(training goes through list_encoder_block)")
    return engine.listenc_block_fwd(X.detach().contiguous(), pad.detach().to(torch.uint8).contiguous(),
                                    [t.detach().contiguous() for t in weights], int(heads))


class _SetAttentionBlockFn(torch.autograd.Function):
    """One multihead attention block whose query rows are not its key rows (models/reranker/SetRank.py:29-56) on rc_setmab_fwd / _bwd.
    Saves Qs, Ks, the mask and the weights only: the backward recomputes the block.  No host synchronisation and no data-dependent
    allocation: capture-safe."""

    @staticmethod
    def forward(ctx, Qs, Ks, pad, heads, workspace, shared_q, *weights):
        det = [t.detach().contiguous() for t in (Qs, Ks, *weights)]
        pad = None if pad is None else pad.detach().to(torch.uint8).contiguous()
        Y = engine.setmab_fwd(det[0], det[1], pad, det[2:], heads, shared_q)
        ctx.save_for_backward(pad, *det)
        ctx.heads, ctx.workspace, ctx.shared_q = heads, workspace, shared_q
        return Y

    @staticmethod
    def backward(ctx, dY):
        pad, Qs, Ks, *weights = ctx.saved_tensors
        dQs, dKs, grads = engine.setmab_bwd(dY.contiguous(), Qs, Ks, pad, weights, ctx.heads, ctx.shared_q, workspace=ctx.workspace)
        return (dQs, dKs, None, None, None, None, *grads)


def set_attention_block(Qs, Ks, pad, weights, heads, workspace=None, shared_q=False):
    """SetRank's MAB (models/reranker/SetRank.py:29-56): LN2(X1 + rFF(X1)), X1 = LN1(Qs + MultiheadAttention(Qs, Ks, Ks)) under the
    key-padding mask pad [B, nk] (true / 1 = padded key; None: no key is masked) -> [B, nq, d], as ONE autograd node (one forward
    launch; the backward is one launch plus the fixed-order reduces).  Ks [B, nk, d]; Qs [B, nq, d], or with shared_q ONE [nq, d]
    source for every list, whose gradient is the sum over the lists.  weights as list_encoder_block takes them
    (engine.LISTENC_WEIGHTS order).  workspace: the model's engine.SetMabWorkspace, reused step after step"""
    return _SetAttentionBlockFn.apply(Qs, Ks, pad, int(heads), workspace, bool(shared_q), *weights)


def set_attention_block_eval(Qs, Ks, pad, weights, heads, shared_q=False):
    """the same block on the evaluation path: forward only, raises when autograd is recording"""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (Qs, Ks, *weights)):
        raise RuntimeError("set_attention_block_eval is the evaluation path and has no backward: call it under torch.no_grad() "
                           "(training goes through set_attention_block)")
    return engine.setmab_fwd(Qs.detach().contiguous(), Ks.detach().contiguous(),
                             None if pad is None else pad.detach().to(torch.uint8).contiguous(),
                             [t.detach().contiguous() for t in weights], int(heads), bool(shared_q))


def induced_set_block(x, pad, I, w1, w2, heads, workspace=None):
    """SetRank's IMSAB (models/reranker/SetRank.py:67-80): h = MAB1(I, x, x) under the key-padding mask, x' = MAB2(x, h, h) without
    one.  x [B, n, d], pad [B, n], I [m, d] the learned inducing points shared by every list, w1 / w2 the two blocks' twelve weights ->
    [B, n, d].  Two set_attention_block nodes: h [B, m, d] passes between them as an ordinary tensor and autograd adds x's two
    gradients (MAB1's keys, MAB2's queries)."""
    h = set_attention_block(I, x, pad, w1, heads, workspace, shared_q=True)
    return set_attention_block(x, h, None, w2, heads, workspace)


def induced_set_block_eval(x, pad, I, w1, w2, heads):
    """the same induced block on the evaluation path: forward only"""
    return set_attention_block_eval(x, set_attention_block_eval(I, x, pad, w1, heads, shared_q=True), None, w2, heads)


class _FinalMlpGateFn(torch.autograd.Function):
    """FinalMLP's feature gates and the first layer of both streams (models/context/FinalMLP.py:188-221, :100-101) on
    rc_finalmlp_gate_fwd / _bwd.  Saves X, the gate inputs, the weights and A_1, A_2 (their own ReLU / dropout masks): the gates are
    recomputed, nothing of size N D is kept.  No host synchronisation and no data-dependent allocation: capture-safe."""

    @staticmethod
    def forward(ctx, X, n_cand, opts, workspace, Zin1, Wg1, bg1, W1, b1, Zin2, Wg2, bg2, W2, b2):
        det = [t.detach().contiguous() for t in (X, Zin1, Wg1, bg1, W1, b1, Zin2, Wg2, bg2, W2, b2)]
        Xf = det[0].reshape(-1, det[0].shape[-1])
        (p1, seed1, site1), (p2, seed2, site2) = opts
        A1, A2 = engine.finalmlp_gate_fwd(Xf, n_cand, (*det[1:6], p1, seed1, site1), (*det[6:11], p2, seed2, site2))
        ctx.save_for_backward(Xf, *det[1:], A1, A2)
        ctx.n_cand, ctx.opts, ctx.workspace, ctx.xshape = n_cand, opts, workspace, X.shape
        return A1, A2

    @staticmethod
    def backward(ctx, dA1, dA2):
        Xf, *par, A1, A2 = ctx.saved_tensors
        (p1, _, site1), (p2, _, site2) = ctx.opts
        # (the mask is the saved output: the backward draws nothing, so it takes no seed)
        dA1 = torch.zeros_like(A1) if dA1 is None else dA1.contiguous()
        dA2 = torch.zeros_like(A2) if dA2 is None else dA2.contiguous()
        dX, g1, g2 = engine.finalmlp_gate_bwd(Xf, ctx.n_cand, (*par[0:5], p1, None, site1), (*par[5:10], p2, None, site2), A1, dA1, A2, dA2,
                                              workspace=ctx.workspace)
        return (dX.view(ctx.xshape), None, None, None) + tuple(g1) + tuple(g2)


def _finalmlp_opts(stream):
    p, seed, site = (tuple(stream[5:]) + (0.0, None, 0)[len(stream) - 5:])
    return (float(p), seed if float(p) > 0.0 else None, int(site))


def finalmlp_gate(X, n_cand, stream1, stream2, workspace=None):
    """(A_1 [N, H_1], A_2 [N, H_2]) with A_s = drop(relu((X * 2 sigmoid(Zin_s Wg_s^T + bg_s)) W_s^T + b_s)): the last Linear + Sigmoid of
    both gate MLPs, the products with the flattened field vectors X [..., D] and the first Linear + ReLU + Dropout of mlp1 / mlp2
    (models/context/FinalMLP.py:203-220, :100-101) as ONE autograd node (one forward launch; backward: tile kernel, reduce, dZin).
    stream = (Zin [1 | B | N, G], Wg [D, G], bg [D], W [H, D], b [H][, drop_p, seed, site]); workspace: the model's
    engine.FinalMLPWorkspace, reused step after step"""
    if not X.is_cuda:
        raise RuntimeError("finalmlp_gate runs on the GPU only (no CPU path)")
    return _FinalMlpGateFn.apply(X, int(n_cand), (_finalmlp_opts(stream1), _finalmlp_opts(stream2)), workspace, *stream1[:5], *stream2[:5])


def finalmlp_gate_eval(X, n_cand, stream1, stream2):
    """the same on the evaluation path: forward only, no dropout, raises when autograd is recording"""
    ts = (X,) + tuple(stream1[:5]) + tuple(stream2[:5])
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise RuntimeError("finalmlp_gate_eval is the evaluation path and has no backward: call it under torch.no_grad() "
                           "(training goes through finalmlp_gate)")
    det = [t.detach().contiguous() for t in ts]
    return engine.finalmlp_gate_fwd(det[0].reshape(-1, det[0].shape[-1]), int(n_cand), (*det[1:6], 0.0, None, 0), (*det[6:11], 0.0, None, 0))


class _FinalMlpFusionFn(torch.autograd.Function):
    """FinalMLP's bilinear fusion (models/context/FinalMLP.py:238-249) on rc_finalmlp_fusion_fwd / _bwd; saves its inputs only.
    Capture-safe."""

    @staticmethod
    def forward(ctx, x, y, w_xy, w_x, b_x, w_y, b_y, heads, workspace):
        det = [t.detach().contiguous() for t in (x, y, w_xy, w_x, b_x, w_y, b_y)]
        xf, yf = det[0].reshape(-1, det[0].shape[-1]), det[1].reshape(-1, det[1].shape[-1])
        out = engine.finalmlp_fusion_fwd(xf, yf, *det[2:], heads)
        ctx.save_for_backward(xf, yf, det[2], det[3], det[5])
        ctx.heads, ctx.workspace, ctx.shapes = heads, workspace, (x.shape, y.shape)
        return out.view(x.shape[:-1])

    @staticmethod
    def backward(ctx, dout):
        xf, yf, w_xy, w_x, w_y = ctx.saved_tensors
        dx, dy, dw_xy, dw_x, db_x, dw_y, db_y = engine.finalmlp_fusion_bwd(xf, yf, w_xy, w_x, w_y, dout.contiguous().view(-1), ctx.heads,
                                                                          workspace=ctx.workspace)
        return dx.view(ctx.shapes[0]), dy.view(ctx.shapes[1]), dw_xy, dw_x, db_x, dw_y, db_y, None, None


def finalmlp_fusion(x, y, w_xy, w_x, b_x, w_y, b_y, heads, workspace=None):
    """w_x x + b_x + w_y y + b_y + sum_h x_h^T W_h y_h (models/context/FinalMLP.py:238-249): x [..., H1], y [..., H2], w_xy the
    reference's [heads * (H1 / heads) * (H2 / heads), 1] parameter, w_x [1, H1], w_y [1, H2], b_x, b_y [1] -> [...], ONE autograd node
    (one forward launch, one backward launch plus the fixed-order reduce)"""
    if not x.is_cuda:
        raise RuntimeError("finalmlp_fusion runs on the GPU only (no CPU path)")
    return _FinalMlpFusionFn.apply(x, y, w_xy, w_x, b_x, w_y, b_y, int(heads), workspace)


def finalmlp_fusion_eval(x, y, w_xy, w_x, b_x, w_y, b_y, heads):
    """the same on the evaluation path: forward only, raises when autograd is recording"""
    ts = (x, y, w_xy, w_x, b_x, w_y, b_y)
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise RuntimeError("finalmlp_fusion_eval is the evaluation path and has no backward: call it under torch.no_grad() "
                           "(training goes through finalmlp_fusion)")
    det = [t.detach().contiguous() for t in ts]
    out = engine.finalmlp_fusion_fwd(det[0].reshape(-1, x.shape[-1]), det[1].reshape(-1, y.shape[-1]), *det[2:], int(heads))
    return out.view(x.shape[:-1])


class _BuirLossFn(torch.autograd.Function):
    """BUIR's training step up to the loss (models/general/BUIR.py:73-110) on rc_buir_fwd / _bwd -> (loss, prediction [B, 1]).
    The prediction is marked non-differentiable: a loss built on it raises instead of training on nothing.  Backward: the forward
    values are recomputed from the saved inputs (autograd's version check refuses tables modified in between); the per-occurrence
    row gradients become dense gradients of the two online tables, the target tables get none."""

    @staticmethod
    def forward(ctx, user_online, user_target, item_online, item_target, W, b, uid, iid, workspace):
        det = [t.detach() for t in (user_online, user_target, item_online, item_target, W, b)]
        loss, pred = engine.buir_fwd(*det, uid, iid, workspace=workspace)
        ctx.save_for_backward(*det, uid, iid)
        ctx.workspace = workspace
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    def backward(ctx, g, _g_pred):
        *tables, uid, iid = ctx.saved_tensors
        gu, gi, dW, db = engine.buir_bwd(g, *tables, uid, iid, workspace=ctx.workspace)
        G_user = engine.embedding_dense_backward(gu, uid, tables[0].shape[0], route="small", small_tag="buir_user")
        G_item = engine.embedding_dense_backward(gi, iid, tables[2].shape[0], route="small", small_tag="buir_item")
        return G_user, None, G_item, None, dW, db, None, None, None


def buir_loss(user_online, user_target, item_online, item_target, W, b, uid, iid, workspace=None):
    """BUIR.forward's training branch and BUIR.loss (models/general/BUIR.py:73-110) for B (user, positive item) rows as ONE
    autograd node -> (loss, prediction [B, 1]); workspace: the model's engine.BuirWorkspace, reused step after step"""
    for t in (user_online, user_target, item_online, item_target, W, b):
        if not t.is_contiguous():
            raise ValueError("buir_loss: tables, weight and bias must be contiguous")
    return _BuirLossFn.apply(user_online, user_target, item_online, item_target, W, b, uid.reshape(-1).contiguous(),
                             iid.reshape(-1).contiguous(), workspace)


def buir_scores(user_online, item_online, W, b, uid, iid):
    """the evaluation path of BUIR.py:78-79: prediction [B, C] = <P(i_c), u> + <P(u), i_c>, as <q, i_c> + c with q = (W + W^T) u +
    b and c = <b, u> (rc_buir_query, rc_buir_scores); forward only: raises when autograd is recording"""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (user_online, item_online, W, b)):
        raise RuntimeError("buir_scores is the evaluation path and has no backward: call it under torch.no_grad() "
                           "(training goes through buir_loss)")
    q, c = engine.buir_query(user_online.detach(), W.detach(), b.detach(), uid)
    return engine.buir_scores(q, c, item_online.detach(), iid)


class _BprLossFn(torch.autograd.Function):
    """GeneralModel.loss (models/BaseModel.py:182-185), closed-form backward."""

    @staticmethod
    def forward(ctx, pred):
        loss, _, gpred = engine.bpr_loss(pred.detach().contiguous())
        ctx.save_for_backward(gpred)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        (gpred,) = ctx.saved_tensors
        return gpred * grad_loss


def bpr_loss(pred):
    return _BprLossFn.apply(pred)


class _ListLossFn(torch.autograd.Function):
    """list-wise losses of ImpressionModel.loss on the HIP engine (rc_list_loss_fwd_bwd): the list-level BPR family with
    its re-weighting variants, listnet, softmaxCE, attention_rank; closed-form backward.  kind: engine.list_kind(loss_n)"""

    @staticmethod
    def forward(ctx, pred, target, max_pos, kind):
        loss, gpred = engine.list_loss(pred.detach().contiguous(), target.contiguous(), max_pos, kind)
        ctx.save_for_backward(gpred)
        ctx.per_row = kind == engine.LIST_KINDS["BPRsimple"]   # the reference leaves this one unreduced: [B]
        return loss if ctx.per_row else loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        (gpred,) = ctx.saved_tensors
        return gpred * (grad_loss[:, None] if ctx.per_row else grad_loss), None, None, None


def list_loss(pred, target, max_pos, kind):
    return _ListLossFn.apply(pred, target, max_pos, kind)


class _FmSecondOrderFn(torch.autograd.Function):
    """0.5 * sum_k ((sum_f v)^2 - sum_f v^2) over stacked field vectors (models/context/FM.py:61)."""

    @staticmethod
    def forward(ctx, V):
        Vc = V.detach().contiguous()
        ctx.save_for_backward(Vc)
        return engine.fm_second_order(Vc)

    @staticmethod
    def backward(ctx, gout):
        (Vc,) = ctx.saved_tensors
        return engine.fm_second_order_bwd(Vc, gout.contiguous())


def fm_second_order(V):
    if not V.is_cuda:
        raise RuntimeError("fm_second_order runs on the GPU only (no CPU path)")
    return _FmSecondOrderFn.apply(V)  # float4 lane-group kernels for emb_size 16/32/64/128, a generic kernel otherwise


class _FmTapFn(torch.autograd.Function):
    """the FM pairwise term AND the flattened field vectors for a second consumer (DeepFM's deep tower, models/context/DeepFM.py:
    19-28) as one autograd node: its backward forms d fm2 / dV on top of the gradient the second consumer sends back in ONE pass
    (rc_fm_second_order_bwd with add) -- as two nodes autograd writes both gradients out and adds them (three more passes over
    [B, C, F, d])."""

    @staticmethod
    def forward(ctx, V):
        Vc = V.detach().contiguous()
        ctx.save_for_backward(Vc)
        flat = Vc.view(*Vc.shape[:-2], Vc.shape[-2] * Vc.shape[-1])
        return engine.fm_second_order(Vc), flat

    @staticmethod
    def backward(ctx, g_fm, g_flat):
        (Vc,) = ctx.saved_tensors
        if g_fm is None:
            return None if g_flat is None else g_flat.reshape(Vc.shape)
        add = None if g_flat is None else g_flat.contiguous().view(Vc.shape)
        return engine.fm_second_order_bwd(Vc, g_fm.contiguous(), add=add)


def fm_second_order_and_flat(V):
    """(fm_second_order(V), V.flatten(start_dim=-2)) as one autograd node"""
    if not V.is_cuda:
        raise RuntimeError("fm_second_order_and_flat runs on the GPU only (no CPU path)")
    return _FmTapFn.apply(V)


class _FieldGatherFn(torch.autograd.Function):
    """stacked field vectors [B, C, F, d] of F embedding tables (models/context/FM.py:49-52); the backward
    builds all F dense gradients with one sort + one segmented sum over the composite (field, id) key."""

    # Two table families gathered with the SAME id tensors (FM-family models: the [vocab, d] vectors and the [vocab, 1] first-order
    # weights of every field, models/context/FM.py:44-57) share the composite keys and, in the backward pass, their sort: the
    # last forward's (ids, key tensor) and the last backward's sorted keys are remembered.  The entries hold the tensors
    # themselves (identity + version are compared, never addresses: a freed tensor's address can come back).
    _last_cid = None      # (ids tuple, versions, n_cand, offsets, cid)
    _last_sort = None     # (cid, n_rows, keys, perm)
    _last_small = None    # (cid, n_rows): the small route's grouping of these keys sits in the workspace "edb_small_fields"

    @staticmethod
    def forward(ctx, n_cand, n_fields, *args):
        ids, tables = args[:n_fields], args[n_fields:]
        ids_c = [x.contiguous() for x in ids]
        offs_now = [0]
        for t in tables:
            offs_now.append(offs_now[-1] + t.shape[0])
        # The caches live for ONE forward / backward of a model: a hit consumes the entry, a backward drops it, and nothing is
        # remembered without autograd (an evaluation loop over a static id buffer rewritten through raw pointers -- which
        # does not bump _version -- can therefore never meet a stale key tensor).
        last = _FieldGatherFn._last_cid
        _FieldGatherFn._last_cid = None
        hit = (last is not None and len(last[0]) == len(ids_c) and all(a is b for a, b in zip(last[0], ids_c))
               and last[1] == tuple(x._version for x in ids_c) and last[2] == n_cand and last[3] == offs_now)
        res = engine.gather_fields([t.detach() for t in tables], ids_c, n_cand, want_cid=not hit)
        out, cid, offs = res.out, res.cid, res.offsets
        if hit:
            cid = last[4]
        else:
            _FieldGatherFn._last_sort = None
            _FieldGatherFn._last_small = None
            if torch.is_grad_enabled():
                _FieldGatherFn._last_cid = (tuple(ids_c), tuple(x._version for x in ids_c), n_cand, offs_now, cid)
        ctx.cid, ctx.offs = cid, offs
        # a field whose vocabulary is small against the batch makes hot rows: the sort-driven reduction handles any skew
        n_ids = cid.numel() // max(1, n_fields)
        # (a field value occurs at most once per row: up to 8,192 ids in all the small route fits whatever the vocabularies)
        ctx.route = "small" if cid.numel() <= 8192 else ("sort" if min(t.shape[0] for t in tables) * 8 <= n_ids else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        offs = ctx.offs
        presorted = None
        _FieldGatherFn._last_cid = None     # the forward this belongs to is over
        if ctx.route == "sort":
            last = _FieldGatherFn._last_sort
            if last is not None and last[0] is ctx.cid and last[1] == offs[-1]:
                presorted = last[2:]
                _FieldGatherFn._last_sort = None    # second (last) user of this sort
            else:
                presorted = engine.sort_ids(ctx.cid.reshape(-1), offs[-1])
                _FieldGatherFn._last_sort = (ctx.cid, offs[-1]) + tuple(presorted)
        again = False
        if ctx.route == "small" and engine.small_route_ok(ctx.cid.numel(), offs[-1], gout.shape[-1]):
            # the small route groups the composite keys in its first launch: the second family gathered with the same keys
            # (same key tensor, nothing else used that workspace in between: it has a tag of its own) runs the sums only
            last = _FieldGatherFn._last_small
            again = last is not None and last[0] is ctx.cid and last[1] == offs[-1]
            _FieldGatherFn._last_small = None if again else (ctx.cid, offs[-1])
        G = engine.embedding_dense_backward(gout.contiguous(), ctx.cid, offs[-1], route=ctx.route, presorted=presorted,
                                            small_again=again, small_tag="edb_small_fields")  # virtual concatenated table
        grads = tuple(G[offs[f]:offs[f + 1]] for f in range(len(offs) - 1))
        return (None, None) + (None,) * len(grads) + grads


def gather_fields(tables, ids, n_cand):
    """tables: F HipEmbedding weights of equal width; ids: F int64 tensors ([B] or [B, C])"""
    return _FieldGatherFn.apply(n_cand, len(tables), *ids, *tables)


class _FieldGatherKindsFn(torch.autograd.Function):
    """ONE table family with numeric fields among the categorical ones (models/context/FinalMLP.py:57-60,79-92: `embedding_dict`
    holds nn.Embedding and Linear(1, d, bias=False) side by side): the same gather launch as the pair's (rc_gather_fields' kinds,
    no second family); backward, one sort of the composite keys with the numeric occurrences behind every row + one segmented sum,
    and rc_numeric_field_grads on gV alone for the Linear weights."""

    @staticmethod
    def forward(ctx, n_cand, n_fields, kinds, *args):
        ids = [x.contiguous() for x in args[:n_fields]]
        tables = args[n_fields:]
        cat = [f for f in range(n_fields) if kinds[f] == engine.FIELD_IDS]
        num = [f for f in range(n_fields) if kinds[f] != engine.FIELD_IDS]
        n_rows = sum(tables[f].shape[0] for f in cat)
        res = engine.gather_fields([t.detach() for t in tables], ids, n_cand, want_cid=True, kinds=kinds, numeric_key=n_rows)
        ctx.cid, ctx.offs, ctx.kinds, ctx.num, ctx.n_cand = res.cid, res.offsets, kinds, num, n_cand
        ctx.values = [ids[f] for f in num]
        return res.out

    @staticmethod
    def backward(ctx, gV):
        offs, num, F = ctx.offs, ctx.num, len(ctx.kinds)
        n_rows, n = offs[-1], ctx.cid.numel()
        gV = gV.contiguous()
        d = gV.shape[-1]
        gw, _ = engine.numeric_field_grads(gV.view(n // F, F, d), None, ctx.values, num, F, ctx.n_cand, d)
        G = None
        if n_rows > 0:
            keys, perm = engine.sort_ids(ctx.cid.reshape(-1), n_rows + 1)
            n_cat = (n // F) * (F - len(num))
            G = engine.embedding_dense_backward(gV, ctx.cid, n_rows, route="sort", presorted=(keys[:n_cat], perm[:n_cat]))
        grads = [None if ctx.kinds[f] != engine.FIELD_IDS else G[offs[f]:offs[f + 1]] for f in range(F)]
        for j, f in enumerate(num):
            grads[f] = gw[j]
        return (None, None, None) + (None,) * F + tuple(grads)


def gather_fields_kinds(tables, ids, n_cand, kinds=None):
    """gather_fields for ONE table family that may hold numeric fields: kinds[f] is engine.FIELD_IDS (tables[f] a [vocab, d] table
    looked up by ids[f]) or the value type of a numeric field (engine.field_kind; tables[f] the Linear(1, d, bias=False) weight
    [d, 1], ids[f] the feature's values).  kinds None / all ids: exactly gather_fields"""
    if kinds is None or all(k == engine.FIELD_IDS for k in kinds):
        return gather_fields(tables, ids, n_cand)
    return _FieldGatherKindsFn.apply(n_cand, len(tables), tuple(int(k) for k in kinds), *ids, *tables)


class _FieldGatherPairFn(torch.autograd.Function):
    """the TWO table families the FM models gather with the same ids (models/context/FM.py:44-57: field vectors [vocab, d] and
    first-order weights [vocab, 1]) as one autograd node: one gather launch forward (rc_gather_fields with tables1); backward, ONE
    grouping of the composite (field, id) keys serves both dense gradients -- the small route's plan (rc_small_row_sums, then
    rc_small_row_sums_planned where the second does not ride, on one zero-filled buffer), or one sort -- instead of one per family.
    Numeric fields (kinds[f] != 0; FM.py:38-41,47-48: Linear(1, d) / Linear(1, 1) on the feature's value) ride in the same gather
    launch (rc_gather_fields' kind: their "row" is x * W[:, 0]); they own no row of the concatenated table, their occurrences
    take no part in the grouping, and their weight gradients are one weighted column sum (rc_numeric_field_grads)."""

    @staticmethod
    def forward(ctx, n_cand, n_fields, rows_opt, kinds, want_fm, bump, *args):
        ids = [x.contiguous() for x in args[:n_fields]]
        tables, tables1 = args[n_fields:2 * n_fields], args[2 * n_fields:]
        kinds = tuple(kinds) if kinds is not None else (engine.FIELD_IDS,) * n_fields
        cat = [f for f in range(n_fields) if kinds[f] == engine.FIELD_IDS]
        num = [f for f in range(n_fields) if kinds[f] != engine.FIELD_IDS]
        d = tables[cat[0]].shape[1] if cat else tables[0].shape[0]
        rows = ids[0].shape[0] * n_cand
        n = rows * n_fields
        n_rows = sum(tables[f].shape[0] for f in cat)
        mark = None
        if rows_opt is not None and cat and n <= 8192 and d % 4 == 0 and engine.small_route_ok(n, n_rows, d):
            # rows mode (HipOptimizer.rows_begin): the gather stamps the looked-up rows, and the backward pass below hands their row
            # sums to the optimizer in a scratch that nothing zero-fills, instead of a dense gradient
            mark = rows_opt.rows_begin([tables[f] for f in cat], [tables1[f] for f in cat])
        n_ids = rows
        ctx.route = "small" if n <= 8192 else ("sort" if cat and min(tables[f].shape[0] for f in cat) * 8 <= n_ids else None)
        if num and not (ctx.route == "small" and engine.small_route_ok(n, max(n_rows, 1), d)):
            ctx.route = "sort"    # (the other groupings of embedding_dense_backward have no key that stands for "no row")
        # what the numeric occurrences carry in cid: the small route and the bucket plan skip negative keys; a sort puts the key
        # past the last row behind every real row (the grouping below stops in front of that tail)
        numeric_key = n_rows if (ctx.route == "sort" and num) else -1
        fusable = d in (16, 32, 64, 128)
        # small batches: the backward pass's grouping of the composite keys depends on the ids alone -- it runs in the gather's
        # launch (rc_gather_fields_fused) instead of as a launch of its own in front of the row sums
        plan = bool(fusable and cat and ctx.route == "small" and any(ctx.needs_input_grad) and engine.small_route_ok(n, n_rows, d))
        fm_here = bool(want_fm and fusable)
        V, L, cid, offs, fm, S, plan_ws = engine.gather_fields([t.detach() for t in tables], ids, n_cand, want_cid=True,
                                                               tables1=[t.detach() for t in tables1], mark=mark, kinds=kinds,
                                                               numeric_key=numeric_key, fm=fm_here, plan=plan,
                                                               bump=bump if (plan or fm_here) else None)
        if want_fm and fm is None:
            fm = engine.fm_second_order(V)      # (a width without the float4 lane-group tiling: its own launch)
        ctx.rows_opt = rows_opt if mark is not None else None
        ctx.cid, ctx.offs, ctx.d = cid, offs, d
        ctx.kinds, ctx.num, ctx.n_cand = kinds, num, n_cand
        ctx.values = [ids[f] for f in num]
        ctx.want_fm, ctx.plan_ws = bool(want_fm), plan_ws
        ctx.has_S = S is not None
        ctx.set_materialize_grads(False)
        if want_fm:
            ctx.save_for_backward(*((V, S) if S is not None else (V,)))
            return V, L, fm
        return V, L

    @staticmethod
    def backward(ctx, gV, gL, g_fm=None):
        offs, d = ctx.offs, ctx.d
        n_rows, n = offs[-1], ctx.cid.numel()
        F = len(offs) - 1
        gV = None if gV is None else gV.contiguous()
        gL = None if gL is None else gL.contiguous()
        num = ctx.num
        gw = gw1 = None
        small = ctx.route == "small" and n_rows > 0 and d % 4 == 0 and engine.small_route_ok(n, n_rows, d)
        planned = small and ctx.plan_ws is not None and gL is not None
        # the FM term's backward: added to the tower's gradient rows where the row sums read them (planned small route: never
        # written out), else one pass of its own (rc_fm_second_order_bwd with add)
        tap = None
        if ctx.want_fm and g_fm is not None:
            saved = ctx.saved_tensors
            Vs = saved[0]
            rideable = (not num) or (16 <= d <= 128 and len(num) <= engine.SMALL_NUMERIC_MAX)
            if planned and ctx.has_S and rideable:
                tap = (Vs.view(n // F, F, d), saved[1].view(n // F, d), g_fm.contiguous().view(-1))
            else:
                gV = engine.fm_second_order_bwd(Vs, g_fm.contiguous(), add=None if gV is None else gV.view(Vs.shape))
        have_v = gV is not None or tap is not None
        # small batches: the numeric fields' weight gradients ride in the row-sums launch of the small route (a launch of their own
        # is ~13 us of a replayed DeepFM step at B = 1,024); otherwise rc_numeric_field_grads on its own
        ride = (num and have_v and gL is not None and small and 16 <= d <= 128
                and len(num) <= engine.SMALL_NUMERIC_MAX)
        riding = (ctx.values, num, F, ctx.n_cand) if ride else None
        if num and not ride and (gV is not None or gL is not None):
            gw, gw1 = engine.numeric_field_grads(None if gV is None else gV.view(n // F, F, d), None if gL is None else gL.view(n // F, F),
                                                 ctx.values, num, F, ctx.n_cand, d)

        def numeric(grads, family):
            """the tables' gradient tuple with the numeric fields' Linear weights filled in"""
            if family is None:
                return grads
            out = list(grads)
            for j, f in enumerate(num):
                out[f] = family[j]
            return tuple(out)

        def row_sums(into=None):
            """(Gv, Gl) of the small route; the numeric fields' gradients land in gw / gw1 when they ride"""
            nonlocal gw, gw1
            if planned and have_v:
                res = engine.small_row_sums_planned(ctx.plan_ws, n, n_rows, None if gV is None else gV.view(n, d), gL.view(n, 1), d,
                                                    (F, n // (F * ctx.n_cand), ctx.n_cand), into=into, numeric=riding, fm=tap)
            else:
                res = engine.small_row_sums_pair(ctx.cid, n_rows, gV.view(n, d), gL.view(n, 1), into=into, numeric=riding)
            if ride:
                gw, gw1 = res[2:]
            return res[:2]

        lead = (None,) * 6
        if ctx.rows_opt is not None:
            if not have_v or gL is None:
                raise RuntimeError("gather_fields_pair (rows mode): both table families must reach the loss")
            Gv, Gl = row_sums(into=ctx.rows_opt.rows_scratch())
            ctx.rows_opt.rows_grads(Gv, Gl)
            return lead + (None,) * F + numeric((None,) * F, gw) + numeric((None,) * F, gw1)
        if n_rows == 0:       # numeric fields only
            Gv = Gl = None
        elif have_v and gL is not None and small:
            Gv, Gl = row_sums()
        else:
            presorted = None
            if ctx.route == "sort":
                # the numeric occurrences (key n_rows) sort behind every row of the virtual table: the grouping takes the head
                keys, perm = engine.sort_ids(ctx.cid.reshape(-1), n_rows + (1 if num else 0))
                n_cat = (n // F) * (F - len(num))
                presorted = (keys[:n_cat], perm[:n_cat])
            Gv = None if gV is None else engine.embedding_dense_backward(gV, ctx.cid, n_rows, route=ctx.route, presorted=presorted)
            Gl = None if gL is None else engine.embedding_dense_backward(gL, ctx.cid, n_rows, route=ctx.route, presorted=presorted)
        cat = lambda G, f: None if (G is None or ctx.kinds[f] != engine.FIELD_IDS) else G[offs[f]:offs[f + 1]]
        gv = numeric(tuple(cat(Gv, f) for f in range(F)), gw)
        gl = numeric(tuple(cat(Gl, f) for f in range(F)), gw1)
        return lead + (None,) * F + gv + gl


def gather_fields_pair(tables, tables1, ids, n_cand, rows_opt=None, kinds=None, fm=False, bump=None):
    """-> (field vectors [B, C, F, d], first-order values [B, C, F, 1]) of the two table families looked up with the same ids.
    fm=True: -> (vectors, values, FM pairwise term [B, C]) -- models/context/FM.py:61's 0.5 sum_k ((sum_f v)^2 - sum_f v^2) formed
    in the gather's launch; its backward is added to the vectors' other gradient (DeepFM's tower) where the row sums read it.
    bump: an int64 [1] device counter whose next engine.step_increment the gather's launch performs early, where it has a slot for
    it (the dropout seed of the tower that consumes the vectors: one one-thread launch fewer per step); nothing the gather launches
    may read it.
    rows_opt: the HipOptimizer that owns the tables, when this forward is part of a whole training step whose optimizer.step()
    follows (graph.GraphedStep sets it): small batches then take the optimizer's rows mode.
    kinds: per field engine.FIELD_IDS (a table looked up by ids) or the value type of a numeric field (engine.field_kind): then
    tables[f] / tables1[f] are the weights of its Linear(1, d) / Linear(1, 1) and ids[f] holds the feature's values"""
    return _FieldGatherPairFn.apply(n_cand, len(tables), rows_opt, None if kinds is None else tuple(kinds), bool(fm), bump, *ids, *tables, *tables1)


class _BceProbFn(torch.autograd.Function):
    """nn.BCELoss on probabilities (models/BaseModel.py:259-267), closed-form backward."""

    @staticmethod
    def forward(ctx, p, y):
        loss, gp = engine.bce_prob(p.detach().contiguous(), y.detach().contiguous().float())
        ctx.save_for_backward(gp)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        (gp,) = ctx.saved_tensors
        return gp * grad_loss, None


def bce_loss(p, y):
    return _BceProbFn.apply(p, y)


UNIT_LOSS_GRAD = None     # float32 scalar buffer holding 1.0 that the step in progress seeds loss.backward() with (graph.GraphedStep)


class _CtrHeadFn(torch.autograd.Function):
    """the CTR head of the context models in training: logit = bias + first-order sum (+ pairwise term) (+ MLP output), sigmoid,
    nn.BCELoss -- one kernel forward, the closed-form d loss / d logit fanned out to the terms backward."""

    @staticmethod
    def forward(ctx, bias, lin, label, *terms):
        n = label.numel()
        t = [x.detach().reshape(-1).contiguous() for x in terms]
        lin2 = lin.detach().reshape(n, -1).contiguous()
        ctx.lin_shape, ctx.term_shapes = lin.shape, [x.shape for x in terms]
        ctx.one_wg = n <= engine.CTR_HEAD_ONE_WG_MAX and lin2.numel() == lin.numel()
        ctx.set_materialize_grads(False)    # p is not differentiable: no [n] block of zeros is filled for it in every backward pass
        if ctx.one_wg:
            # one workgroup: probabilities, loss MEAN and sum gz (the bias gradient) in the same launch.  Inside a whole training
            # step whose backward is seeded with the constant 1 (graph.GraphedStep announces its buffer: UNIT_LOSS_GRAD) the launch
            # also leaves the backward fan-out and takes Adam's pending step-count increment along
            ctx.full = UNIT_LOSS_GRAD is not None and UNIT_LOSS_GRAD.device == lin2.device
            res = engine.ctr_head_sums(bias.detach(), lin2, t[0] if len(t) > 0 else None, t[1] if len(t) > 1 else None,
                                       label.reshape(-1).contiguous(), full=ctx.full)
            p, sums, gz = res[:3]
            ctx.save_for_backward(gz, sums, *res[3:])
            ctx.mark_non_differentiable(p)
            return p, sums[0].reshape(())
        p, loss, gz = engine.ctr_head(bias.detach(), lin2, t[0] if len(t) > 0 else None,
                                      t[1] if len(t) > 1 else None, label.reshape(-1).contiguous())
        ctx.save_for_backward(gz)
        ctx.mark_non_differentiable(p)
        return p, loss.reshape(())

    @staticmethod
    def backward(ctx, _gp, g_loss):
        if g_loss is None:      # the loss did not reach the objective
            return (None, None, None) + (None,) * len(ctx.term_shapes)
        if ctx.one_wg:
            gz, sums = ctx.saved_tensors[:2]
            n = gz.shape[0]
            unit = UNIT_LOSS_GRAD
            if ctx.full and unit is not None and g_loss.data_ptr() == unit.data_ptr() and g_loss.numel() == 1:
                g_lin, g_bias = ctx.saved_tensors[2:]       # the forward launch wrote them for exactly this seed
                return (g_bias, g_lin.view(ctx.lin_shape), None) + tuple(gz.reshape(sh) for sh in ctx.term_shapes)
            # one launch: g = gz * g_loss for the terms, the contiguous [n, F] block of the first-order weights, the bias gradient
            g, g_lin, g_bias = engine.ctr_head_bwd(gz, sums, g_loss.reshape(1).float().contiguous(), ctx.lin_shape.numel() // n)
            return (g_bias, g_lin.view(ctx.lin_shape), None) + tuple(g.reshape(sh) for sh in ctx.term_shapes)
        (gz,) = ctx.saved_tensors
        g = gz * g_loss
        n = g.shape[0]
        g_lin = g.reshape(n, *([1] * (len(ctx.lin_shape) - 1))).expand(ctx.lin_shape)
        return (g.sum().reshape(1), g_lin, None) + tuple(g.reshape(sh) for sh in ctx.term_shapes)


def ctr_head(bias, lin, label, terms):
    """-> (p [n] probabilities, BCE loss scalar); lin: first-order values [n, ..., F] (summed over the trailing dims per row),
    terms: up to two tensors of n elements added to the logit"""
    if not lin.is_cuda:
        raise RuntimeError("ctr_head runs on the GPU only (no CPU path)")
    assert len(terms) <= 2
    return _CtrHeadFn.apply(bias, lin, label, *terms)


class _BceRankingFn(torch.autograd.Function):
    """ContextModel.loss, loss_n 'BCE' (models/BaseContextModel.py:53-56), closed-form backward"""

    @staticmethod
    def forward(ctx, pred):
        loss, gpred = engine.bce_ranking(pred.detach().contiguous())
        ctx.save_for_backward(gpred)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        (gpred,) = ctx.saved_tensors
        return gpred * grad_loss


def bce_ranking_loss(pred):
    return _BceRankingFn.apply(pred)


class _NeumfFn(torch.autograd.Function):
    """NeuMF head, one hidden layer (models/general/NeuMF.py:61-75): rc_neumf_fwd / rc_neumf_bwd."""

    @staticmethod
    def forward(ctx, mf_u, mf_i, mlp_u, mlp_i, W1, b1, w_out, uid, iid, drop_p=0.0, seed=None):
        P = {"mf_u": mf_u.detach(), "mf_i": mf_i.detach(), "mlp_u": mlp_u.detach(), "mlp_i": mlp_i.detach(),
             "W1": W1.detach().contiguous(), "b1": b1.detach().contiguous(),
             "w_out": w_out.detach().reshape(-1).contiguous()}
        ctx.P, ctx.uid, ctx.iid, ctx.wshape = P, uid, iid, w_out.shape
        ctx.drop = (drop_p, seed)  # the backward regenerates the mask from the same device seed
        return engine.neumf_fwd(P, uid, iid, drop_p, seed)

    @staticmethod
    def backward(ctx, gpred):
        P, uid, iid = ctx.P, ctx.uid, ctx.iid
        rows, dense = engine.neumf_bwd(P, uid, iid, gpred.contiguous(), *ctx.drop)
        uid_occ = uid.repeat_interleave(iid.shape[1])
        ku, pu = engine.sort_ids(uid_occ, P["mf_u"].shape[0])
        ki, pi = engine.sort_ids(iid, P["mf_i"].shape[0])

        # the mf / mlp tables of a side share ids: one sort and one head list serve both
        _, hu, nhu = engine.segment_heads(ku, pu, want_single=False)
        _, hi, nhi = engine.segment_heads(ki, pi, want_single=False)

        def dense_pair(ta, tb, ga, gb, keys, perm, heads, n_heads):  # one pass over the ids for both tables
            Ga, Gb = torch.zeros_like(P[ta]), torch.zeros_like(P[tb])
            if engine.segmented_pair_supported(P[ta].shape[1]):
                engine.segmented_update_pair(keys, perm, rows[ga], rows[gb], dense_grad=(Ga, Gb), heads=heads, n_heads=n_heads)
            else:
                engine.segmented_update(keys, perm, rows[ga], dense_grad=Ga, heads=heads, n_heads=n_heads)
                engine.segmented_update(keys, perm, rows[gb], dense_grad=Gb, heads=heads, n_heads=n_heads)
            return Ga, Gb
        g_mf_u, g_mlp_u = dense_pair("mf_u", "mlp_u", "g_mf_u", "g_mlp_u", ku, pu, hu, nhu)
        g_mf_i, g_mlp_i = dense_pair("mf_i", "mlp_i", "g_mf_i", "g_mlp_i", ki, pi, hi, nhi)
        return (g_mf_u, g_mf_i, g_mlp_u, g_mlp_i,
                dense["W1"], dense["b1"], dense["w_out"].view(ctx.wshape), None, None, None, None)


def neumf_scores(mf_u, mf_i, mlp_u, mlp_i, W1, b1, w_out, uid, iid, drop_p=0.0, seed=None):
    """drop_p > 0 (training): hidden-layer dropout inside the kernels; `seed` int64 [1] device tensor the caller
    bumps once per forward (engine.step_increment)"""
    return _NeumfFn.apply(mf_u, mf_i, mlp_u, mlp_i, W1, b1, w_out, uid.contiguous(), iid.contiguous(), drop_p, seed)


_SAS_ATTRS = (("Wq", "masked_attn_head.q_linear.weight"), ("bq", "masked_attn_head.q_linear.bias"),
              ("Wk", "masked_attn_head.k_linear.weight"), ("bk", "masked_attn_head.k_linear.bias"),
              ("Wv", "masked_attn_head.v_linear.weight"), ("bv", "masked_attn_head.v_linear.bias"),
              ("ln1w", "layer_norm1.weight"), ("ln1b", "layer_norm1.bias"), ("W1", "linear1.weight"),
              ("b1", "linear1.bias"), ("W2", "linear2.weight"), ("b2", "linear2.bias"),
              ("ln2w", "layer_norm2.weight"), ("ln2b", "layer_norm2.bias"))


def _get_attr(mod, path):
    for part in path.split("."):
        mod = getattr(mod, part)
    return mod


class _SasrecEncodeFn(torch.autograd.Function):
    """SASRec encoder (models/sequential/SASRec.py:58-76): rc_sasrec_fwd / rc_sasrec_bwd.
    Inputs: item table, position table, then 14 parameters per block in engine.SAS_LAYER_KEYS order."""

    @staticmethod
    def forward(ctx, item_emb, pos_emb, n_heads, hist, lengths, drop_p, seed, *flat):
        n_layers = len(flat) // 14
        layers = [{k: flat[14 * l + j].detach().contiguous() for j, (k, _) in enumerate(_SAS_ATTRS)}
                  for l in range(n_layers)]
        need_grad = any(t.requires_grad for t in (item_emb, pos_emb) + tuple(flat))
        hv, xsave = engine.sasrec_fwd(item_emb.detach(), pos_emb.detach(), layers, n_heads, hist, lengths,
                                      save=need_grad, drop_p=drop_p, seed=seed)
        ctx.layers, ctx.n_heads, ctx.hist, ctx.lengths, ctx.xsave = layers, n_heads, hist, lengths, xsave
        ctx.drop_p, ctx.seed = drop_p, seed
        ctx.n_items, ctx.n_pos = item_emb.shape[0], pos_emb.shape[0]
        return hv

    @staticmethod
    def backward(ctx, dhv):
        hist, lengths = ctx.hist, ctx.lengths
        g_hist, dgrads = engine.sasrec_bwd(ctx.layers, ctx.n_heads, lengths, ctx.xsave, dhv.contiguous(),
                                           drop_p=ctx.drop_p, seed=ctx.seed)
        GI = engine.embedding_dense_backward(g_hist, hist, ctx.n_items)
        GP = engine.sasrec_pos_grad(g_hist, lengths, ctx.n_pos)
        flat = [g[k].contiguous() for g in dgrads for k, _ in _SAS_ATTRS]
        return (GI, GP, None, None, None, None, None) + tuple(flat)


def sasrec_layer_params(blocks):
    """[{engine.SAS_LAYER_KEYS name: parameter storage}] of utils.layers.TransformerLayer blocks (no copies)"""
    return [{k: _get_attr(b, path).data for k, path in _SAS_ATTRS} for b in blocks]


def sasrec_encode(item_emb, pos_emb, blocks, n_heads, hist, lengths, drop_p=0.0, seed=None):
    """blocks: nn.ModuleList of utils.layers.TransformerLayer (parameters only are used).  drop_p > 0 (training):
    dropout1 / dropout2 of every block inside the batch-level kernels; `seed` int64 [1] device tensor the caller
    bumps once per forward (engine.step_increment)"""
    flat = [_get_attr(b, path) for b in blocks for _, path in _SAS_ATTRS]
    return _SasrecEncodeFn.apply(item_emb, pos_emb, n_heads, hist.contiguous(), lengths.contiguous(), float(drop_p), seed, *flat)


# ---- the encoder layer by layer, any shape (csrc/seq_layers.hip + the GEMMs of csrc/mlp.hip) ---------------------------------

class _SeqEmbedFn(torch.autograd.Function):
    """item rows + position rows of a right-padded history as B * L rows, position id = length - index (SASRec.py:58-66) or, with
    fwdpos, the index itself (ContraRec.py:259-267); the backward is the two dense embedding gradients (the rows' gradients are
    zero on the padding)"""

    @staticmethod
    def forward(ctx, item_emb, pos_emb, hist, lengths, fwdpos):
        ctx.hist, ctx.lengths, ctx.fwdpos = hist, lengths, fwdpos
        ctx.n_items, ctx.n_pos = item_emb.shape[0], pos_emb.shape[0]
        embed = engine.seq_embed_fwdpos if fwdpos else engine.seq_embed
        return embed(item_emb.detach(), pos_emb.detach(), hist, lengths)

    @staticmethod
    def backward(ctx, gX):
        B, L = ctx.hist.shape
        g = gX.contiguous()
        GI = engine.embedding_dense_backward(g.view(B, L, -1), ctx.hist, ctx.n_items)
        pos_grad = engine.seq_pos_grad_fwdpos if ctx.fwdpos else engine.seq_pos_grad
        GP = pos_grad(g, ctx.lengths, B, L, ctx.n_pos)
        return GI, GP, None, None, None


class _SeqAttentionFn(torch.autograd.Function):
    """scaled_dot_product_attention of every head (utils/layers.py:52-63) on Q / K / V [B * L, H * dk]; nothing of size L x L is
    kept: the backward recomputes the probabilities from the saved log-sum-exp"""

    @staticmethod
    def forward(ctx, q, k, v, off, B, L, H, mask, causal):
        qc, kc, vc = q.detach().contiguous(), k.detach().contiguous(), v.detach().contiguous()
        out, lse = engine.seq_attention_fwd(qc, kc, vc, off, B, L, H, mask=mask, causal=causal)
        ctx.save_for_backward(qc, kc, vc, lse)
        ctx.args = (off, B, L, H, mask, causal)
        return out

    @staticmethod
    def backward(ctx, dctx):
        qc, kc, vc, lse = ctx.saved_tensors
        off, B, L, H, mask, causal = ctx.args
        dQ, dK, dV = engine.seq_attention_bwd(qc, kc, vc, off, B, L, H, lse, dctx.contiguous(), mask=mask, causal=causal)
        return dQ, dK, dV, None, None, None, None, None, None


class _AddLayerNormFn(torch.autograd.Function):
    """LayerNorm(dropout(branch) + residual) (utils/layers.py:110,117) in one kernel each way; the dropout mask is the
    counter-based stream of the batch encoder (never stored)"""

    @staticmethod
    def forward(ctx, a, r, w, b, off, L, drop_p, seed, site):
        ac = a.detach().contiguous()
        y, xhat, rstd = engine.seq_add_layernorm_fwd(ac, None if r is None else r.detach().contiguous(), w.detach(), b.detach(), off, L,
                                                     drop_p, seed, site)
        ctx.save_for_backward(xhat, rstd, w.detach())
        ctx.args = (off, L, drop_p, seed, site, r is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        xhat, rstd, w = ctx.saved_tensors
        off, L, drop_p, seed, site, has_r = ctx.args
        dA, dR, dw, db = engine.seq_add_layernorm_bwd(dy.contiguous(), xhat, rstd, w, off, L, drop_p, seed, site, need_dR=has_r)
        return dA, dR, dw, db, None, None, None, None, None


class _SeqPickLastFn(torch.autograd.Function):
    """hv[b] = x[b, len_b - 1] (SASRec.py:76)"""

    @staticmethod
    def forward(ctx, x, lengths, B, L):
        ctx.args = (lengths, B, L)
        return engine.seq_pick_last(x.detach().contiguous(), lengths, B, L)

    @staticmethod
    def backward(ctx, dhv):
        lengths, B, L = ctx.args
        return engine.seq_pick_last_bwd(dhv.contiguous(), lengths, B, L), None, None, None


def _encode_layers(fwdpos, causal, item_emb, pos_emb, blocks, n_heads, hist, lengths, drop_p, seed):
    """the layer loop both encoders share: the embedding with either position rule, the TransformerLayers with the causal mask or
    with the key-padding mask alone, the row at position length - 1"""
    hist, lengths = hist.contiguous(), lengths.contiguous()
    B, L = hist.shape
    off = engine.seq_offsets(lengths, L)
    x = _SeqEmbedFn.apply(item_emb, pos_emb, hist, lengths, fwdpos)
    for l, blk in enumerate(blocks):
        a = blk.masked_attn_head
        q = linear(x, a.q_linear.weight, a.q_linear.bias)
        k = linear(x, a.k_linear.weight, a.k_linear.bias)
        v = linear(x, a.v_linear.weight, a.v_linear.bias)
        c = _SeqAttentionFn.apply(q, k, v, off, B, L, n_heads, None, causal)
        y1 = _AddLayerNormFn.apply(c, x, blk.layer_norm1.weight, blk.layer_norm1.bias, off, L, float(drop_p), seed, 2 * l)
        h = linear(y1, blk.linear1.weight, blk.linear1.bias, relu=True)
        f = linear(h, blk.linear2.weight, blk.linear2.bias)
        x = _AddLayerNormFn.apply(f, y1, blk.layer_norm2.weight, blk.layer_norm2.bias, off, L, float(drop_p), seed, 2 * l + 1)
    return _SeqPickLastFn.apply(x, lengths, B, L)


def sasrec_encode_layers(item_emb, pos_emb, blocks, n_heads, hist, lengths, drop_p=0.0, seed=None):
    """The SASRec encoder (SASRec.py:58-76) block by block for the shapes outside the register-resident kernels' envelope
    (engine.sasrec_supported): embeddings, every Linear (fp32 MFMA GEMMs, bias / ReLU in the epilogue), the attention of every
    head, LayerNorm(dropout(.) + residual) -- all HIP kernels, autograd only strings them together.  -> hv [B, d], the output
    row at position length - 1 of every sequence"""
    return _encode_layers(False, True, item_emb, pos_emb, blocks, n_heads, hist, lengths, drop_p, seed)   # causal mask only (SASRec.py:69-70)


def bert4rec_encode_layers(item_emb, pos_emb, blocks, n_heads, hist, lengths):
    """ContraRec's BERT4RecEncoder (ContraRec.py:259-276) on the same kernels: position id = index, no causal mask (a valid row
    attends to every valid row of its sequence: `off` restricts queries and keys alike), no dropout.  -> hv [B, d]"""
    return _encode_layers(True, False, item_emb, pos_emb, blocks, n_heads, hist, lengths, 0.0, None)


class _ContraLossFn(torch.autograd.Function):
    """ContraLoss behind F.normalize (ContraRec.py:92,142-193) on rc_contra_loss_fwd / _bwd: va, vb [B, d] un-normalised, labels
    int64 [B] or None.  Backward: the two [B, d] gradients of the views."""

    @staticmethod
    def forward(ctx, va, vb, labels, temperature, workspace):
        ws = workspace if workspace is not None else engine.ContraWorkspace()
        loss, buf, gen = engine.contra_loss_fwd(va.detach(), vb.detach(), labels, temperature, workspace=ws)
        ctx.buf, ctx.gen, ctx.workspace, ctx.labels = buf, gen, ws, labels
        ctx.batch, ctx.d, ctx.temperature = va.shape[0], va.shape[1], temperature
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        if ctx.workspace.generation != ctx.gen:
            raise RuntimeError("contra_loss: another contra_loss forward ran on this workspace before this backward; give each "
                               "pending loss a workspace of its own (rechorus_amd.engine.ContraWorkspace)")
        ga, gb = engine.contra_loss_bwd(g, ctx.labels, ctx.batch, ctx.d, ctx.temperature, ctx.buf)
        return ga, gb, None, None, None


def contra_loss(va, vb, labels, temperature, workspace=None):
    """ContraRec's context-context loss (ContraRec.py:92,102,142-193) of the two views' encoder outputs [B, d] as ONE autograd
    node; labels None: InfoNCE; workspace: the model's engine.ContraWorkspace, reused step after step (None: a fresh one)"""
    if not va.is_cuda:
        raise RuntimeError("contra_loss runs on the GPU only (no CPU path)")
    labels = None if labels is None else labels.contiguous()
    return _ContraLossFn.apply(va.contiguous(), vb.contiguous(), labels, float(temperature), workspace)


def sasrec_layers_supported(d, n_heads, L):
    """sasrec_encode_layers covers this shape: emb_size a multiple of 4 up to 1,024 whose heads divide it, history up to 1,024"""
    return d % 4 == 0 and 4 <= d <= 1024 and n_heads >= 1 and d % n_heads == 0 and engine.seq_attention_supported(L, d // n_heads)


class _LinearFn(torch.autograd.Function):
    """drop(relu(x W^T + b)) as one fp32 MFMA GEMM with the epilogue fused (rc_linear_fwd); backward = mask + two GEMMs
    (rc_linear_bwd).  The saved output is its own ReLU / dropout mask."""

    @staticmethod
    def forward(ctx, x, W, b, relu, drop_p, seed, site):
        xs = x.detach().reshape(-1, x.shape[-1]).contiguous()
        Wd = W.detach().contiguous()
        y = engine.linear_fwd(xs, Wd, None if b is None else b.detach().contiguous(), relu, drop_p, seed, site)
        ctx.save_for_backward(xs, Wd, y if (relu or drop_p > 0) else None)
        ctx.drop_p, ctx.has_b, ctx.xshape = float(drop_p), b is not None, x.shape
        ctx.need_dx = x.requires_grad
        return y.view(*x.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, dy):
        xs, Wd, y = ctx.saved_tensors
        dyf = dy.reshape(-1, dy.shape[-1]).contiguous()
        dX, dW, db = engine.linear_bwd(xs, Wd, y, dyf, ctx.drop_p, need_dx=ctx.need_dx, need_db=ctx.has_b)
        return (dX.view(ctx.xshape) if dX is not None else None), dW, db, None, None, None, None


def linear(x, W, b=None, relu=False, drop_p=0.0, seed=None, site=0):
    """nn.Linear (+ ReLU + training-mode dropout) on the HIP engine; x [..., K]"""
    if not x.is_cuda:
        raise RuntimeError("linear runs on the GPU only (no CPU path)")
    if float(drop_p) > 0.0 and not relu:
        # the backward pass takes the saved output as its own mask (y > 0): without the ReLU a kept negative output would
        # get a zero gradient -- refuse instead of returning wrong gradients (mlp_plan never builds this combination)
        raise ValueError("linear: dropout needs relu=True (the kernels' dropout mask is the sign of the saved output)")
    return _LinearFn.apply(x, W, b, bool(relu), float(drop_p), seed, int(site))


def mlp_plan(modules):
    """[(nn.Linear, relu?, dropout p)] when `modules` (an nn.Sequential's children) is a chain of Linear [-> ReLU] [-> Dropout]
    groups -- what MLP_Block builds without norms / Dice -- else None (the caller keeps torch's modules)"""
    plan, i, mods = [], 0, list(modules)
    while i < len(mods):
        if type(mods[i]) is not nn.Linear:
            return None
        lin, relu, p = mods[i], False, 0.0
        i += 1
        if i < len(mods) and type(mods[i]) is nn.ReLU:
            relu, i = True, i + 1
        if i < len(mods) and type(mods[i]) is nn.Dropout:
            if not relu:
                return None  # the kernels' mask is the saved output: dropout without ReLU would lose the sign information
            p, i = float(mods[i].p), i + 1
        plan.append((lin, relu, p))
    return plan or None


class _MlpFn(torch.autograd.Function):
    """a whole mlp_plan as ONE autograd node: forward = one rc_linear_fwd per layer; backward = rc_linear_bwd per layer,
    top down, where the dX product of layer i + 1 applies the ReLU / dropout mask of layer i in its epilogue (the saved output of
    layer i is the input of layer i + 1), so no layer but the top one makes a separate masking pass over [M, width]."""

    @staticmethod
    def _tail(spec, params, M):
        """the last hidden layer + a width -> 1 output layer as the two tower-tail kernels (csrc/tower_tail.hip)?"""
        n = len(spec)
        if n < 2:
            return False
        (relu2, _, _), (relu3, p3, _) = spec[n - 2], spec[n - 1]
        W2, W3 = params[2 * (n - 2)], params[2 * (n - 1)]
        return bool(relu2 and not relu3 and p3 == 0.0 and W3.shape[0] == 1 and engine.tower_tail_supported(M, W2.shape[1], W2.shape[0]))

    @staticmethod
    def forward(ctx, x, spec, seed, *params):
        # spec: tuple of (relu, drop_p, has_bias) per layer; params: W_0, b_0 | None, W_1, ...
        xs = x.detach().reshape(-1, x.shape[-1]).contiguous()
        saved, h = [], xs
        n = len(spec)
        tail = _MlpFn._tail(spec, params, xs.shape[0])
        for site, (relu, p, has_b) in enumerate(spec):
            W = params[2 * site].detach().contiguous()
            b = params[2 * site + 1].detach().contiguous() if has_b else None
            if tail and site == n - 2:
                # one kernel for this layer and the output layer: H2 (saved: the output layer's input and this layer's mask), z
                W3 = params[2 * (n - 1)].detach().contiguous()
                b3 = params[2 * (n - 1) + 1].detach().contiguous() if spec[n - 1][2] else None
                if all(t.data_ptr() % 16 == 0 for t in (h, W, W3)):   # (float4 operand loads; an offset view keeps the GEMM route)
                    H2, z = engine.tower_tail_fwd(h, W, b, W3, b3, p, seed, site)
                    saved += [h, W, H2, W3]
                    h = z
                    break
                tail = False
            y = engine.linear_fwd(h, W, b, relu, p, seed, site)
            saved += [h, W]
            h = y
        ctx.save_for_backward(*saved, h)
        ctx.spec, ctx.xshape, ctx.need_dx, ctx.tail = spec, x.shape, x.requires_grad, tail
        return h.view(*x.shape[:-1], h.shape[-1])

    @staticmethod
    def backward(ctx, dy):
        spec = ctx.spec
        *saved, y_top = ctx.saved_tensors
        n = len(spec)
        dz = dy.reshape(-1, dy.shape[-1]).contiguous()
        grads = [None] * (2 * n)
        top = n - 1
        if ctx.tail:
            X2, W2, H2, W3 = saved[2 * (n - 2)], saved[2 * (n - 2) + 1], saved[2 * (n - 1)], saved[2 * (n - 1) + 1]
            below = spec[n - 3] if n > 2 else None
            x_act = below is not None and (below[0] or below[1] > 0)
            dX, dW2, db2, dW3, db3 = engine.tower_tail_bwd(X2, W2, W3, H2, dz, spec[n - 2][1], need_dx=(n > 2 or ctx.need_dx), x_act=x_act,
                                                           x_drop_p=below[1] if x_act else 0.0, need_db2=spec[n - 2][2], need_db3=spec[n - 1][2])
            grads[2 * (n - 2)], grads[2 * (n - 2) + 1], grads[2 * (n - 1)], grads[2 * (n - 1) + 1] = dW2, db2, dW3, db3
            dz, top = dX, n - 3
        # (the weight-gradient products on a second stream beside the dX chain -- rc_linear_bwd takes dX / dW separately --
        #  measured SLOWER inside the replayed graph at B = 1,024: 0.389 against 0.377 ms, profiles/r05h_gemm_probe.txt)
        for i in range(top, -1, -1):
            X, W = saved[2 * i], saved[2 * i + 1]
            relu, p, has_b = spec[i]
            # the top layer masks its own dY (Y = its saved output); every other layer receives a dY that the layer above
            # already masked in its dX product (x_act)
            y = y_top if (i == n - 1 and (relu or p > 0)) else None
            below = spec[i - 1] if i > 0 else None
            x_act = below is not None and (below[0] or below[1] > 0)
            need_dx = i > 0 or ctx.need_dx
            dX, dW, db = engine.linear_bwd(X, W, y, dz, p, need_dx=need_dx, need_db=has_b, x_act=x_act,
                                           x_drop_p=below[1] if x_act else 0.0)
            grads[2 * i], grads[2 * i + 1] = dW, db
            dz = dX
        return (dz.view(ctx.xshape) if dz is not None else None, None, None, *grads)


def mlp_forward(x, plan, training, seed):
    """run a mlp_plan (Linear [-> ReLU] [-> Dropout] groups) as one autograd node (dropout only in training mode; `seed` bumped
    by the caller)"""
    if not x.is_cuda:
        raise RuntimeError("mlp_forward runs on the GPU only (no CPU path)")
    spec = tuple((bool(relu), float(p) if training else 0.0, lin.bias is not None) for lin, relu, p in plan)
    params = []
    for lin, _, _ in plan:
        params += [lin.weight, lin.bias]
    return _MlpFn.apply(x, spec, seed, *params)


class HipOptimizer:
    """torch.optim.{SGD,Adam,Adagrad,Adadelta} semantics (dense, weight decay per param group) executed by
    rc_dense_update.  Built by the runner in place of `eval('torch.optim.X')`
    (helpers/BaseRunner.py:110-114); accepts the same param-group list
    (`model.customize_parameters()`, models/BaseModel.py:64-73)."""

    def __init__(self, param_groups, name="Adam", lr=1e-3, weight_decay=0.0, capturable=False):
        if name not in ("SGD", "Adam", "Adagrad", "Adadelta"):
            raise ValueError(f"HipOptimizer: optimizer {name!r} not built (SGD, Adam, Adagrad, Adadelta)")
        self.name, self.lr = name, lr
        # capturable: Adam's step count lives on the device, so step() can be recorded in a hipGraph
        self.capturable = capturable
        self._step_dev = None
        self.param_groups = []
        for g in param_groups:
            g = dict(g)
            g.setdefault("lr", lr)
            g.setdefault("weight_decay", weight_decay)
            g["params"] = list(g["params"])
            self.param_groups.append(g)
        self.state = {}
        self.step_count = 0
        self._rows = None           # the rows-mode step in flight (rows_begin .. step)
        self._rows_state = None     # its persistent buffers: row flags, the touched rows' gradient scratch

    # ---- rows mode: Adam over embedding tables of which a small batch touches a fraction of a percent ----------------------
    # torch.optim.Adam on a dense gradient updates every row every step (helpers/BaseRunner.py:110-114,206), so the pass over
    # tables and state cannot be skipped -- but the dense GRADIENT can.  At batch_size 1024 DeepFM's tables are 71 MB of which
    # 10 K rows have a gradient: the step zero-filled 71 MB, wrote row sums into it and read all of it back.  Here the gather
    # stamps the rows it looks up with the step's number, the backward pass writes the row sums into a scratch that is never
    # cleared, and the update reads a gradient only where the stamp matches (g = 0 elsewhere): rc_dense_update_rows_dev,
    # bit-identical to the dense step.  (Splitting the pass -- unstamped rows on a second stream beside forward / backward,
    # stamped rows at the end -- was measured and lost: profiles/r08_rows_adam_split_vs_single.txt.)
    def rows_ok(self):
        return self.name == "Adam" and self.capturable and os.environ.get("RC_ROWS_ADAM", "1") != "0"

    def _hyper_of(self, p):
        for g in self.param_groups:
            if any(q is p for q in g["params"]):
                return engine.make_hyper(self.name, lr=g["lr"], l2=g["weight_decay"], step=max(self.step_count, 1))
        return None

    def rows_begin(self, tables, tables1):
        """-> (row flags, step count on the device) for the gather to stamp, or None (rows mode not available: dense step)"""
        if not self.rows_ok():
            return None
        if self._rows is not None:
            raise RuntimeError("HipOptimizer rows mode: the previous training forward was not followed by backward + step()")
        params = list(tables) + list(tables1)
        hypers = [self._hyper_of(p) for p in params]
        if any(h is None for h in hypers):
            return None
        dev = params[0].device
        key = tuple(id(p) for p in params)
        st = self._rows_state
        capturing = torch.cuda.is_current_stream_capturing()    # (buffers are created by an eager step)
        if st is None or st["key"] != key:
            if capturing:
                return None
            n_rows, d = sum(t.shape[0] for t in tables), tables[0].shape[1]
            st = self._rows_state = {"key": key, "flags": torch.zeros(n_rows, dtype=torch.int32, device=dev),
                                     "G": torch.empty(n_rows * (d + 1), dtype=torch.float32, device=dev)}
        if self._step_dev is None:
            if capturing:
                return None
            self._step_dev = torch.full((1,), self.step_count, dtype=torch.int64, device=dev)
        for p in params:
            ps = self.state.setdefault(p, {})
            for k in ("m", "v"):
                if k not in ps:
                    if capturing:
                        return None
                    ps[k] = torch.zeros_like(p)
        offs, run = [], 0
        for t in tables:
            offs.append(run)
            run += t.shape[0]
        offs.append(run)
        self._rows = {"params": params, "hypers": hypers, "offs": offs, "F": len(tables), "G": None}
        # step() increments the count in front of its update launch; nothing between this gather (which reads count + 1) and that
        # launch reads it, so a tower's dropout-seed increment may take it along (engine.defer_increment)
        engine.defer_increment(self._step_dev)
        return st["flags"], self._step_dev

    def _rows_items(self, Gs):
        r, st = self._rows, self._rows_state
        F, offs, flags = r["F"], r["offs"], st["flags"]
        items = []
        for i, (p, h) in enumerate(zip(r["params"], r["hypers"])):
            f = i % F
            ps = self.state[p]
            items.append((p.data, Gs[i // F][offs[f]:offs[f + 1]], h, ps["m"], ps["v"], flags[offs[f]:offs[f + 1]], p.shape[1]))
        return items

    def rows_abort(self):
        """forget a rows-mode step that did not reach step() (the caller's step raised).  The tables took no update, but the gather
        stamped its rows with the number the NEXT step will carry too (the count was not incremented): the stamps are cleared, or
        rows of the abandoned batch would read stale gradient rows"""
        if self._rows is not None:
            self._rows = None
            folded = engine.take_deferred(self._step_dev)
            if self._rows_state is not None and not torch.cuda.is_current_stream_capturing():
                self._rows_state["flags"].zero_()
                if folded:      # the count went up with a tower's seed although no update followed: the step is forgotten
                    self._step_dev.sub_(1)

    def rows_scratch(self):
        return self._rows_state["G"]

    def rows_grads(self, Gv, Gl):
        self._rows["G"] = (Gv, Gl)

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            for p in g["params"]:
                p.grad = None

    @torch.no_grad()
    def step(self):
        """every parameter with a gradient in ONE rc_dense_update_multi call (per 36 tensors)"""
        items = []
        dev = None
        rows = self._rows
        if rows is not None and rows["G"] is None:
            raise RuntimeError("HipOptimizer rows mode: step() without the backward pass of the training forward")
        if rows is not None:      # (validated before anything is counted: a refused step leaves the optimizer as it was)
            mine = {id(q) for q in rows["params"]}
            if any(p.grad is not None and id(p) in mine for g in self.param_groups for p in g["params"]):
                raise RuntimeError("HipOptimizer rows mode: a table of the rows-mode gather also received a dense gradient")
        self.step_count += 1
        for g in self.param_groups:
            h = engine.make_hyper(self.name, lr=g["lr"], l2=g["weight_decay"], step=max(self.step_count, 1))
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state.setdefault(p, {})
                m = v = None
                # (state created once: `st.setdefault(k, torch.zeros_like(p))` would allocate and zero-fill a tensor of the
                # parameter's size on EVERY step just to throw it away -- 48 fill kernels per DeepFM step, 24 % of its
                # replayed GPU time in profiles/r02z_deepfm_kernel_stats.csv)
                if self.name in ("Adam", "Adagrad", "Adadelta"):   # exp_avg / state_sum / square_avg
                    if "m" not in st:
                        st["m"] = torch.zeros_like(p)
                    m = st["m"]
                if self.name in ("Adam", "Adadelta"):              # exp_avg_sq / acc_delta
                    if "v" not in st:
                        st["v"] = torch.zeros_like(p)
                    v = st["v"]
                grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                items.append((p.data, grad, h, m, v))
                dev = p.device
        if rows is not None:
            # the tables (gradient rows where stamped, g = 0 elsewhere) and every other parameter in one launch
            everything = [(w, gr, h, m, v, None, 0) for w, gr, h, m, v in items] + self._rows_items(rows["G"])
            if not engine.take_deferred(self._step_dev):      # (else a tower's seed increment took the count along)
                engine.step_increment(self._step_dev)
            engine.dense_update_rows(everything, self._step_dev, touched=2)
            self._rows = None
            return
        if self.capturable and items:
            if self._step_dev is None:  # (allocated outside any capture: the first step runs eagerly)
                self._step_dev = torch.full((1,), self.step_count - 1, dtype=torch.int64, device=dev)
            engine.dense_update_multi(items, self.name, step_dev=self._step_dev)
        else:
            engine.dense_update_multi(items, self.name)
