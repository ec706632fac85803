// chorus.hip -- Chorus (Wang et al., SIGIR 2020; reference models/sequential/Chorus.py:100-153), stage 2: an item's vector is its
// embedding plus its relational embeddings I[i] + Rel[r], each weighted by a temporal kernel of the time since the user's most recent
// history item in that relation, with the kernel's parameters read from three small per-category tables (betas, sigmas, mus:
// [n_cat, R] each):
//     decay_r = [t_r >= 0] clamp(kappa_r(t_r; betas, sigmas, mus [k, r]), -1, 1),   S = sum_r decay_r,
//     z = (1 + S) I[i] + sum_r decay_r Rel[r],   pred = <u', z> (+ user_bias[u] + item_bias[i]),   u' = U[u]  or  w o U[u] (GMF).
// Stage 1 (Chorus.py:155-177) is the launch sequence of rc_cfkg_fwd_bwd on (i_embeddings, r_embeddings) and has no kernel here.
//
// The FACTORED form is built: pred = (1 + S) <u', I[i]> + sum_r decay_r <u', Rel[r]>.  The R dot products with Rel are formed once
// per tuple, a candidate costs one row read and one DPP row reduction, and the integration itself is scalar work of one lane.
//
// Lane algebra of the front (chorus_front_kernel): one wave per tuple, kChorusTuples = 16 tuples per workgroup (four per wave, in
// turn).  LPR = d / 4 consecutive lanes own a candidate's I row (one float4 each), G = 64 / LPR candidates per wave trip.
//   1  <u', I[i_c]> for every candidate, kChorusStreamU rows in flight per lane-group, staged in the tuple's own coef row
//   2  ONE LANE PER CANDIDATE: category id and intervals first, then the 3 R parameter loads (one hop behind the category id, none
//      behind another), the kernels, the score (staged in the tuple's gpred row); GeneralModel.loss over the staged scores
//   3  the same lane: gpred, the kernels again with their derivatives (two or three expf per relation against a round trip of
//      3 R floats through memory), the kgrad row, coef = gpred (1 + S), and its share of gd[r] = sum_c gpred decay_r
//   4  zsum = sum_c coef_c I[i_c] (the rows again: they were just read by this wave) + sum_r gd[r] Rel[r]; ugrad = (w o) zsum;
//      the tuple's share of GRel[r] is gd[r] u' and of gw is U[u] o zsum: register accumulators across the wave's tuples, LDS in
//      wave order, one [R + 1, d] partial per workgroup, summed in workgroup order by chorus_partial_reduce_kernel.
// rc_chorus_scores_bwd is the same kernel without phase 2, with gpred given.
//
// The category update (three [n_cat, R] tables whose every row is hit by thousands of occurrences): the sorted occurrence list is
// cut every kChorusPiece = 1,024 positions; one workgroup sums one piece (a slice per half-wave or quarter-wave in ascending
// position, the slices in slice order), cutting at every change of category; a second kernel adds a category's pieces in piece order
// and applies the optimizer.  No segment is ever walked by one wave alone.
// No floating-point atomics anywhere; every sum has a fixed order, so results are bit-identical from run to run.
#include "bpr_math.hpp"
#include "common.hpp"
#include "opt_math.hpp"

namespace rc {

constexpr int kChorusMaxR = 8;        // relations, the self relation included
constexpr int kChorusTuples = 16;     // tuples per workgroup of the front
constexpr int kChorusStreamU = 4;     // candidate rows in flight per lane-group
constexpr int kChorusScoreU = 8;      // candidates per lane-group of one workgroup trip of the score kernel
constexpr int kChorusPiece = 1024;    // sorted positions one workgroup of the category update sums
constexpr int kChorusCatTables = 3;   // betas, sigmas, mus: the order of kgrad's column blocks and of every [3] array below
constexpr float kChorusLogSqrt2Pi = 0.91893853320467274178f;

struct ChorusKinds {
  int k[kChorusMaxR];   // 0 exponential, 1 normal around 0 ('complement'), 2 difference of normals ('substitute')
};

struct ChorusArgs {
  const float* U;
  const float* I;
  const float* Rel;
  const float* betas;
  const float* sigmas;
  const float* mus;
  const float* w;    // prediction.weight [d]; NULL selects BPR
  const float* ub;
  const float* ib;
  const int64_t* uid;
  const int64_t* iid;
  const int64_t* cid;
  const float* iv;   // relational_interval [B, C, R]
  ChorusKinds kinds;
  int B, C, R;
  float inv_b;
  const float* gin;  // rc_chorus_scores_bwd: the given gpred
  float* pred;
  float* loss_vec;
  float* gpred;
  float* coef;
  float* ugrad;
  float* ubgrad;
  float* kgrad;
  float* uprime;
  float* partial;    // [workgroups, R + 1, d]
};

__device__ __forceinline__ void chorus_fma4(float4& acc, float g, const float4& r) {
  acc.x = fmaf(g, r.x, acc.x);
  acc.y = fmaf(g, r.y, acc.y);
  acc.z = fmaf(g, r.z, acc.z);
  acc.w = fmaf(g, r.w, acc.w);
}

__device__ __forceinline__ float4 chorus_mul4(const float4& x, const float4& y) {
  return make_float4(x.x * y.x, x.y * y.y, x.z * y.z, x.w * y.w);
}

__device__ __forceinline__ void chorus_wave_mem_sync() {   // the wave's own global stores, read back by its other lanes
  __threadfence();
  __builtin_amdgcn_wave_barrier();
}

// decay = [tr >= 0] clamp(kappa, -1, 1) for one (candidate, relation); xb = betas[k, r] + 1, xs = sigmas[k, r] + 1, mu = mus[k, r] + 1.
// GRAD: d decay / d (betas, sigmas, mus)[k, r] with the mask and both clamp gates applied (torch's clamp passes the gradient on
// the closed interval).
template <bool GRAD>
__device__ __forceinline__ float chorus_decay(int kind, float tr, float xb, float xs, float mu, float& db, float& ds, float& dm) {
  const bool on = tr >= 0.f;
  const float dt = on ? tr : 0.f;
  const float beta = fminf(fmaxf(xb, 1e-10f), 10.f);
  float kappa, kb = 0.f, ks = 0.f, km = 0.f;
  if (kind == 0) {
    kappa = expf(logf(beta) - beta * dt);
    if (GRAD) kb = kappa * (1.f / beta - dt);
  } else {
    const float n0 = expf(-(dt * dt) / (2.f * (beta * beta)) - logf(beta) - kChorusLogSqrt2Pi);
    float dn0 = 0.f;
    if (GRAD) dn0 = n0 * ((dt * dt) / (beta * beta * beta) - 1.f / beta);
    if (kind == 1) {
      kappa = n0;
      kb = dn0;
    } else {
      const float sigma = fminf(fmaxf(xs, 1e-10f), 10.f);
      const float z = dt - mu;
      const float var = sigma * sigma;
      const float n1 = expf(-(z * z) / (2.f * var) - logf(sigma) - kChorusLogSqrt2Pi);
      kappa = n1 - n0;
      if (GRAD) {
        kb = -dn0;
        ks = n1 * ((z * z) / (var * sigma) - 1.f / sigma);
        km = n1 * (z / var);
      }
    }
  }
  if (GRAD) {
    const bool gate = on && kappa >= -1.f && kappa <= 1.f;
    db = (gate && xb >= 1e-10f && xb <= 10.f) ? kb : 0.f;
    ds = (gate && xs >= 1e-10f && xs <= 10.f) ? ks : 0.f;
    dm = gate ? km : 0.f;
  }
  return on ? fminf(fmaxf(kappa, -1.f), 1.f) : 0.f;
}

// One lane, one candidate: category id and intervals first, then the 3 R parameters; relations in ascending order.
//   S = sum_r decay_r,  dsum = sum_r decay_r ur[r]
// GRAD (g = gpred of the candidate, p = <u', I[i]>): the kgrad row, and gd[r] += g decay_r.
// NR = 1, 2, 4 or 8 >= R relation slots are unrolled (register arrays with static indices); a slot past R re-reads relation 0 and is
// left out of every sum.
template <bool GRAD, int NR>
__device__ __forceinline__ void chorus_integrate(const ChorusArgs& a, int64_t o, const float (&ur)[NR], float& S, float& dsum,
                                                 float g, float p, float (&gd)[NR]) {
  const int R = a.R;
  const int64_t k = a.cid[o];
  const float* ivr = a.iv + o * R;
  float tr[NR], xb[NR], xs[NR], xm[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) tr[r] = r < R ? ivr[r] : -1.f;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int64_t q = k * R + (r < R ? r : 0);
    xb[r] = a.betas[q] + 1.0f;
    xs[r] = a.sigmas[q] + 1.0f;
    xm[r] = a.mus[q] + 1.0f;
  }
  S = 0.f;
  dsum = 0.f;
  float* krow = GRAD ? a.kgrad + o * (3 * R) : nullptr;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    if (r < R) {
      float db, ds, dm;
      const float decay = chorus_decay<GRAD>(a.kinds.k[r], tr[r], xb[r], xs[r], xm[r], db, ds, dm);
      S += decay;
      dsum = fmaf(decay, ur[r], dsum);
      if (GRAD) {
        const float gr = g * (p + ur[r]);
        krow[r] = gr * db;
        krow[R + r] = gr * ds;
        krow[2 * R + r] = gr * dm;
        gd[r] = fmaf(g, decay, gd[r]);
      }
    }
  }
}

// ---- scores ---------------------------------------------------------------------------------------------------------------------
template <int D, int NR>
__global__ __launch_bounds__(kBlock) void chorus_scores_kernel(ChorusArgs a, int chunks) {
  constexpr int LPR = D / 4, G = 64 / LPR;
  constexpr int CPB = (kBlock / 64) * G * kChorusScoreU;   // candidates per workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane / LPR, l = lane % LPR;
  const int64_t t = blockIdx.x / chunks;
  const int c0 = (int)(blockIdx.x % chunks) * CPB + wave * (G * kChorusScoreU);
  if (c0 >= a.C) return;   // wave-uniform; no workgroup barrier in this kernel
  const bool gmf = a.w != nullptr;
  const int64_t u = a.uid[t];
  const int64_t* ids = a.iid + t * a.C;
  int64_t id[kChorusScoreU];
#pragma unroll
  for (int k = 0; k < kChorusScoreU; ++k) {
    const int c = c0 + k * G + grp;
    id[k] = ids[c < a.C ? c : c0];
  }
  float4 q4 = reinterpret_cast<const float4*>(a.U + u * D)[l];
  float4 r[kChorusScoreU];
#pragma unroll
  for (int k = 0; k < kChorusScoreU; ++k) r[k] = load_stream4(reinterpret_cast<const float4*>(a.I + id[k] * D) + l);
  if (gmf) q4 = chorus_mul4(q4, reinterpret_cast<const float4*>(a.w)[l]);
  float ur[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const float4 rel = reinterpret_cast<const float4*>(a.Rel)[(k < a.R ? k : 0) * LPR + l];
    ur[k] = row_allreduce_sum<LPR>(dot4(q4, rel));
  }
  const float ubu = gmf ? 0.f : a.ub[u];
  float gd[NR];
#pragma unroll
  for (int k = 0; k < kChorusScoreU; ++k) {
    const int c = c0 + k * G + grp;
    const float p = row_allreduce_sum<LPR>(dot4(q4, r[k]));
    if (l == 0 && c < a.C) {
      const int64_t o = t * a.C + c;
      float S, dsum;
      chorus_integrate<false, NR>(a, o, ur, S, dsum, 0.f, 0.f, gd);
      const float pc = fmaf(1.0f + S, p, dsum);
      a.pred[o] = gmf ? pc : (pc + ubu) + a.ib[id[k]];
    }
  }
}

// ---- the front: scores, loss and backward (LOSS), or the backward for a given gpred ---------------------------------------------------
template <int D, bool LOSS, int NR>
__global__ __launch_bounds__(kBlock) void chorus_front_kernel(ChorusArgs a) {
  constexpr int LPR = D / 4, G = 64 / LPR, NW = kBlock / 64, NP = NR + 1;
  __shared__ float4 part[NW * NP * LPR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane / LPR, l = lane % LPR;
  const int C = a.C, R = a.R;
  const bool gmf = a.w != nullptr;
  const float4 w4 = gmf ? reinterpret_cast<const float4*>(a.w)[l] : make_float4(1.f, 1.f, 1.f, 1.f);
  float4 rel[NR], racc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    rel[r] = reinterpret_cast<const float4*>(a.Rel)[(r < R ? r : 0) * LPR + l];
    racc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float4 wacc = make_float4(0.f, 0.f, 0.f, 0.f);

  for (int it = 0; it < kChorusTuples / NW; ++it) {
    const int64_t t = (int64_t)blockIdx.x * kChorusTuples + it * NW + wave;
    if (t >= a.B) break;   // wave-uniform, and t grows with `it`; only wave-level synchronisation inside this loop
    const int64_t u = a.uid[t];
    const float4 u4 = reinterpret_cast<const float4*>(a.U + u * D)[l];
    const float4 q4 = gmf ? chorus_mul4(u4, w4) : u4;
    const int64_t* ids = a.iid + t * C;
    float* stage = a.coef + t * C;   // <u', I[i_c]>, then coef
    float ur[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) ur[r] = row_allreduce_sum<LPR>(dot4(q4, rel[r]));   // the same in every lane-group

    // ---- 1: the candidate dot products
    for (int c0 = 0; c0 < C; c0 += kChorusStreamU * G) {
      float4 row[kChorusStreamU];
#pragma unroll
      for (int k = 0; k < kChorusStreamU; ++k) {
        const int c = c0 + k * G + grp;
        const int64_t id = ids[c < C ? c : 0];   // slots past C re-read candidate 0; masked at the store
        row[k] = reinterpret_cast<const float4*>(a.I + id * D)[l];   // (plain loads: the rows are read again in phase 4)
      }
#pragma unroll
      for (int k = 0; k < kChorusStreamU; ++k) {
        const int c = c0 + k * G + grp;
        const float p = row_allreduce_sum<LPR>(dot4(q4, row[k]));
        if (l == 0 && c < C) stage[c] = p;
      }
    }
    chorus_wave_mem_sync();

    // ---- 2: one lane per candidate: the score; the tuple's loss
    float* sp = a.gpred + t * C;   // the scores, then gpred
    float pos = 0.f, mx = 0.f, inv_se = 0.f, P = 0.f, A = 0.f, dLdP = 0.f;
    float gd[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) gd[r] = 0.f;
    if (LOSS) {
      const float ubu = gmf ? 0.f : a.ub[u];
      for (int c = lane; c < C; c += 64) {
        const int64_t o = t * C + c;
        float S, dsum;
        chorus_integrate<false, NR>(a, o, ur, S, dsum, 0.f, 0.f, gd);
        const float pc = fmaf(1.0f + S, stage[c], dsum);
        sp[c] = gmf ? pc : (pc + ubu) + a.ib[ids[c]];
      }
      chorus_wave_mem_sync();
      pos = sp[0];
      mx = -INFINITY;
      for (int c = 1 + lane; c < C; c += 64) mx = fmaxf(mx, sp[c]);
      mx = wave_allreduce_max(mx);
      float se = 0.f;
      for (int c = 1 + lane; c < C; c += 64) se += expf(sp[c] - mx);
      se = wave_allreduce_sum(se);
      inv_se = 1.0f / se;
      for (int c = 1 + lane; c < C; c += 64) {
        const float pc = sp[c];
        const float w = expf(pc - mx) * inv_se;
        const float s = sigmoidf_(pos - pc);
        P = fmaf(w, s, P);
        A = fmaf(w, s * (1.0f - s), A);
      }
      P = wave_allreduce_sum(P);
      A = wave_allreduce_sum(A);
      const BprRow br = bpr_row(P, a.inv_b);
      dLdP = br.dLdP;
      if (lane == 0) a.loss_vec[t] = br.loss;
      __builtin_amdgcn_wave_barrier();   // every lane holds pos before slot 0 is overwritten
    }

    // ---- 3: the same lane per candidate: gpred, the kgrad row, coef
    float gsum = 0.f;
    for (int c = lane; c < C; c += 64) {   // each lane overwrites only the slots it read itself
      const int64_t o = t * C + c;
      float g;
      if (LOSS) {
        const float pc = sp[c];
        if (c == 0) {
          g = dLdP * A;
        } else {
          const float w = expf(pc - mx) * inv_se;
          const float s = sigmoidf_(pos - pc);
          g = dLdP * bpr_dP_dneg(w, s, P);
        }
        if (a.pred != nullptr) a.pred[o] = pc;
        sp[c] = g;
      } else {
        g = a.gin[o];
      }
      float S, dsum;
      chorus_integrate<true, NR>(a, o, ur, S, dsum, g, stage[c], gd);
      stage[c] = g * (1.0f + S);
      gsum += g;
    }
    gsum = wave_allreduce_sum(gsum);
#pragma unroll
    for (int r = 0; r < NR; ++r) gd[r] = wave_allreduce_sum(gd[r]);   // 0 for r >= R
    if (lane == 0) a.ubgrad[t] = gsum;
    chorus_wave_mem_sync();

    // ---- 4: zsum = sum_c coef_c I[i_c] + sum_r gd[r] Rel[r]
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c0 = 0; c0 < C; c0 += kChorusStreamU * G) {
      float4 row[kChorusStreamU];
      float cf[kChorusStreamU];
#pragma unroll
      for (int k = 0; k < kChorusStreamU; ++k) {
        const int c = c0 + k * G + grp;
        const int64_t id = ids[c < C ? c : 0];
        row[k] = reinterpret_cast<const float4*>(a.I + id * D)[l];
        cf[k] = c < C ? stage[c] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < kChorusStreamU; ++k) chorus_fma4(acc, cf[k], row[k]);
    }
    acc.x = groups_allreduce_sum<LPR, 64>(acc.x);
    acc.y = groups_allreduce_sum<LPR, 64>(acc.y);
    acc.z = groups_allreduce_sum<LPR, 64>(acc.z);
    acc.w = groups_allreduce_sum<LPR, 64>(acc.w);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (r < R) {
        chorus_fma4(acc, gd[r], rel[r]);
        chorus_fma4(racc[r], gd[r], q4);
      }
    }
    if (gmf) {
      const float4 uz = chorus_mul4(u4, acc);
      wacc.x += uz.x; wacc.y += uz.y; wacc.z += uz.z; wacc.w += uz.w;
      acc = chorus_mul4(w4, acc);
    }
    if (grp == 0) {
      reinterpret_cast<float4*>(a.ugrad + t * D)[l] = acc;
      if (gmf) reinterpret_cast<float4*>(a.uprime + t * D)[l] = q4;
    }
  }

  // the waves of the workgroup in wave order (every lane-group of a wave holds the same accumulators)
  if (lane < LPR) {
#pragma unroll
    for (int r = 0; r < NR; ++r) part[(wave * NP + r) * LPR + l] = racc[r];
    part[(wave * NP + NR) * LPR + l] = wacc;
  }
  __syncthreads();
  const int slots = R + 1;   // GRel rows, then gw
  for (int j = threadIdx.x; j < slots * LPR; j += kBlock) {
    const int k = j / LPR, ll = j % LPR;
    const int src = (k < R ? k : NR) * LPR + ll;
    float4 s = part[src];
#pragma unroll
    for (int wv = 1; wv < NW; ++wv) {
      const float4 y = part[wv * NP * LPR + src];
      s.x += y.x; s.y += y.y; s.z += y.z; s.w += y.w;
    }
    reinterpret_cast<float4*>(a.partial + (int64_t)blockIdx.x * slots * D)[j] = s;
  }
}

// One workgroup per slot k (GRel row k; slot R: gw): lane-group g sums the partials of workgroups g, g + GPB, ... in that order (four
// loads in flight), then lane-group 0's lanes add the GPB sums in group order.
template <int D>
__global__ __launch_bounds__(kBlock) void chorus_partial_reduce_kernel(const float* partial, int n_blocks, int R, float* GRel, float* gw) {
  constexpr int LPR = D / 4, GPB = kBlock / LPR;
  __shared__ float4 part[kBlock];
  const int l = threadIdx.x % LPR, g = threadIdx.x / LPR;
  const int k = blockIdx.x;
  const float4* p = reinterpret_cast<const float4*>(partial) + (int64_t)k * LPR + l;
  const int64_t stride = (int64_t)(R + 1) * LPR;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i0 = g; i0 < n_blocks; i0 += 4 * GPB) {
    float4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + q * GPB;
      v[q] = p[(i < n_blocks ? i : i0) * stride];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (i0 + q * GPB < n_blocks) {
        acc.x += v[q].x; acc.y += v[q].y; acc.z += v[q].z; acc.w += v[q].w;
      }
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  if (g == 0) {
    float4 s = part[l];
    for (int q = 1; q < GPB; ++q) {
      const float4 y = part[q * LPR + l];
      s.x += y.x; s.y += y.y; s.z += y.z; s.w += y.w;
    }
    float* out = k < R ? GRel + (int64_t)k * D : gw;
    reinterpret_cast<float4*>(out)[l] = s;
  }
}

// ---- the category update ----------------------------------------------------------------------------------------------------------
struct ChorusCat {
  float* W[kChorusCatTables];
  float* M[kChorusCatTables];
  float* V[kChorusCatTables];
  float* dense[kChorusCatTables];
  const uint32_t* keys;
  const uint32_t* perm;
  int64_t n_occ;
  int64_t n_cat;
  const float* kgrad;
  int R;
  const uint32_t* heads;
  const uint32_t* n_heads;
  float* first;      // [pieces, 3 R]: the sum of the run that holds a piece's first position, over that piece
  float* headpart;   // [n_cat, 3 R]: the sum of the run of category k from its head to the end of the head's piece, where the head
                     // is not a piece's first position
  OptScalars o;
};

// Workgroup q sums the positions [q P, (q + 1) P) of the sorted list, cut at every change of key.  Thread (s, e) walks slice s (P / NS
// consecutive positions) for element e of the 3 R in ascending position; thread (0, e) then joins the slices in slice order.  A run
// that holds the piece's first position goes to first[q]; every other run starts at a head inside the piece and goes to
// headpart[key] (one run per key, so one writer per element).
template <int LPS>
__global__ __launch_bounds__(kBlock) void chorus_cat_piece_kernel(ChorusCat a) {
  constexpr int NS = kBlock / LPS, SLEN = kChorusPiece / NS, Q = 8;
  __shared__ float lead[NS][LPS], tail[NS][LPS];
  __shared__ int has_tail[NS];
  const int e = threadIdx.x % LPS, s = threadIdx.x / LPS;
  const int R3 = 3 * a.R;
  const bool live = e < R3;
  const int ee = live ? e : 0;
  const int64_t n = a.n_occ;
  const int64_t p0 = (int64_t)blockIdx.x * kChorusPiece;
  const int64_t j0 = p0 + (int64_t)s * SLEN;
  const int64_t j1 = j0 + SLEN < n ? j0 + SLEN : n;
  float acc = 0.f, leadv = 0.f;
  bool leading = true;
  if (j0 < n) {
    uint32_t key = a.keys[j0];
    for (int64_t jb = j0; jb < j1; jb += Q) {
      uint32_t kk[Q];
      float v[Q];
#pragma unroll
      for (int i = 0; i < Q; ++i) {   // Q positions requested together; the adds below stay in order
        const int64_t j = jb + i < j1 ? jb + i : j0;
        kk[i] = a.keys[j];
        v[i] = a.kgrad[(int64_t)a.perm[j] * R3 + ee];
      }
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        if (jb + i < j1) {
          if (kk[i] != key) {   // the same for every thread of the slice
            if (leading) {
              leadv = acc;
              leading = false;
            } else if (live && key < a.n_cat) {   // a run that starts and ends inside this slice
              a.headpart[(int64_t)key * R3 + e] = acc;
            }
            acc = 0.f;
            key = kk[i];
          }
          acc += v[i];
        }
      }
    }
    if (leading) leadv = acc;
  }
  lead[s][e] = leadv;
  tail[s][e] = leading ? 0.f : acc;
  if (e == 0) has_tail[s] = (j0 < n && !leading) ? 1 : 0;
  __syncthreads();
  if (s == 0 && live) {
    float cur = lead[0][e];
    uint32_t curkey = a.keys[p0];
    bool piece_first = true;
    auto flush = [&]() {
      if (piece_first) a.first[(int64_t)blockIdx.x * R3 + e] = cur;
      else if (curkey < a.n_cat) a.headpart[(int64_t)curkey * R3 + e] = cur;
    };
    for (int ss = 0; ss < NS; ++ss) {
      const int64_t sj0 = p0 + (int64_t)ss * SLEN;
      if (sj0 >= n) break;
      if (ss > 0) {
        const uint32_t k0 = a.keys[sj0];
        if (k0 == curkey) {
          cur += lead[ss][e];
        } else {   // the run ended exactly at the slice boundary
          flush();
          cur = lead[ss][e];
          curkey = k0;
          piece_first = false;
        }
      }
      if (has_tail[ss]) {
        flush();
        const int64_t sj1 = sj0 + SLEN < n ? sj0 + SLEN : n;
        cur = tail[ss][e];
        curkey = a.keys[sj1 - 1];
        piece_first = false;
      }
    }
    flush();
  }
}

// one float of table `tix` (runtime index, per lane): select, not a dynamically indexed kernel argument
template <class T>
__device__ __forceinline__ T* chorus_pick(T* const (&p)[kChorusCatTables], int tix) {
  T* r = p[0];
#pragma unroll
  for (int k = 1; k < kChorusCatTables; ++k) r = (tix == k) ? p[k] : r;
  return r;
}

// 32 lanes per listed head, lane e takes element e of the 3 R: the end of the segment by bisection of the sorted keys, the pieces of
// the row in piece order (eight loads in flight), then the dense gradient or the optimizer on (betas | sigmas | mus)[key, e % R].
template <int MODE>
__global__ __launch_bounds__(kBlock) void chorus_cat_apply_kernel(ChorusCat a) {
  constexpr int LPH = 32, HPB = kBlock / LPH, Q = 8;
  const int e = threadIdx.x % LPH;
  const int64_t h = (int64_t)blockIdx.x * HPB + threadIdx.x / LPH;
  const int R3 = 3 * a.R;
  if (h >= (int64_t)*a.n_heads || e >= R3) return;   // no cross-lane operation in this kernel
  const int64_t n = a.n_occ;
  const int64_t j0 = a.heads[h];
  const uint32_t key = a.keys[j0];
  if (key >= a.n_cat) return;
  int64_t lo = j0 + 1, hi = n;   // the first position past j0 whose key is larger
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a.keys[mid] > key) hi = mid;
    else lo = mid + 1;
  }
  const int64_t q0 = j0 / kChorusPiece, q1 = (lo - 1) / kChorusPiece;
  float g = (j0 % kChorusPiece == 0) ? a.first[q0 * R3 + e] : a.headpart[(int64_t)key * R3 + e];
  for (int64_t qb = q0 + 1; qb <= q1; qb += Q) {
    float v[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) v[i] = a.first[(qb + i <= q1 ? qb + i : qb) * R3 + e];
#pragma unroll
    for (int i = 0; i < Q; ++i)
      if (qb + i <= q1) g += v[i];
  }
  const int tix = e / a.R;
  const size_t idx = (size_t)key * a.R + (e % a.R);
  if (MODE == MODE_DENSE_GRAD) {
    chorus_pick(a.dense, tix)[idx] = g;
    return;
  }
  float* W = chorus_pick(a.W, tix);
  if (W == nullptr) return;   // a table without a gradient is left alone
  float w = W[idx], m = 0.f, v = 0.f;
  if (mode_has_m(MODE)) m = chorus_pick(a.M, tix)[idx];
  if (mode_has_v(MODE)) v = chorus_pick(a.V, tix)[idx];
  opt_elem<MODE>(a.o, g, w, m, v);
  W[idx] = w;
  if (mode_has_m(MODE)) chorus_pick(a.M, tix)[idx] = m;
  if (mode_has_v(MODE)) chorus_pick(a.V, tix)[idx] = v;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static int chorus_slots(int R) { return R <= 1 ? 1 : (R <= 2 ? 2 : (R <= 4 ? 4 : 8)); }   // unrolled relation slots of the kernels
static bool chorus_width_ok(int d) { return d == 16 || d == 32 || d == 64 || d == 128; }

static int chorus_shape_check(const char* who, int d, int C, int R, int min_c) {
  RC_REQUIRE(chorus_width_ok(d), "%s: emb_size d=%d has no kernel (16, 32, 64, 128)", who, d);
  RC_REQUIRE(C >= min_c, "%s: need C >= %d candidates, got %d", who, min_c, C);
  RC_REQUIRE(R >= 1 && R <= kChorusMaxR, "%s: relation_num R=%d outside 1..%d (item relations + 1)", who, R, kChorusMaxR);
  return RC_OK;
}

static int chorus_fill_args(const char* who, ChorusArgs* a, const float* U, const float* I, const float* Rel, const float* betas,
                            const float* sigmas, const float* mus, const float* w, const float* user_bias, const float* item_bias,
                            const int64_t* uid, const int64_t* iid, const int64_t* cid, const float* intervals, const int* kinds, int B,
                            int C, int d, int R, int min_c) {
  RC_REQUIRE(U && I && Rel && betas && sigmas && mus && uid && iid && cid && intervals && kinds, "%s: null pointer", who);
  RC_REQUIRE(w != nullptr || (user_bias && item_bias), "%s: the BPR head (w = NULL) needs user_bias and item_bias", who);
  RC_TRY(chorus_shape_check(who, d, C, R, min_c));
  RC_REQUIRE(B > 0, "%s: need B >= 1, got B=%d", who, B);
  RC_REQUIRE((int64_t)B * C * 3 * R < ((int64_t)1 << 40), "%s: B * C too large (B=%d C=%d)", who, B, C);
  RC_REQUIRE(aligned16(U, I, Rel, w), "%s: U, I, Rel and w must be 16-byte aligned", who);
  memset(a, 0, sizeof(*a));
  for (int r = 0; r < R; ++r) {
    RC_REQUIRE(kinds[r] >= 0 && kinds[r] <= 2, "%s: kinds[%d]=%d is none of 0 (exponential), 1 (complement), 2 (substitute)", who, r,
               kinds[r]);
    a->kinds.k[r] = kinds[r];
  }
  a->U = U; a->I = I; a->Rel = Rel; a->betas = betas; a->sigmas = sigmas; a->mus = mus; a->w = w; a->ub = user_bias; a->ib = item_bias;
  a->uid = uid; a->iid = iid; a->cid = cid; a->iv = intervals; a->B = B; a->C = C; a->R = R;
  return RC_OK;
}

static size_t chorus_front_ws_bytes(int64_t B, int d, int R) {
  if (!chorus_width_ok(d) || R < 1 || R > kChorusMaxR) return 0;
  if (B < 1) B = 1;
  const int64_t blocks = (B + kChorusTuples - 1) / kChorusTuples;
  return align_up((size_t)blocks * (R + 1) * d * sizeof(float), 256);
}

template <bool LOSS>
static int chorus_front_launch(const char* who, ChorusArgs& a, int d, float* GRel, float* gw, void* ws, size_t ws_bytes,
                               rc_stream_t stream) {
  RC_REQUIRE(a.coef && a.ugrad && a.ubgrad && a.kgrad && GRel && ws, "%s: null pointer", who);
  RC_REQUIRE(a.w == nullptr || (gw && a.uprime), "%s: the GMF head (w given) needs gw and uprime", who);
  RC_REQUIRE(aligned16(a.ugrad, a.uprime, GRel, gw, ws), "%s: ugrad, uprime, GRel, gw and the workspace must be 16-byte aligned", who);
  const size_t need = chorus_front_ws_bytes(a.B, d, a.R);
  if (ws_bytes < need) return fail(RC_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, need);
  a.partial = reinterpret_cast<float*>(ws);
  const int blocks = (a.B + kChorusTuples - 1) / kChorusTuples;
  hipStream_t s = as_stream(stream);
  return dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", d, [&](auto D) -> int {
    RC_TRY((dispatch_or_fail<1, 2, 4, 8>(who, "relation slots", chorus_slots(a.R), [&](auto NR) -> int {
      hipLaunchKernelGGL((chorus_front_kernel<D(), LOSS, NR()>), dim3(blocks), dim3(kBlock), 0, s, a);
      RC_LAUNCH_CHECK();
      return RC_OK;
    })));
    hipLaunchKernelGGL((chorus_partial_reduce_kernel<D()>), dim3(a.R + (a.w != nullptr ? 1 : 0)), dim3(kBlock), 0, s, a.partial, blocks,
                       a.R, GRel, gw);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

static int chorus_scores_impl(const float* U, const float* I, const float* Rel, const float* betas, const float* sigmas,
                              const float* mus, const float* w, const float* user_bias, const float* item_bias, const int64_t* uid,
                              const int64_t* iid, const int64_t* cid, const float* intervals, const int* kinds, int B, int C, int d,
                              int R, float* pred, rc_stream_t stream) {
  static const char* who = "rc_chorus_scores";
  if (B == 0) return RC_OK;
  ChorusArgs a;
  RC_TRY(chorus_fill_args(who, &a, U, I, Rel, betas, sigmas, mus, w, user_bias, item_bias, uid, iid, cid, intervals, kinds, B, C, d, R, 1));
  RC_REQUIRE(pred != nullptr, "%s: null pointer", who);
  a.pred = pred;
  hipStream_t s = as_stream(stream);
  return dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", d, [&](auto D) -> int {
    constexpr int CPB = (kBlock / 64) * (256 / D()) * kChorusScoreU;
    const int64_t chunks = ((int64_t)C + CPB - 1) / CPB;
    const int64_t blocks = chunks * B;
    if (blocks > kMaxGridX) return fail(RC_ERR_UNSUPPORTED, "%s: grid too large (B=%d C=%d)", who, B, C);
    return dispatch_or_fail<1, 2, 4, 8>(who, "relation slots", chorus_slots(R), [&](auto NR) -> int {
      hipLaunchKernelGGL((chorus_scores_kernel<D(), NR()>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a, (int)chunks);
      RC_LAUNCH_CHECK();
      return RC_OK;
    });
  });
}

static int chorus_fwd_bwd_impl(const float* U, const float* I, const float* Rel, const float* betas, const float* sigmas,
                               const float* mus, const float* w, const float* user_bias, const float* item_bias, const int64_t* uid,
                               const int64_t* iid, const int64_t* cid, const float* intervals, const int* kinds, int B, int C, int d,
                               int R, float inv_b, float* pred, float* loss_vec, float* gpred, float* coef, float* ugrad, float* ubgrad,
                               float* kgrad, float* GRel, float* gw, float* uprime, void* ws, size_t ws_bytes, rc_stream_t stream) {
  static const char* who = "rc_chorus_fwd_bwd";
  if (B == 0) return RC_OK;
  ChorusArgs a;
  RC_TRY(chorus_fill_args(who, &a, U, I, Rel, betas, sigmas, mus, w, user_bias, item_bias, uid, iid, cid, intervals, kinds, B, C, d, R, 2));
  RC_REQUIRE(loss_vec && gpred, "%s: null pointer", who);
  a.inv_b = inv_b; a.pred = pred; a.loss_vec = loss_vec; a.gpred = gpred; a.coef = coef; a.ugrad = ugrad; a.ubgrad = ubgrad;
  a.kgrad = kgrad; a.uprime = uprime;
  return chorus_front_launch<true>(who, a, d, GRel, gw, ws, ws_bytes, stream);
}

static int chorus_scores_bwd_impl(const float* U, const float* I, const float* Rel, const float* betas, const float* sigmas,
                                  const float* mus, const float* w, const int64_t* uid, const int64_t* iid, const int64_t* cid,
                                  const float* intervals, const int* kinds, const float* gpred, int B, int C, int d, int R, float* coef,
                                  float* ugrad, float* ubgrad, float* kgrad, float* GRel, float* gw, float* uprime, void* ws,
                                  size_t ws_bytes, rc_stream_t stream) {
  static const char* who = "rc_chorus_scores_bwd";
  if (B == 0) return RC_OK;
  ChorusArgs a;
  // (the biases enter the score additively: their values are not read by the backward; U stands in for the two pointers)
  RC_TRY(chorus_fill_args(who, &a, U, I, Rel, betas, sigmas, mus, w, U, U, uid, iid, cid, intervals, kinds, B, C, d, R, 1));
  RC_REQUIRE(gpred != nullptr, "%s: null pointer", who);
  a.ub = nullptr; a.ib = nullptr;
  a.gin = gpred; a.coef = coef; a.ugrad = ugrad; a.ubgrad = ubgrad; a.kgrad = kgrad; a.uprime = uprime;
  return chorus_front_launch<false>(who, a, d, GRel, gw, ws, ws_bytes, stream);
}

struct ChorusCatWs {
  float* first;
  float* headpart;
  int64_t pieces;
  size_t total;
};

static ChorusCatWs carve_chorus_cat_ws(void* base, int64_t n_occ, int64_t n_cat, int R) {
  Carver cv(base);
  ChorusCatWs w;
  w.pieces = (n_occ + kChorusPiece - 1) / kChorusPiece;
  w.first = cv.take<float>((size_t)w.pieces * 3 * R);
  w.headpart = cv.take<float>((size_t)n_cat * 3 * R);
  w.total = cv.off;
  return w;
}

static int chorus_category_update_impl(float* const* W, float* const* M, float* const* V, int64_t n_cat, int R, const uint32_t* keys,
                                       const uint32_t* perm, int64_t n_occ, const float* kgrad, const rc_opt_hyper* h,
                                       float* const* dense_grad, const uint32_t* heads, const uint32_t* n_heads, void* ws,
                                       size_t ws_bytes, rc_stream_t stream) {
  static const char* who = "rc_chorus_category_update";
  if (n_occ == 0) return RC_OK;
  const bool dense = dense_grad != nullptr;
  if (dense) {
    int given = 0;
    for (int k = 0; k < kChorusCatTables; ++k) given += dense_grad[k] != nullptr;
    RC_REQUIRE(given == kChorusCatTables, "%s: all three dense gradients or none (got %d)", who, given);
  }
  RC_REQUIRE(keys && perm && kgrad && ws, "%s: null pointer", who);
  RC_REQUIRE(heads && n_heads, "%s: the head list of rc_segment_heads is required", who);
  RC_REQUIRE(dense || W != nullptr, "%s: no output (the three tables, or the dense gradients)", who);
  RC_REQUIRE(R >= 1 && R <= kChorusMaxR, "%s: relation_num R=%d outside 1..%d", who, R, kChorusMaxR);
  RC_REQUIRE(n_cat >= 1 && n_cat < ((int64_t)1 << 31), "%s: bad shape n_cat=%lld", who, (long long)n_cat);
  RC_REQUIRE(n_occ > 0 && n_occ < ((int64_t)1 << 31), "%s: bad shape n_occ=%lld", who, (long long)n_occ);
  ChorusCat a;
  memset(&a, 0, sizeof(a));
  int mode = MODE_DENSE_GRAD;
  if (!dense) {
    bool have_m = M != nullptr, have_v = V != nullptr;
    RC_REQUIRE(W[0] != nullptr, "%s: no output (betas is null)", who);
    for (int k = 0; k < kChorusCatTables; ++k) {   // a null sigmas / mus is left alone: no relation of kind 2, no gradient
      a.W[k] = W[k];
      have_m = have_m && (W[k] == nullptr || M[k] != nullptr);
      have_v = have_v && (W[k] == nullptr || V[k] != nullptr);
    }
    RC_TRY(fill_opt_scalars(who, h, &a.o));
    mode = mode_of(h);
    RC_TRY(opt_state_check(who, mode, have_m, have_v));
    for (int k = 0; k < kChorusCatTables; ++k) {
      a.M[k] = (mode_has_m(mode) && W[k] != nullptr) ? M[k] : nullptr;
      a.V[k] = (mode_has_v(mode) && W[k] != nullptr) ? V[k] : nullptr;
    }
  } else {
    for (int k = 0; k < kChorusCatTables; ++k) a.dense[k] = dense_grad[k];
  }
  const ChorusCatWs w = carve_chorus_cat_ws(ws, n_occ, n_cat, R);
  if (ws_bytes < w.total) return fail(RC_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, w.total);
  a.keys = keys; a.perm = perm; a.n_occ = n_occ; a.n_cat = n_cat; a.kgrad = kgrad; a.R = R; a.heads = heads; a.n_heads = n_heads;
  a.first = w.first; a.headpart = w.headpart;
  hipStream_t s = as_stream(stream);
  if (3 * R <= 16) {
    hipLaunchKernelGGL((chorus_cat_piece_kernel<16>), dim3((unsigned)w.pieces), dim3(kBlock), 0, s, a);
  } else {
    hipLaunchKernelGGL((chorus_cat_piece_kernel<32>), dim3((unsigned)w.pieces), dim3(kBlock), 0, s, a);
  }
  RC_LAUNCH_CHECK();
  const int64_t max_heads = n_occ < n_cat ? n_occ : n_cat;
  const int64_t blocks = (max_heads + (kBlock / 32) - 1) / (kBlock / 32);
  return dispatch_or_fail<MODE_DENSE_GRAD, MODE_SGD, MODE_ADAM, MODE_ADAGRAD>(who, "update mode", mode, [&](auto MD) -> int {
    hipLaunchKernelGGL((chorus_cat_apply_kernel<MD()>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

}  // namespace rc

using namespace rc;

extern "C" enum rc_status rc_chorus_check_shape(int d, int C, int R) {
  return (enum rc_status)chorus_shape_check("rc_chorus_check_shape", d, C, R, 1);
}

extern "C" size_t rc_chorus_front_tuples_per_block(void) { return (size_t)kChorusTuples; }

extern "C" size_t rc_chorus_category_piece(void) { return (size_t)kChorusPiece; }

extern "C" enum rc_status rc_chorus_scores(const float* U, const float* I, const float* Rel, const float* betas, const float* sigmas,
                                           const float* mus, const float* w, const float* user_bias, const float* item_bias,
                                           const int64_t* uid, const int64_t* iid, const int64_t* cid, const float* intervals,
                                           const int* kinds, int B, int C, int d, int R, float* pred, rc_stream_t stream) {
  return (enum rc_status)chorus_scores_impl(U, I, Rel, betas, sigmas, mus, w, user_bias, item_bias, uid, iid, cid, intervals, kinds, B,
                                            C, d, R, pred, stream);
}

extern "C" size_t rc_chorus_front_workspace_bytes(int64_t B, int d, int R) { return chorus_front_ws_bytes(B, d, R); }

extern "C" enum rc_status rc_chorus_fwd_bwd(const float* U, const float* I, const float* Rel, const float* betas, const float* sigmas,
                                            const float* mus, const float* w, const float* user_bias, const float* item_bias,
                                            const int64_t* uid, const int64_t* iid, const int64_t* cid, const float* intervals,
                                            const int* kinds, int B, int C, int d, int R, float inv_b, float* pred, float* loss_vec,
                                            float* gpred, float* coef, float* ugrad, float* ubgrad, float* kgrad, float* GRel, float* gw,
                                            float* uprime, void* ws, size_t ws_bytes, rc_stream_t stream) {
  return (enum rc_status)chorus_fwd_bwd_impl(U, I, Rel, betas, sigmas, mus, w, user_bias, item_bias, uid, iid, cid, intervals, kinds, B,
                                             C, d, R, inv_b, pred, loss_vec, gpred, coef, ugrad, ubgrad, kgrad, GRel, gw, uprime, ws,
                                             ws_bytes, stream);
}

extern "C" enum rc_status rc_chorus_scores_bwd(const float* U, const float* I, const float* Rel, const float* betas, const float* sigmas,
                                               const float* mus, const float* w, const int64_t* uid, const int64_t* iid,
                                               const int64_t* cid, const float* intervals, const int* kinds, const float* gpred, int B,
                                               int C, int d, int R, float* coef, float* ugrad, float* ubgrad, float* kgrad, float* GRel,
                                               float* gw, float* uprime, void* ws, size_t ws_bytes, rc_stream_t stream) {
  return (enum rc_status)chorus_scores_bwd_impl(U, I, Rel, betas, sigmas, mus, w, uid, iid, cid, intervals, kinds, gpred, B, C, d, R,
                                                coef, ugrad, ubgrad, kgrad, GRel, gw, uprime, ws, ws_bytes, stream);
}

extern "C" size_t rc_chorus_category_update_workspace_bytes(int64_t n_occ, int64_t n_cat, int R) {
  if (n_occ < 1) n_occ = 1;
  if (n_cat < 1) n_cat = 1;
  if (R < 1 || R > kChorusMaxR) return 0;
  return carve_chorus_cat_ws(nullptr, n_occ, n_cat, R).total;
}

extern "C" enum rc_status rc_chorus_category_update(float* const* W, float* const* M, float* const* V, int64_t n_cat, int R,
                                                    const uint32_t* keys, const uint32_t* perm, int64_t n_occ, const float* kgrad,
                                                    const rc_opt_hyper* h, float* const* dense_grad, const uint32_t* heads,
                                                    const uint32_t* n_heads, void* ws, size_t ws_bytes, rc_stream_t stream) {
  return (enum rc_status)chorus_category_update_impl(W, M, V, n_cat, R, keys, perm, n_occ, kgrad, h, dense_grad, heads, n_heads, ws,
                                                     ws_bytes, stream);
}
