// slrc.hip -- SLRC+ (Wang et al., TheWebConf 2019; reference models/sequential/SLRCPlus.py:62-89): BPRMF with user and item biases plus
// a per-candidate Hawkes excitation read from five narrow per-item tables (alphas, pis, betas, sigmas, mus: [n_items, R] each),
//     pred[b, c] = <U[u_b], I[i]> + user_bias[u_b] + item_bias[i] + sum_r alpha_r (pi_r e_r + (1 - pi_r) n_r) [t_r >= 0],
// with GeneralModel.loss (models/BaseModel.py:182-185) on top.  Scores, the fused forward / loss / backward and the item-side row
// update of all seven item tables in one pass over the sorted candidate ids; the one-float-per-row user_bias update.
//
// Lane algebra: LPR = d / 4 consecutive lanes own a candidate's I row (one float4 each, read once), G = 64 / LPR candidates per wave
// trip, one tuple per wave.  The dot products go through a DPP row reduction into an LDS strip; then ONE LANE PER CANDIDATE adds the
// biases and the excitation (5 R scalar loads: rows of an [n_items, 3] table are not 16-byte aligned), and the same lane writes the
// candidate's 5 R partial derivatives, times gpred, into its hgrad row once the tuple's loss has produced gpred (the excitation is
// evaluated a second time for that: two expf per relation against a round trip of the row through memory).  The item update then
// needs neither the intervals nor any transcendental.
//
// Paths of rc_slrc_fwd_bwd (rc_slrc_fwd_bwd_layout reports the choice):
//   register   each lane-group holds CPL = ceil(C / G) <= 25 candidate rows (4 CPL VGPRs per lane) between the score and the backward
//              sum: C <= 400 / 200 / 100 / 50 at d = 16 / 32 / 64 / 128.
//   streaming  any C >= 2: the scores staged in the tuple's own gpred row, the candidate rows re-read for the backward sum (they were
//              just read by the same wave: L2 hits).
// No floating-point atomics; every sum has a fixed order.
#include "bpr_math.hpp"
#include "common.hpp"
#include "opt_math.hpp"

namespace rc {

constexpr int kSlrcMaxCpl = 25;    // candidate rows per lane-group on the register path
constexpr int kSlrcMaxR = 8;       // relations, the self relation included
constexpr int kSlrcLongSeg = 32;   // occurrences one lane-group sums on its own in the item update
constexpr int kSlrcTables = 7;     // I, item_bias, alphas, pis, betas, sigmas, mus: the order of every [7] array below
constexpr float kLogSqrt2Pi = 0.91893853320467274178f;

struct SlrcTables {
  const float* U;
  const float* I;
  const float* ub;
  const float* ib;
  const float* ga;
  const float* H[5];   // alphas, pis, betas, sigmas, mus
};

struct SlrcArgs {
  SlrcTables t;
  const int64_t* uid;
  const int64_t* iid;
  const float* iv;     // relational_interval [B, C, R]
  int B, C, R;
  float inv_b;
  float* pred;
  float* loss_vec;
  float* gpred;
  float* ugrad;
  float* ubgrad;
  float* hgrad;
  float* gagrad;
};

__device__ __forceinline__ void slrc_fma4(float4& acc, float g, const float4& r) {
  acc.x = fmaf(g, r.x, acc.x);
  acc.y = fmaf(g, r.y, acc.y);
  acc.z = fmaf(g, r.z, acc.z);
  acc.w = fmaf(g, r.w, acc.w);
}

__device__ __forceinline__ void slrc_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The excitation of candidate `id` with intervals iv[0, R); dga = sum_r decay_r mask_r = d pred / d global_alpha.  GRAD: the 5 R
// partial derivatives d pred / d (alphas | pis | betas | sigmas | mus)[id, r], times g, go to hrow, clamp and mask applied (torch's clamp
// passes the gradient on [min, max], both ends included).  One lane, scalar loads, relations in ascending order.
template <bool GRAD>
__device__ __forceinline__ float slrc_excite(const SlrcTables& t, int64_t id, const float* iv, int R, float ga, float* hrow, float& dga,
                                             float g = 1.f) {
  float exc = 0.f;
  dga = 0.f;
  for (int r = 0; r < R; ++r) {
    const size_t k = (size_t)id * R + r;
    const float tr = iv[r];
    const bool on = tr >= 0.f;
    const float dt = on ? tr : 0.f;
    const float alpha = ga + t.H[0][k];
    const float pi = t.H[1][k] + 0.5f;
    const float xb = t.H[2][k] + 1.0f;
    const float xs = t.H[3][k] + 1.0f;
    const float mu = t.H[4][k] + 1.0f;
    const float beta = fminf(fmaxf(xb, 1e-10f), 10.f);
    const float sigma = fminf(fmaxf(xs, 1e-10f), 10.f);
    const float e = expf(logf(beta) - beta * dt);
    const float z = dt - mu;
    const float var = sigma * sigma;
    const float n = expf(-(z * z) / (2.f * var) - logf(sigma) - kLogSqrt2Pi);
    const float decay = pi * e + (1.f - pi) * n;
    if (on) {
      exc += alpha * decay;
      dga += decay;
    }
    if (GRAD) {
      const bool pb = xb >= 1e-10f && xb <= 10.f;
      const bool ps = xs >= 1e-10f && xs <= 10.f;
      const float an = alpha * (1.f - pi) * n;
      hrow[r] = on ? g * decay : 0.f;
      hrow[R + r] = on ? g * (alpha * (e - n)) : 0.f;
      hrow[2 * R + r] = (on && pb) ? g * (alpha * pi * e * (1.f / beta - dt)) : 0.f;
      hrow[3 * R + r] = (on && ps) ? g * (an * ((z * z) / (var * sigma) - 1.f / sigma)) : 0.f;
      hrow[4 * R + r] = on ? g * (an * (z / var)) : 0.f;
    }
  }
  return exc;
}

// ---- scores ---------------------------------------------------------------------------------------------------------------------
constexpr int kSlrcScoreU = 8;   // candidates per lane-group of one workgroup trip, all loads in flight before the first reduction

template <int D>
__global__ __launch_bounds__(kBlock) void slrc_scores_kernel(SlrcArgs a, int chunks) {
  constexpr int LPR = D / 4, G = 64 / LPR;
  constexpr int CPB = (kBlock / 64) * G * kSlrcScoreU;   // candidates per workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane / LPR, l = lane % LPR;
  const int64_t t = blockIdx.x / chunks;
  const int c0 = (int)(blockIdx.x % chunks) * CPB + wave * (G * kSlrcScoreU);
  if (c0 >= a.C) return;   // wave-uniform
  const int64_t u = a.uid[t];
  const float4 q4 = reinterpret_cast<const float4*>(a.t.U + u * D)[l];
  const int64_t* ids = a.iid + t * a.C;
  float4 r[kSlrcScoreU];
  int64_t id[kSlrcScoreU];
#pragma unroll
  for (int k = 0; k < kSlrcScoreU; ++k) {
    const int c = c0 + k * G + grp;
    id[k] = ids[c < a.C ? c : c0];
    r[k] = load_stream4(reinterpret_cast<const float4*>(a.t.I + id[k] * D) + l);
  }
  const float ubu = a.t.ub[u], ga = a.t.ga[0];
#pragma unroll
  for (int k = 0; k < kSlrcScoreU; ++k) {
    const int c = c0 + k * G + grp;
    const float p = row_allreduce_sum<LPR>(dot4(q4, r[k]));
    if (l == 0 && c < a.C) {
      const int64_t o = t * a.C + c;
      float dga;
      const float exc = slrc_excite<false>(a.t, id[k], a.iv + o * a.R, a.R, ga, nullptr, dga);
      a.pred[o] = ((p + ubu) + a.t.ib[id[k]]) + exc;
    }
  }
}

// ---- fused forward / loss / backward, register path -------------------------------------------------------------------------------
template <int CPL>
constexpr int slrc_min_waves() { return CPL >= 13 ? 2 : 4; }

template <int D, int CPL>
__global__ __launch_bounds__(kBlock, (slrc_min_waves<CPL>())) void slrc_fwd_bwd_kernel(SlrcArgs a) {
  constexpr int LPR = D / 4, G = 64 / LPR;
  constexpr int SLOTS = G * CPL;
  constexpr int NPL = (SLOTS + 63) / 64;
  __shared__ float strip_mem[(kBlock / 64) * SLOTS];

  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (t >= a.B) return;   // wave-uniform; only wave-level synchronisation below
  const int grp = lane / LPR, l = lane % LPR;
  const int C = a.C, R = a.R, R5 = 5 * a.R;
  float* strip = strip_mem + (threadIdx.x >> 6) * SLOTS;

  // ---- gather: the user row, then this group's CPL candidate rows, all loads in flight
  const int64_t u = a.uid[t];
  const float4 q4 = reinterpret_cast<const float4*>(a.t.U + u * D)[l];
  const int64_t* ids = a.iid + t * C;
  float4 r[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int c = j * G + grp;
    const int64_t id = ids[c < C ? c : 0];   // slots past C re-read candidate 0; masked below
    r[j] = load_stream4(reinterpret_cast<const float4*>(a.t.I + id * D) + l);
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const float pj = row_allreduce_sum<LPR>(dot4(q4, r[j]));
    if (l == 0) strip[grp * CPL + j] = pj;
  }
  slrc_wave_lds_sync();

  // ---- one lane per candidate (slot s = grp * CPL + j  <->  candidate c = j * G + grp): biases and excitation
  const float ubu = a.t.ub[u], ga = a.t.ga[0];
  float pc[NPL];
  int cc[NPL];
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int s = lane + k * 64;
    const int c = (s % CPL) * G + s / CPL;
    cc[k] = (s < SLOTS && c < C) ? c : -1;
    pc[k] = 0.f;
    if (cc[k] >= 0) {
      const int64_t id = ids[c];
      const int64_t o = t * C + c;
      float dga;
      const float exc = slrc_excite<false>(a.t, id, a.iv + o * R, R, ga, nullptr, dga);
      pc[k] = ((strip[s] + ubu) + a.t.ib[id]) + exc;
    }
  }
  const float pos = __shfl(pc[0], 0, 64);   // slot 0 is candidate 0
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < NPL; ++k)
    if (cc[k] >= 1) mx = fmaxf(mx, pc[k]);
  mx = wave_allreduce_max(mx);
  float ew[NPL], sg[NPL];
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    ew[k] = cc[k] >= 1 ? expf(pc[k] - mx) : 0.f;
    se += ew[k];
  }
  se = wave_allreduce_sum(se);
  const float inv_se = 1.0f / se;
  float P = 0.f, A = 0.f;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    ew[k] *= inv_se;
    sg[k] = sigmoidf_(pos - pc[k]);
    P = fmaf(ew[k], sg[k], P);
    A = fmaf(ew[k], sg[k] * (1.0f - sg[k]), A);
  }
  P = wave_allreduce_sum(P);
  A = wave_allreduce_sum(A);
  const BprRow br = bpr_row(P, a.inv_b);
  if (lane == 0) a.loss_vec[t] = br.loss;
  float gsum = 0.f, gda = 0.f;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int s = lane + k * 64;
    float g = br.dLdP * bpr_dP_dneg(ew[k], sg[k], P);
    if (cc[k] == 0) g = br.dLdP * A;
    if (cc[k] < 0) g = 0.f;
    if (s < SLOTS) strip[s] = g;
    if (cc[k] >= 0) {
      const int64_t o = t * C + cc[k];
      a.gpred[o] = g;
      if (a.pred != nullptr) a.pred[o] = pc[k];
      // the excitation again, now with g: its derivative rows are written once, already scaled (the five table rows were just
      // read by this lane; recomputing two expf per relation costs less than a round trip of the row through memory)
      float dga;
      slrc_excite<true>(a.t, ids[cc[k]], a.iv + o * R, R, ga, a.hgrad + o * R5, dga, g);
      gsum += g;
      gda = fmaf(g, dga, gda);
    }
  }
  gsum = wave_allreduce_sum(gsum);
  gda = wave_allreduce_sum(gda);
  if (lane == 0) {
    a.ubgrad[t] = gsum;
    a.gagrad[t] = gda;
  }
  slrc_wave_lds_sync();

  // ---- backward: ugrad = sum_c g_c I[i_c]
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int j = 0; j < CPL; ++j) slrc_fma4(acc, strip[grp * CPL + j], r[j]);   // broadcast read, 0 on slots past C
  acc.x = groups_allreduce_sum<LPR, 64>(acc.x);
  acc.y = groups_allreduce_sum<LPR, 64>(acc.y);
  acc.z = groups_allreduce_sum<LPR, 64>(acc.z);
  acc.w = groups_allreduce_sum<LPR, 64>(acc.w);
  if (grp == 0) reinterpret_cast<float4*>(a.ugrad + t * D)[l] = acc;
}

// ---- fused forward / loss / backward, streaming path: any C >= 2 -----------------------------------------------------------------
constexpr int kSlrcStreamU = 4;   // candidate rows in flight per lane-group

template <int D>
__global__ __launch_bounds__(kBlock) void slrc_fwd_bwd_stream_kernel(SlrcArgs a) {
  constexpr int LPR = D / 4, G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (t >= a.B) return;   // wave-uniform; no workgroup barrier in this kernel
  const int grp = lane / LPR, l = lane % LPR;
  const int C = a.C, R = a.R, R5 = 5 * a.R;
  const int64_t u = a.uid[t];
  const float4 q4 = reinterpret_cast<const float4*>(a.t.U + u * D)[l];
  const int64_t* ids = a.iid + t * C;
  float* stage = a.gpred + t * C;   // dot products, then scores, then the gradient scalars

  for (int c0 = 0; c0 < C; c0 += kSlrcStreamU * G) {
    float4 r[kSlrcStreamU];
#pragma unroll
    for (int k = 0; k < kSlrcStreamU; ++k) {
      const int c = c0 + k * G + grp;
      const int64_t id = ids[c < C ? c : 0];
      r[k] = reinterpret_cast<const float4*>(a.t.I + id * D)[l];   // (plain loads: the rows are read again below)
    }
#pragma unroll
    for (int k = 0; k < kSlrcStreamU; ++k) {
      const int c = c0 + k * G + grp;
      const float p = row_allreduce_sum<LPR>(dot4(q4, r[k]));
      if (l == 0 && c < C) stage[c] = p;
    }
  }
  __threadfence();   // the wave's own stores, read back by its other lanes
  __builtin_amdgcn_wave_barrier();

  // one lane per candidate: biases and excitation
  const float ubu = a.t.ub[u], ga = a.t.ga[0];
  for (int c = lane; c < C; c += 64) {
    const int64_t id = ids[c];
    const int64_t o = t * C + c;
    float dga;
    const float exc = slrc_excite<false>(a.t, id, a.iv + o * R, R, ga, nullptr, dga);
    stage[c] = ((stage[c] + ubu) + a.t.ib[id]) + exc;
  }
  __threadfence();
  __builtin_amdgcn_wave_barrier();

  const float pos = stage[0];
  float mx = -INFINITY;
  for (int c = 1 + lane; c < C; c += 64) mx = fmaxf(mx, stage[c]);
  mx = wave_allreduce_max(mx);
  float se = 0.f;
  for (int c = 1 + lane; c < C; c += 64) se += expf(stage[c] - mx);
  se = wave_allreduce_sum(se);
  const float inv_se = 1.0f / se;
  float P = 0.f, A = 0.f;
  for (int c = 1 + lane; c < C; c += 64) {
    const float pc = stage[c];
    const float w = expf(pc - mx) * inv_se;
    const float s = sigmoidf_(pos - pc);
    P = fmaf(w, s, P);
    A = fmaf(w, s * (1.0f - s), A);
  }
  P = wave_allreduce_sum(P);
  A = wave_allreduce_sum(A);
  const BprRow br = bpr_row(P, a.inv_b);
  if (lane == 0) a.loss_vec[t] = br.loss;
  __builtin_amdgcn_wave_barrier();   // every lane holds pos before slot 0 is overwritten
  float gsum = 0.f, gda = 0.f;
  for (int c = lane; c < C; c += 64) {   // each lane overwrites only the slots it read itself
    const float pc = stage[c];
    float g;
    if (c == 0) {
      g = br.dLdP * A;
    } else {
      const float w = expf(pc - mx) * inv_se;
      const float s = sigmoidf_(pos - pc);
      g = br.dLdP * bpr_dP_dneg(w, s, P);
    }
    const int64_t o = t * C + c;
    if (a.pred != nullptr) a.pred[o] = pc;
    stage[c] = g;
    float dga;   // the excitation again, now with g: the derivative rows are written once, already scaled
    slrc_excite<true>(a.t, ids[c], a.iv + o * R, R, ga, a.hgrad + o * R5, dga, g);
    gsum += g;
    gda = fmaf(g, dga, gda);
  }
  gsum = wave_allreduce_sum(gsum);
  gda = wave_allreduce_sum(gda);
  if (lane == 0) {
    a.ubgrad[t] = gsum;
    a.gagrad[t] = gda;
  }
  __threadfence();
  __builtin_amdgcn_wave_barrier();

  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c0 = 0; c0 < C; c0 += kSlrcStreamU * G) {
    float4 r[kSlrcStreamU];
    float g[kSlrcStreamU];
#pragma unroll
    for (int k = 0; k < kSlrcStreamU; ++k) {
      const int c = c0 + k * G + grp;
      const int64_t id = ids[c < C ? c : 0];
      r[k] = reinterpret_cast<const float4*>(a.t.I + id * D)[l];
      g[k] = c < C ? stage[c] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kSlrcStreamU; ++k) slrc_fma4(acc, g[k], r[k]);
  }
  acc.x = groups_allreduce_sum<LPR, 64>(acc.x);
  acc.y = groups_allreduce_sum<LPR, 64>(acc.y);
  acc.z = groups_allreduce_sum<LPR, 64>(acc.z);
  acc.w = groups_allreduce_sum<LPR, 64>(acc.w);
  if (grp == 0) reinterpret_cast<float4*>(a.ugrad + t * D)[l] = acc;
}

// ---- backward of the biases and the excitation for a GIVEN gpred (the autograd node of the dense engine: any loss on the scores) -----
// One wave per tuple, one lane per candidate (c = lane, lane + 64, ...): the hgrad row scaled by gpred, and the per-tuple sums
// ubgrad = sum_c g, gagrad = sum_c g * d pred / d global_alpha (per lane in ascending c, then the wave's fixed tree).
__global__ __launch_bounds__(kBlock) void slrc_excite_bwd_kernel(SlrcArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (t >= a.B) return;   // wave-uniform
  const int C = a.C, R = a.R, R5 = 5 * a.R;
  const float ga = a.t.ga[0];
  float gsum = 0.f, gda = 0.f;
  for (int c = lane; c < C; c += 64) {
    const int64_t o = t * C + c;
    const float g = a.gpred[o];
    float dga;
    slrc_excite<true>(a.t, a.iid[o], a.iv + o * R, R, ga, a.hgrad + o * R5, dga, g);
    gsum += g;
    gda = fmaf(g, dga, gda);
  }
  gsum = wave_allreduce_sum(gsum);
  gda = wave_allreduce_sum(gda);
  if (lane == 0) {
    a.ubgrad[t] = gsum;
    a.gagrad[t] = gda;
  }
}

// ---- item-side update: all seven item tables in one pass over the sorted candidate ids ----------------------------------------------
// One lane-group (LPR = d / 4 lanes) per listed head.  Over the segment's occurrences o = perm[j] in ascending sorted position it sums
// gpred[o] * U[uid[o / C]] (one float4 per lane), gpred[o] (item_bias) and the 5 R floats of hgrad[o] (lane l takes elements l,
// l + LPR, ...), then applies the optimizer to (or writes the dense gradient of) row `key` of every table: I with the step's l2, the
// five Hawkes tables with the step's l2, item_bias with l2 = 0.  Rows with more than kSlrcLongSeg occurrences are listed (integer
// atomic: the list order decides which workgroup takes which row, never the order of a sum) and taken by one workgroup each, whose
// lane-groups stride over the segment in a fixed pattern and combine in a fixed LDS tree.
struct SlrcUpd {
  float* W[kSlrcTables];
  float* M[kSlrcTables];
  float* V[kSlrcTables];
  float* dense[kSlrcTables];
  const float* U;
  const int64_t* uid;
  const uint32_t* keys;
  const uint32_t* perm;
  int64_t n_occ;
  const float* gpred;
  const float* hgrad;
  int C, R;
  const uint32_t* heads;
  const uint32_t* n_heads;
  uint32_t* n_long;
  uint32_t* long_list;
  uint32_t long_cap;
  OptScalars o;        // the step's hyper-parameters
  OptScalars o_bias;   // the same with l2 = 0 ('bias' parameters take no weight decay, models/BaseModel.py:64-73)
};

template <int LPR>
constexpr int slrc_kpl() { return (5 * kSlrcMaxR + LPR - 1) / LPR; }   // hgrad elements per lane

template <int LPR>
struct SlrcAcc {
  float4 i4;
  float b;
  float h[slrc_kpl<LPR>()];
  __device__ __forceinline__ void zero() {
    i4 = make_float4(0.f, 0.f, 0.f, 0.f);
    b = 0.f;
#pragma unroll
    for (int q = 0; q < slrc_kpl<LPR>(); ++q) h[q] = 0.f;
  }
};

// adds occurrence o's contribution (ascending-position order is the caller's)
template <int D>
__device__ __forceinline__ void slrc_occ_add(const SlrcUpd& a, uint32_t o, int l, SlrcAcc<D / 4>& acc) {
  constexpr int LPR = D / 4;
  const float g = a.gpred[o];
  const int64_t row = a.uid[o / (uint32_t)a.C];
  const float4 s = reinterpret_cast<const float4*>(a.U + row * D)[l];
  acc.i4.x += g * s.x;
  acc.i4.y += g * s.y;
  acc.i4.z += g * s.z;
  acc.i4.w += g * s.w;
  acc.b += g;
  const int R5 = 5 * a.R;
  const float* hrow = a.hgrad + (size_t)o * R5;
#pragma unroll
  for (int q = 0; q < slrc_kpl<LPR>(); ++q) {
    const int k = l + q * LPR;
    if (k < R5) acc.h[q] += hrow[k];
  }
}

// one float of table `tix` (runtime index, per lane): select, not a dynamically indexed kernel argument
template <class T>
__device__ __forceinline__ T* slrc_pick(T* const (&p)[kSlrcTables], int tix) {
  T* r = p[0];
#pragma unroll
  for (int k = 1; k < kSlrcTables; ++k) r = (tix == k) ? p[k] : r;
  return r;
}

template <int MODE>
__device__ __forceinline__ void slrc_apply1(const SlrcUpd& a, const OptScalars& o, int tix, size_t idx, float g) {
  if (MODE == MODE_DENSE_GRAD) {
    slrc_pick(a.dense, tix)[idx] = g;
    return;
  }
  float* W = slrc_pick(a.W, tix);
  float w = W[idx], m = 0.f, v = 0.f;
  if (mode_has_m(MODE)) m = slrc_pick(a.M, tix)[idx];
  if (mode_has_v(MODE)) v = slrc_pick(a.V, tix)[idx];
  opt_elem<MODE>(o, g, w, m, v);
  W[idx] = w;
  if (mode_has_m(MODE)) slrc_pick(a.M, tix)[idx] = m;
  if (mode_has_v(MODE)) slrc_pick(a.V, tix)[idx] = v;
}

template <int D, int MODE>
__device__ __forceinline__ void slrc_apply_row(const SlrcUpd& a, uint32_t key, int l, const SlrcAcc<D / 4>& acc) {
  constexpr int LPR = D / 4;
  const size_t idx4 = (size_t)key * LPR + l;
  if (MODE == MODE_DENSE_GRAD) {
    reinterpret_cast<float4*>(a.dense[0])[idx4] = acc.i4;
  } else {
    const float4 w = load_stream4(reinterpret_cast<const float4*>(a.W[0]) + idx4);
    opt_row4<MODE>(a.o, a.W[0], a.M[0], a.V[0], idx4, w, acc.i4);
  }
  if (l == 0) slrc_apply1<MODE>(a, a.o_bias, 1, key, acc.b);
  const int R5 = 5 * a.R;
#pragma unroll
  for (int q = 0; q < slrc_kpl<LPR>(); ++q) {
    const int k = l + q * LPR;
    if (k < R5) slrc_apply1<MODE>(a, a.o, 2 + k / a.R, (size_t)key * a.R + (k % a.R), acc.h[q]);
  }
}

template <int D, int MODE>
__global__ __launch_bounds__(kBlock) void slrc_item_update_kernel(SlrcUpd a) {
  constexpr int LPR = D / 4, GPB = kBlock / LPR;
  const int l = threadIdx.x % LPR;
  const int64_t n = a.n_occ;
  const int64_t nh = (int64_t)*a.n_heads;
  const int64_t g = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
  if (g >= nh) return;   // no cross-lane operation in this kernel
  const int64_t j = a.heads[g];
  const uint32_t key = a.keys[j];
  if (j + kSlrcLongSeg < n && a.keys[j + kSlrcLongSeg] == key) {   // keys are sorted: one probe decides; left to the long-row kernel
    if (l == 0) {
      const uint32_t slot = atomicAdd(a.n_long, 1u);
      if (slot < a.long_cap) a.long_list[slot] = (uint32_t)j;
    }
    return;
  }
  SlrcAcc<LPR> acc;
  acc.zero();
  for (int64_t jj = j; jj < n && a.keys[jj] == key; ++jj) slrc_occ_add<D>(a, a.perm[jj], l, acc);
  slrc_apply_row<D, MODE>(a, key, l, acc);
}

template <int D, int MODE>
__global__ __launch_bounds__(kBlock) void slrc_item_update_long_kernel(SlrcUpd a) {
  constexpr int LPR = D / 4, GPB = kBlock / LPR, KPL = slrc_kpl<LPR>();
  __shared__ float4 part4[kBlock];
  __shared__ float partb[kBlock];
  __shared__ float parth[KPL][kBlock];
  const int l = threadIdx.x % LPR, g = threadIdx.x / LPR;
  const int64_t n = a.n_occ;
  uint32_t n_long = *a.n_long;
  if (n_long > a.long_cap) n_long = a.long_cap;
  for (uint32_t i = blockIdx.x; i < n_long; i += gridDim.x) {   // workgroup-uniform
    const int64_t j0 = a.long_list[i];
    const uint32_t key = a.keys[j0];
    SlrcAcc<LPR> acc;
    acc.zero();
    // lane-group g takes positions j0 + g, j0 + g + GPB, ... in ascending order
    for (int64_t jj = j0 + g; jj < n && a.keys[jj] == key; jj += GPB) slrc_occ_add<D>(a, a.perm[jj], l, acc);
    part4[threadIdx.x] = acc.i4;
    partb[threadIdx.x] = acc.b;
#pragma unroll
    for (int q = 0; q < KPL; ++q) parth[q][threadIdx.x] = acc.h[q];
#pragma unroll
    for (int off = GPB / 2; off >= 1; off >>= 1) {
      __syncthreads();
      if (g < off) {
        const int p = threadIdx.x + off * LPR;
        float4 x = part4[threadIdx.x];
        const float4 y = part4[p];
        x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
        part4[threadIdx.x] = x;
        partb[threadIdx.x] += partb[p];
#pragma unroll
        for (int q = 0; q < KPL; ++q) parth[q][threadIdx.x] += parth[q][p];
      }
    }
    __syncthreads();
    if (g == 0) {
      acc.i4 = part4[threadIdx.x];
      acc.b = partb[threadIdx.x];
#pragma unroll
      for (int q = 0; q < KPL; ++q) acc.h[q] = parth[q][threadIdx.x];
      slrc_apply_row<D, MODE>(a, key, l, acc);
    }
    __syncthreads();   // the partials are reused by the next row
  }
}

// ---- user_bias: one float per row.  One thread per sorted position; the thread at a segment's head sums its occurrences in ascending
// position and applies the optimizer with l2 = 0 (or writes the dense gradient).
template <int MODE>
__global__ __launch_bounds__(kBlock) void slrc_user_bias_kernel(float* W, float* M, float* V, float* dense, const uint32_t* keys,
                                                                 const uint32_t* perm, int64_t n, const float* ubgrad, OptScalars o) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const uint32_t key = keys[j];
  if (j > 0 && keys[j - 1] == key) return;
  float g = 0.f;
  for (int64_t jj = j; jj < n && keys[jj] == key; ++jj) g += ubgrad[perm[jj]];
  if (MODE == MODE_DENSE_GRAD) {
    dense[key] = g;
    return;
  }
  float w = W[key], m = 0.f, v = 0.f;
  if (mode_has_m(MODE)) m = M[key];
  if (mode_has_v(MODE)) v = V[key];
  opt_elem<MODE>(o, g, w, m, v);
  W[key] = w;
  if (mode_has_m(MODE)) M[key] = m;
  if (mode_has_v(MODE)) V[key] = v;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static bool slrc_width_ok(int d) { return d == 16 || d == 32 || d == 64 || d == 128; }

static int slrc_shape_check(const char* who, int d, int C, int R, int min_c) {
  RC_REQUIRE(slrc_width_ok(d), "%s: emb_size d=%d has no kernel (16, 32, 64, 128)", who, d);
  RC_REQUIRE(C >= min_c, "%s: need C >= %d candidates, got %d", who, min_c, C);
  RC_REQUIRE(R >= 1 && R <= kSlrcMaxR, "%s: relation_num R=%d outside 1..%d (item relations + 1)", who, R, kSlrcMaxR);
  return RC_OK;
}

// rows per lane-group on the register path of (d, C); 0: the streaming path
static int slrc_pick_cpl(int d, int C) {
  static const int buckets[] = {1, 2, 4, 8, 13, kSlrcMaxCpl};
  if (!slrc_width_ok(d) || C < 2) return 0;
  const int G = 256 / d;
  const int need = (C + G - 1) / G;
  for (int b : buckets)
    if (need <= b) return b;
  return 0;
}

static int slrc_fill_args(const char* who, SlrcArgs* a, const float* U, const float* I, const float* user_bias, const float* item_bias,
                          const float* global_alpha, const float* alphas, const float* pis, const float* betas, const float* sigmas,
                          const float* mus, const int64_t* uid, const int64_t* iid, const float* intervals, int B, int C, int d, int R,
                          int min_c) {
  RC_REQUIRE(U && I && user_bias && item_bias && global_alpha && alphas && pis && betas && sigmas && mus && uid && iid && intervals,
             "%s: null pointer", who);
  RC_TRY(slrc_shape_check(who, d, C, R, min_c));
  RC_REQUIRE(B > 0, "%s: need B >= 1, got B=%d", who, B);
  RC_REQUIRE((int64_t)B * C * 5 * R < ((int64_t)1 << 40), "%s: B * C too large (B=%d C=%d)", who, B, C);
  RC_REQUIRE(aligned16(U, I), "%s: U and I must be 16-byte aligned", who);
  memset(a, 0, sizeof(*a));
  a->t.U = U; a->t.I = I; a->t.ub = user_bias; a->t.ib = item_bias; a->t.ga = global_alpha;
  a->t.H[0] = alphas; a->t.H[1] = pis; a->t.H[2] = betas; a->t.H[3] = sigmas; a->t.H[4] = mus;
  a->uid = uid; a->iid = iid; a->iv = intervals; a->B = B; a->C = C; a->R = R;
  return RC_OK;
}

template <int D>
static int dispatch_slrc_reg(const SlrcArgs& a, int cpl, hipStream_t s) {
  return dispatch_or_fail<1, 2, 4, 8, 13, kSlrcMaxCpl>("rc_slrc_fwd_bwd", "rows per lane-group", cpl, [&](auto CPL) -> int {
    const int blocks = (a.B + (kBlock / 64) - 1) / (kBlock / 64);
    hipLaunchKernelGGL((slrc_fwd_bwd_kernel<D, CPL()>), dim3(blocks), dim3(kBlock), 0, s, a);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

struct SlrcWs {
  uint32_t* n_long;
  uint32_t* long_list;
  uint32_t long_cap;
  size_t total;
};

static SlrcWs carve_slrc_ws(void* base, int64_t n_occ) {
  Carver cv(base);
  SlrcWs w;
  w.long_cap = (uint32_t)(n_occ / (kSlrcLongSeg + 1)) + 1;   // rows with more than kSlrcLongSeg occurrences
  w.n_long = cv.take<uint32_t>(1);
  w.long_list = cv.take<uint32_t>(w.long_cap);
  w.total = cv.off;
  return w;
}

}  // namespace rc

using namespace rc;

extern "C" enum rc_status rc_slrc_check_shape(int d, int C, int R) {
  return (enum rc_status)slrc_shape_check("rc_slrc_check_shape", d, C, R, 1);
}

extern "C" size_t rc_slrc_fwd_bwd_layout(int d, int C, int R) {
  if (R < 1 || R > kSlrcMaxR) return 0;
  return (size_t)slrc_pick_cpl(d, C);
}

extern "C" enum rc_status rc_slrc_scores(const float* U, const float* I, const float* user_bias, const float* item_bias,
                                         const float* global_alpha, const float* alphas, const float* pis, const float* betas,
                                         const float* sigmas, const float* mus, const int64_t* uid, const int64_t* iid,
                                         const float* intervals, int B, int C, int d, int R, float* pred, rc_stream_t stream) {
  static const char* who = "rc_slrc_scores";
  if (B == 0) return RC_OK;
  SlrcArgs a;
  int rc = slrc_fill_args(who, &a, U, I, user_bias, item_bias, global_alpha, alphas, pis, betas, sigmas, mus, uid, iid, intervals, B, C,
                          d, R, 1);
  if (rc != RC_OK) return (enum rc_status)rc;
  if (pred == nullptr) return (enum rc_status)fail(RC_ERR_INVALID_ARG, "%s: null pointer", who);
  a.pred = pred;
  hipStream_t s = as_stream(stream);
  return (enum rc_status)dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", d, [&](auto D) -> int {
    constexpr int CPB = (kBlock / 64) * (256 / D()) * kSlrcScoreU;
    const int64_t chunks = ((int64_t)C + CPB - 1) / CPB;
    const int64_t blocks = chunks * B;
    if (blocks > kMaxGridX) return fail(RC_ERR_UNSUPPORTED, "%s: grid too large (B=%d C=%d)", who, B, C);
    hipLaunchKernelGGL((slrc_scores_kernel<D()>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a, (int)chunks);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

extern "C" enum rc_status rc_slrc_fwd_bwd(const float* U, const float* I, const float* user_bias, const float* item_bias,
                                          const float* global_alpha, const float* alphas, const float* pis, const float* betas,
                                          const float* sigmas, const float* mus, const int64_t* uid, const int64_t* iid,
                                          const float* intervals, int B, int C, int d, int R, float inv_b, float* pred, float* loss_vec,
                                          float* gpred, float* ugrad, float* ubgrad, float* hgrad, float* gagrad, rc_stream_t stream) {
  static const char* who = "rc_slrc_fwd_bwd";
  if (B == 0) return RC_OK;
  SlrcArgs a;
  int rc = slrc_fill_args(who, &a, U, I, user_bias, item_bias, global_alpha, alphas, pis, betas, sigmas, mus, uid, iid, intervals, B, C,
                          d, R, 2);
  if (rc != RC_OK) return (enum rc_status)rc;
  if (!(loss_vec && gpred && ugrad && ubgrad && hgrad && gagrad)) return (enum rc_status)fail(RC_ERR_INVALID_ARG, "%s: null pointer", who);
  if (!aligned16(ugrad)) return (enum rc_status)fail(RC_ERR_INVALID_ARG, "%s: ugrad must be 16-byte aligned", who);
  a.inv_b = inv_b; a.pred = pred; a.loss_vec = loss_vec; a.gpred = gpred; a.ugrad = ugrad; a.ubgrad = ubgrad; a.hgrad = hgrad;
  a.gagrad = gagrad;
  hipStream_t s = as_stream(stream);
  const int cpl = slrc_pick_cpl(d, C);
  return (enum rc_status)dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", d, [&](auto D) -> int {
    if (cpl > 0) return dispatch_slrc_reg<D()>(a, cpl, s);
    const int blocks = (B + (kBlock / 64) - 1) / (kBlock / 64);
    hipLaunchKernelGGL((slrc_fwd_bwd_stream_kernel<D()>), dim3(blocks), dim3(kBlock), 0, s, a);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

extern "C" enum rc_status rc_slrc_excitation_bwd(const float* global_alpha, const float* alphas, const float* pis, const float* betas,
                                                 const float* sigmas, const float* mus, const int64_t* iid, const float* intervals,
                                                 const float* gpred, int B, int C, int R, float* hgrad, float* ubgrad, float* gagrad,
                                                 rc_stream_t stream) {
  static const char* who = "rc_slrc_excitation_bwd";
  if (B == 0) return RC_OK;
  if (!(global_alpha && alphas && pis && betas && sigmas && mus && iid && intervals && gpred && hgrad && ubgrad && gagrad))
    return (enum rc_status)fail(RC_ERR_INVALID_ARG, "%s: null pointer", who);
  int rc = slrc_shape_check(who, 64, C, R, 1);
  if (rc != RC_OK) return (enum rc_status)rc;
  if (B < 0 || (int64_t)B * C * 5 * R >= ((int64_t)1 << 40))
    return (enum rc_status)fail(RC_ERR_INVALID_ARG, "%s: bad shape B=%d C=%d", who, B, C);
  SlrcArgs a;
  memset(&a, 0, sizeof(a));
  a.t.ga = global_alpha;
  a.t.H[0] = alphas; a.t.H[1] = pis; a.t.H[2] = betas; a.t.H[3] = sigmas; a.t.H[4] = mus;
  a.iid = iid; a.iv = intervals; a.gpred = const_cast<float*>(gpred); a.B = B; a.C = C; a.R = R;
  a.hgrad = hgrad; a.ubgrad = ubgrad; a.gagrad = gagrad;
  const int blocks = (B + (kBlock / 64) - 1) / (kBlock / 64);
  hipLaunchKernelGGL(slrc_excite_bwd_kernel, dim3(blocks), dim3(kBlock), 0, as_stream(stream), a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (enum rc_status)fail(RC_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  return RC_OK;
}

extern "C" size_t rc_slrc_item_update_workspace_bytes(int64_t n_occ, int d) {
  (void)d;
  if (n_occ < 1) n_occ = 1;
  return carve_slrc_ws(nullptr, n_occ).total;
}

static int slrc_item_update_impl(float* const* W, float* const* M, float* const* V, int d, int R, const uint32_t* keys,
                                 const uint32_t* perm, int64_t n_occ, const float* gpred, const float* hgrad, const float* U,
                                 const int64_t* uid, int C, const rc_opt_hyper* h, float* const* dense_grad, const uint32_t* heads,
                                 const uint32_t* n_heads, void* ws, size_t ws_bytes, rc_stream_t stream) {
  static const char* who = "rc_slrc_item_update";
  if (n_occ == 0) return RC_OK;
  const bool dense = dense_grad != nullptr;
  if (dense) {
    int given = 0;
    for (int k = 0; k < kSlrcTables; ++k) given += dense_grad[k] != nullptr;
    RC_REQUIRE(given == kSlrcTables, "%s: all seven dense gradients or none (got %d)", who, given);
  }
  RC_REQUIRE(keys && perm && gpred && hgrad && U && uid && ws, "%s: null pointer", who);
  RC_REQUIRE(heads && n_heads, "%s: the head list of rc_segment_heads is required", who);
  RC_REQUIRE(dense || W != nullptr, "%s: no output (the seven tables, or the dense gradients)", who);
  RC_TRY(slrc_shape_check(who, d, C, R, 1));
  RC_REQUIRE(n_occ > 0 && n_occ < ((int64_t)1 << 31), "%s: bad shape n_occ=%lld", who, (long long)n_occ);
  SlrcUpd a;
  memset(&a, 0, sizeof(a));
  int mode = MODE_DENSE_GRAD;
  if (!dense) {
    bool have_m = M != nullptr, have_v = V != nullptr;
    for (int k = 0; k < kSlrcTables; ++k) {
      RC_REQUIRE(W[k] != nullptr, "%s: no output (table %d of seven is null)", who, k);
      RC_REQUIRE(W[k] != U, "%s: U must be distinct from the item tables", who);
      a.W[k] = W[k];
      have_m = have_m && M[k] != nullptr;
      have_v = have_v && V[k] != nullptr;
    }
    RC_TRY(fill_opt_scalars(who, h, &a.o));
    a.o_bias = a.o;
    a.o_bias.l2 = 0.f;
    mode = mode_of(h);
    RC_TRY(opt_state_check(who, mode, have_m, have_v));
    for (int k = 0; k < kSlrcTables; ++k) {
      a.M[k] = mode_has_m(mode) ? M[k] : nullptr;
      a.V[k] = mode_has_v(mode) ? V[k] : nullptr;
    }
    RC_REQUIRE(aligned16(a.W[0], a.M[0], a.V[0]), "%s: I and its state must be 16-byte aligned", who);
  } else {
    for (int k = 0; k < kSlrcTables; ++k) a.dense[k] = dense_grad[k];
    RC_REQUIRE(aligned16(a.dense[0]), "%s: the dense gradient of I must be 16-byte aligned", who);
  }
  RC_REQUIRE(aligned16(U), "%s: U must be 16-byte aligned", who);
  const SlrcWs w = carve_slrc_ws(ws, n_occ);
  if (ws_bytes < w.total) return fail(RC_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, w.total);
  a.U = U; a.uid = uid; a.keys = keys; a.perm = perm; a.n_occ = n_occ; a.gpred = gpred; a.hgrad = hgrad; a.C = C; a.R = R;
  a.heads = heads; a.n_heads = n_heads; a.n_long = w.n_long; a.long_list = w.long_list; a.long_cap = w.long_cap;
  hipStream_t s = as_stream(stream);
  RC_HIP(hipMemsetAsync(w.n_long, 0, sizeof(uint32_t), s));
  return dispatch_or_fail<MODE_DENSE_GRAD, MODE_SGD, MODE_ADAM, MODE_ADAGRAD>(who, "update mode", mode, [&](auto MD) -> int {
    return dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", d, [&](auto D) -> int {
      constexpr int GPB = kBlock / (D() / 4);              // heads per workgroup
      const int64_t blocks = (n_occ + GPB - 1) / GPB;      // upper bound on the listed heads: every position
      if (blocks > kMaxGridX) return fail(RC_ERR_UNSUPPORTED, "%s: grid too large", who);
      hipLaunchKernelGGL((slrc_item_update_kernel<D(), MD()>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
      RC_LAUNCH_CHECK();
      if (n_occ > kSlrcLongSeg) {   // otherwise no segment can be long
        const unsigned long_blocks = a.long_cap < 2048u ? a.long_cap : 2048u;
        hipLaunchKernelGGL((slrc_item_update_long_kernel<D(), MD()>), dim3(long_blocks), dim3(kBlock), 0, s, a);
        RC_LAUNCH_CHECK();
      }
      return RC_OK;
    });
  });
}

extern "C" enum rc_status rc_slrc_item_update(float* const* W, float* const* M, float* const* V, int d, int R, const uint32_t* keys,
                                              const uint32_t* perm, int64_t n_occ, const float* gpred, const float* hgrad,
                                              const float* U, const int64_t* uid, int C, const rc_opt_hyper* h,
                                              float* const* dense_grad, const uint32_t* heads, const uint32_t* n_heads, void* ws,
                                              size_t ws_bytes, rc_stream_t stream) {
  return (enum rc_status)slrc_item_update_impl(W, M, V, d, R, keys, perm, n_occ, gpred, hgrad, U, uid, C, h, dense_grad, heads,
                                               n_heads, ws, ws_bytes, stream);
}

static int slrc_user_bias_impl(float* user_bias, float* m, float* v, const uint32_t* keys, const uint32_t* perm, int64_t n_occ,
                               const float* ubgrad, const rc_opt_hyper* h, float* dense_grad, rc_stream_t stream) {
  static const char* who = "rc_slrc_user_bias_update";
  if (n_occ == 0) return RC_OK;
  const bool dense = dense_grad != nullptr;
  RC_REQUIRE(keys && perm && ubgrad, "%s: null pointer", who);
  RC_REQUIRE(dense || user_bias, "%s: no output (user_bias, or the dense gradient)", who);
  RC_REQUIRE(n_occ > 0 && n_occ < ((int64_t)1 << 31), "%s: bad shape n_occ=%lld", who, (long long)n_occ);
  OptScalars o;
  memset(&o, 0, sizeof(o));
  int mode = MODE_DENSE_GRAD;
  if (!dense) {
    RC_TRY(fill_opt_scalars(who, h, &o));
    o.l2 = 0.f;   // 'bias' parameters take no weight decay
    mode = mode_of(h);
    RC_TRY(opt_state_check(who, mode, m != nullptr, v != nullptr));
  }
  hipStream_t s = as_stream(stream);
  const int64_t blocks = (n_occ + kBlock - 1) / kBlock;
  return dispatch_or_fail<MODE_DENSE_GRAD, MODE_SGD, MODE_ADAM, MODE_ADAGRAD>(who, "update mode", mode, [&](auto MD) -> int {
    hipLaunchKernelGGL((slrc_user_bias_kernel<MD()>), dim3((unsigned)blocks), dim3(kBlock), 0, s, user_bias, m, v, dense_grad, keys,
                       perm, n_occ, ubgrad, o);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

extern "C" enum rc_status rc_slrc_user_bias_update(float* user_bias, float* m, float* v, const uint32_t* keys, const uint32_t* perm,
                                                   int64_t n_occ, const float* ubgrad, const rc_opt_hyper* h, float* dense_grad,
                                                   rc_stream_t stream) {
  return (enum rc_status)slrc_user_bias_impl(user_bias, m, v, keys, perm, n_occ, ubgrad, h, dense_grad, stream);
}
