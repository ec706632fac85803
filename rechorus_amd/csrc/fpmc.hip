// fpmc.hip -- FPMC (Rendle et al., WWW 2010; reference models/sequential/FPMC.py:44-56): four embedding tables, two dot
// products per candidate,
//     pred[b, c] = <UI[uid[b]], IU[iid[b, c]]> + <LI[lid[b]], IL[iid[b, c]]>,
// with GeneralModel.loss (models/BaseModel.py:182-185) on top.  Scores, the fused forward / loss / backward-to-query-rows and the
// item-side row update of the two candidate tables in one pass over the sorted candidate ids.
//
// Lane algebra: the PAIR ROW.  A candidate's two rows (IU[i] | IL[i]) are treated as one row of 2 d floats against the tuple's
// query row (UI[u] | LI[l]): LPR = d / 2 consecutive lanes own a candidate, the lower d / 4 lanes one float4 of the IU row each,
// the upper d / 4 lanes one float4 of the IL row.  One DPP row reduction over the LPR lanes then yields the SUM of the two dot
// products (the lower half reduces the first term, the upper half the second, the last step adds them), and in the backward pass
// the lower lanes accumulate ugrad = sum_c g_c IU[i_c] while the upper lanes accumulate lgrad = sum_c g_c IL[i_c].  Every
// candidate row is read once, as one coalesced 4 d-byte segment per table.
//
// Paths of rc_fpmc_fwd_bwd (rc_fpmc_fwd_bwd_layout reports the choice):
//   register   G = 128 / d lane-groups per wave, each holding CPL = ceil(C / G) <= 50 pair rows (4 CPL VGPRs per lane): the whole
//              candidate block of a tuple -- 51.2 KB at d = 64, C = 100 -- stays in one wave's registers between the score and the
//              backward sum, two waves per SIMD.  The loss goes through a C-float LDS strip per tuple, one lane per candidate, as
//              in fused_body.hpp.  Envelope C <= 50 * 128 / d (d = 16: 33 rows): 264 / 200 / 100 / 50 candidates at d = 16 / 32 / 64 / 128.
//   streaming  any C >= 2: one wave per tuple, the scores staged in the tuple's own gpred row (global memory: no LDS bound on C),
//              the candidate rows re-read for the backward sum (they were just read by the same wave: L2 hits).
// No floating-point atomics; every sum has a fixed order.
#include "bpr_math.hpp"
#include "common.hpp"
#include "fused_body.hpp"
#include "opt_math.hpp"

namespace rc {

constexpr int kFpmcMaxCpl = 50;    // pair rows per lane-group on the register path (200 of the 256 VGPRs of a two-wave SIMD)
constexpr int kFpmcLongSeg = 32;   // occurrences one lane-group sums on its own in the item update

struct FpmcArgs {
  const float* UI;
  const float* LI;
  const float* IU;
  const float* IL;
  const int64_t* uid;
  const int64_t* lid;
  const int64_t* iid;
  int B, C;
  float inv_b;
  float* pred;
  float* loss_vec;
  float* gpred;
  float* ugrad;
  float* lgrad;
};

// the float4 of the pair row (A[ra] | Bt[rb]) that lane l of LPR = D / 2 owns
template <int D>
__device__ __forceinline__ const float4* pair_slot(const float* A, const float* Bt, int64_t ra, int64_t rb, int l) {
  constexpr int H = D / 4;
  const bool up = l >= H;
  return reinterpret_cast<const float4*>((up ? Bt : A) + (up ? rb : ra) * D) + (up ? l - H : l);
}

__device__ __forceinline__ void fma4(float4& acc, float g, const float4& r) {
  acc.x = fmaf(g, r.x, acc.x);
  acc.y = fmaf(g, r.y, acc.y);
  acc.z = fmaf(g, r.z, acc.z);
  acc.w = fmaf(g, r.w, acc.w);
}

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- scores ---------------------------------------------------------------------------------------------------------------------
// A workgroup takes kScoreU candidates per lane-group of one tuple (all loads in flight before the first reduction).
constexpr int kScoreU = 8;

template <int D>
__global__ __launch_bounds__(kBlock) void fpmc_scores_kernel(FpmcArgs a, int chunks) {
  constexpr int LPR = D / 2, G = 64 / LPR;
  constexpr int CPB = (kBlock / 64) * G * kScoreU;   // candidates per workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane / LPR, l = lane % LPR;
  const int64_t t = blockIdx.x / chunks;
  const int c0 = (int)(blockIdx.x % chunks) * CPB + wave * (G * kScoreU);
  if (c0 >= a.C) return;   // wave-uniform
  const float4 q4 = *pair_slot<D>(a.UI, a.LI, a.uid[t], a.lid[t], l);
  const int64_t* ids = a.iid + t * a.C;
  float4 r[kScoreU];
#pragma unroll
  for (int u = 0; u < kScoreU; ++u) {
    const int c = c0 + u * G + grp;
    const int64_t id = ids[c < a.C ? c : c0];
    r[u] = load_stream4(pair_slot<D>(a.IU, a.IL, id, id, l));
  }
#pragma unroll
  for (int u = 0; u < kScoreU; ++u) {
    const int c = c0 + u * G + grp;
    const float p = row_allreduce_sum<LPR>(dot4(q4, r[u]));
    if (l == 0 && c < a.C) a.pred[t * a.C + c] = p;
  }
}

// ---- fused forward / loss / backward, register path -------------------------------------------------------------------------------
template <int CPL>
constexpr int fpmc_min_waves() { return CPL >= 26 ? 2 : (CPL >= 20 ? 3 : 4); }

template <int D, int GS, int CPL>
__global__ __launch_bounds__(kBlock, (fpmc_min_waves<CPL>())) void fpmc_fwd_bwd_kernel(FpmcArgs a) {
  constexpr int H = D / 4, LPR = D / 2;
  constexpr int S = LPR * GS;
  static_assert(S <= 64 && (64 % S) == 0, "tuple must fit a wave");
  constexpr int TPW = 64 / S;
  constexpr int SLOTS = GS * CPL;
  constexpr int NPL = (SLOTS + S - 1) / S;
  __shared__ float strip_mem[(kBlock / 64) * TPW * SLOTS];

  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const int64_t t_raw = wave * TPW + lane / S;
  const bool tv = t_raw < a.B;
  const int64_t t = tv ? t_raw : (int64_t)a.B - 1;   // clamp: every lane stays in the shuffles
  const int sub = lane % S;
  const int grp = sub / LPR;
  const int l = sub % LPR;
  const int C = a.C;
  float* strip = strip_mem + ((threadIdx.x >> 6) * TPW + lane / S) * SLOTS;

  // ---- gather: the query pair row, then this group's CPL candidate pair rows, all loads in flight
  const float4 q4 = *pair_slot<D>(a.UI, a.LI, a.uid[t], a.lid[t], l);
  const int64_t* ids = a.iid + t * C;
  float4 r[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int c = j * GS + grp;
    const int64_t id = ids[c < C ? c : 0];   // slots past C re-read candidate 0; masked below
    r[j] = load_stream4(pair_slot<D>(a.IU, a.IL, id, id, l));
  }

  // ---- scores (both terms in one reduction) -> strip
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const float pj = row_allreduce_sum<LPR>(dot4(q4, r[j]));
    if (l == 0) strip[grp * CPL + j] = pj;
  }
  wave_lds_sync();

  // ---- loss, one lane per candidate (slot s = grp * CPL + j  <->  candidate c = j * GS + grp)
  float pc[NPL];
  int cc[NPL];
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int s = sub + k * S;
    const int c = (s % CPL) * GS + s / CPL;
    cc[k] = (s < SLOTS && c < C) ? c : -1;
    pc[k] = s < SLOTS ? strip[s] : 0.f;
  }
  const float pos = strip[0];
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < NPL; ++k)
    if (cc[k] >= 1) mx = fmaxf(mx, pc[k]);
  mx = tuple_allreduce_max<S>(mx);
  float ew[NPL], sg[NPL];
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    ew[k] = cc[k] >= 1 ? expf(pc[k] - mx) : 0.f;
    se += ew[k];
  }
  se = tuple_allreduce_sum<S>(se);
  const float inv_se = 1.0f / se;
  float P = 0.f, A = 0.f;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    ew[k] *= inv_se;
    sg[k] = sigmoidf_(pos - pc[k]);
    P = fmaf(ew[k], sg[k], P);
    A = fmaf(ew[k], sg[k] * (1.0f - sg[k]), A);
  }
  P = tuple_allreduce_sum<S>(P);
  A = tuple_allreduce_sum<S>(A);
  const BprRow br = bpr_row(P, a.inv_b);
  if (tv && sub == 0) a.loss_vec[t] = br.loss;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int s = sub + k * S;
    float g = br.dLdP * bpr_dP_dneg(ew[k], sg[k], P);
    if (cc[k] == 0) g = br.dLdP * A;
    if (cc[k] < 0) g = 0.f;
    if (s < SLOTS) strip[s] = g;
    if (tv && cc[k] >= 0) {
      a.gpred[t * C + cc[k]] = g;
      if (a.pred != nullptr) a.pred[t * C + cc[k]] = pc[k];
    }
  }
  wave_lds_sync();

  // ---- backward: lower lanes sum g_c * IU[i_c] (ugrad), upper lanes g_c * IL[i_c] (lgrad)
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int j = 0; j < CPL; ++j) fma4(acc, strip[grp * CPL + j], r[j]);   // broadcast read, 0 on slots past C
  acc.x = groups_allreduce_sum<LPR, S>(acc.x);
  acc.y = groups_allreduce_sum<LPR, S>(acc.y);
  acc.z = groups_allreduce_sum<LPR, S>(acc.z);
  acc.w = groups_allreduce_sum<LPR, S>(acc.w);
  if (tv && grp == 0) {
    const bool up = l >= H;
    reinterpret_cast<float4*>((up ? a.lgrad : a.ugrad) + t * D)[up ? l - H : l] = acc;
  }
}

// ---- fused forward / loss / backward, streaming path: any C >= 2 -----------------------------------------------------------------
constexpr int kStreamU = 4;   // candidate pair rows in flight per lane-group

template <int D>
__global__ __launch_bounds__(kBlock) void fpmc_fwd_bwd_stream_kernel(FpmcArgs a) {
  constexpr int H = D / 4, LPR = D / 2, G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (t >= a.B) return;   // wave-uniform; no workgroup barrier in this kernel
  const int grp = lane / LPR, l = lane % LPR;
  const int C = a.C;
  const float4 q4 = *pair_slot<D>(a.UI, a.LI, a.uid[t], a.lid[t], l);
  const int64_t* ids = a.iid + t * C;
  float* stage = a.gpred + t * C;   // scores first, the gradient scalars afterwards

  for (int c0 = 0; c0 < C; c0 += kStreamU * G) {
    float4 r[kStreamU];
#pragma unroll
    for (int u = 0; u < kStreamU; ++u) {
      const int c = c0 + u * G + grp;
      const int64_t id = ids[c < C ? c : 0];
      r[u] = *pair_slot<D>(a.IU, a.IL, id, id, l);   // (plain loads: the rows are read again below)
    }
#pragma unroll
    for (int u = 0; u < kStreamU; ++u) {
      const int c = c0 + u * G + grp;
      const float p = row_allreduce_sum<LPR>(dot4(q4, r[u]));
      if (l == 0 && c < C) stage[c] = p;
    }
  }
  __threadfence();   // the wave's own stores, read back by its other lanes
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
    if (a.pred != nullptr) a.pred[t * C + c] = pc;
    stage[c] = g;
  }
  __threadfence();
  __builtin_amdgcn_wave_barrier();

  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c0 = 0; c0 < C; c0 += kStreamU * G) {
    float4 r[kStreamU];
    float g[kStreamU];
#pragma unroll
    for (int u = 0; u < kStreamU; ++u) {
      const int c = c0 + u * G + grp;
      const int64_t id = ids[c < C ? c : 0];
      r[u] = *pair_slot<D>(a.IU, a.IL, id, id, l);
      g[u] = c < C ? stage[c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kStreamU; ++u) fma4(acc, g[u], r[u]);
  }
  acc.x = groups_allreduce_sum<LPR, 64>(acc.x);
  acc.y = groups_allreduce_sum<LPR, 64>(acc.y);
  acc.z = groups_allreduce_sum<LPR, 64>(acc.z);
  acc.w = groups_allreduce_sum<LPR, 64>(acc.w);
  if (grp == 0) {
    const bool up = l >= H;
    reinterpret_cast<float4*>((up ? a.lgrad : a.ugrad) + t * D)[up ? l - H : l] = acc;
  }
}

// ---- item-side update: both candidate tables in one pass over the sorted candidate ids ----------------------------------------------
// One pair lane-group (LPR = d / 2 lanes) per listed head: the lower lanes sum gpred[o] * UI[uid[o / C]] for table IU, the upper
// lanes gpred[o] * LI[lid[o / C]] for table IL, over the segment's occurrences in ascending sorted position; then each half applies
// the optimizer to (or writes the dense gradient of) its table's row.  Rows with more than kFpmcLongSeg occurrences are listed
// (integer atomic: the list order decides which workgroup takes which row, no sum) and taken by one workgroup each, whose lane-groups
// stride over the segment in a fixed pattern and combine in a fixed LDS tree.
struct FpmcUpd {
  float* W[2];       // IU, IL
  float* M[2];
  float* V[2];
  float* dense[2];
  const float* Q[2];         // UI, LI
  const int64_t* qid[2];     // uid, lid
  const uint32_t* keys;
  const uint32_t* perm;
  int64_t n_occ;
  const float* gpred;
  int C;
  const uint32_t* heads;
  const uint32_t* n_heads;
  uint32_t* n_long;
  uint32_t* long_list;
  uint32_t long_cap;
  OptScalars o;
};

template <int D>
__device__ __forceinline__ float4 fpmc_occ_grad4_o(const FpmcUpd& a, uint32_t o, int up, int ll) {
  const float g = a.gpred[o];
  const int64_t row = a.qid[up][o / (uint32_t)a.C];
  float4 s = reinterpret_cast<const float4*>(a.Q[up] + row * D)[ll];
  s.x *= g; s.y *= g; s.z *= g; s.w *= g;
  return s;
}
template <int D>
__device__ __forceinline__ float4 fpmc_occ_grad4(const FpmcUpd& a, int64_t jj, int up, int ll) {
  return fpmc_occ_grad4_o<D>(a, a.perm[jj], up, ll);
}

// the table row of `key` this lane owns, requested before the gradient chain starts (read-once: non-temporal)
template <int D, int MODE>
__device__ __forceinline__ float4 fpmc_load_row4(const FpmcUpd& a, uint32_t key, int up, int ll) {
  if (MODE == MODE_DENSE_GRAD) return make_float4(0.f, 0.f, 0.f, 0.f);
  return load_stream4(reinterpret_cast<const float4*>(a.W[up]) + (size_t)key * (D / 4) + ll);
}

template <int D, int MODE>
__device__ __forceinline__ void fpmc_apply_row4(const FpmcUpd& a, uint32_t key, int up, int ll, const float4& w, const float4& g) {
  const size_t idx = (size_t)key * (D / 4) + ll;
  if (MODE == MODE_DENSE_GRAD) {
    reinterpret_cast<float4*>(a.dense[up])[idx] = g;
    return;
  }
  opt_row4<MODE>(a.o, a.W[up], a.M[up], a.V[up], idx, w, g);
}

__device__ __forceinline__ void add4_(float4& x, const float4& y) {
  x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
}

// Dependent-load depth: heads[g] -> {keys[j], keys[j + 1], perm[j], perm[j + 1]} -> {table row, gpred, query id} -> {query row} -> store.
// The kernel is bound by that chain, not by bandwidth, so a lane-group takes kFpmcHpg independent heads and requests every level of
// both chains together (the table rows and the first two occurrences of each: most rows of a large catalogue occur once or twice).
// A row's sum keeps ascending sorted position whatever the interleaving.
constexpr int kFpmcHpg = 2;

template <int D, int MODE>
__global__ __launch_bounds__(kBlock) void fpmc_item_update_kernel(FpmcUpd a) {
  constexpr int H = D / 4, LPR = D / 2, GPB = kBlock / LPR, HPG = kFpmcHpg;
  const int l = threadIdx.x % LPR;
  const int up = l >= H ? 1 : 0, ll = up ? l - H : l;
  const int64_t n = a.n_occ;
  const int64_t nh = (int64_t)*a.n_heads;
  const int64_t g = ((int64_t)blockIdx.x * GPB + threadIdx.x / LPR) * HPG;
  if (g >= nh) return;   // no cross-lane operation in this kernel
  int64_t j[HPG];
  uint32_t key[HPG], o0[HPG], o1[HPG];
  bool multi[HPG], hot[HPG];
  float4 w[HPG], acc[HPG], s1[HPG];
#pragma unroll
  for (int h = 0; h < HPG; ++h) j[h] = a.heads[g + h < nh ? g + h : g];
#pragma unroll
  for (int h = 0; h < HPG; ++h) {
    const bool has_next = j[h] + 1 < n;
    key[h] = a.keys[j[h]];
    multi[h] = has_next && a.keys[j[h] + 1] == key[h];
    o0[h] = a.perm[j[h]];
    o1[h] = a.perm[has_next ? j[h] + 1 : j[h]];
    hot[h] = j[h] + kFpmcLongSeg < n && a.keys[j[h] + kFpmcLongSeg] == key[h];   // keys are sorted: one probe decides
  }
#pragma unroll
  for (int h = 0; h < HPG; ++h) w[h] = fpmc_load_row4<D, MODE>(a, key[h], up, ll);
#pragma unroll
  for (int h = 0; h < HPG; ++h) acc[h] = fpmc_occ_grad4_o<D>(a, o0[h], up, ll);
#pragma unroll
  for (int h = 0; h < HPG; ++h) s1[h] = fpmc_occ_grad4_o<D>(a, o1[h], up, ll);   // (a single occurrence: the next segment's first row, requested but not added)
#pragma unroll
  for (int h = 0; h < HPG; ++h) {
    if (g + h >= nh) break;
    if (hot[h]) {   // more than kFpmcLongSeg occurrences: left to fpmc_item_update_long_kernel untouched
      if (l == 0) {
        const uint32_t slot = atomicAdd(a.n_long, 1u);
        if (slot < a.long_cap) a.long_list[slot] = (uint32_t)j[h];
      }
      continue;
    }
    if (multi[h]) {
      add4_(acc[h], s1[h]);
      for (int64_t jj = j[h] + 2; jj < n && a.keys[jj] == key[h]; ++jj) add4_(acc[h], fpmc_occ_grad4<D>(a, jj, up, ll));
    }
    fpmc_apply_row4<D, MODE>(a, key[h], up, ll, w[h], acc[h]);
  }
}

template <int D, int MODE>
__global__ __launch_bounds__(kBlock) void fpmc_item_update_long_kernel(FpmcUpd a) {
  constexpr int H = D / 4, LPR = D / 2, GPB = kBlock / LPR;
  __shared__ float4 part[kBlock];
  const int l = threadIdx.x % LPR, g = threadIdx.x / LPR;
  const int up = l >= H ? 1 : 0, ll = up ? l - H : l;
  const int64_t n = a.n_occ;
  uint32_t n_long = *a.n_long;
  if (n_long > a.long_cap) n_long = a.long_cap;
  for (uint32_t i = blockIdx.x; i < n_long; i += gridDim.x) {   // workgroup-uniform
    const int64_t j0 = a.long_list[i];
    const uint32_t key = a.keys[j0];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    // lane-group g takes positions j0 + g, j0 + g + GPB, ...: two in flight per trip, added in position order
    for (int64_t jj = j0 + g; jj < n && a.keys[jj] == key; jj += 2 * GPB) {
      const float4 s0 = fpmc_occ_grad4<D>(a, jj, up, ll);
      const bool more = jj + GPB < n && a.keys[jj + GPB] == key;
      const float4 s1 = more ? fpmc_occ_grad4<D>(a, jj + GPB, up, ll) : make_float4(0.f, 0.f, 0.f, 0.f);
      add4_(acc, s0);
      add4_(acc, s1);
    }
    part[threadIdx.x] = acc;
#pragma unroll
    for (int off = GPB / 2; off >= 1; off >>= 1) {
      __syncthreads();
      if (g < off) {
        float4 x = part[threadIdx.x];
        add4_(x, part[threadIdx.x + off * LPR]);
        part[threadIdx.x] = x;
      }
    }
    __syncthreads();
    if (g == 0) fpmc_apply_row4<D, MODE>(a, key, up, ll, fpmc_load_row4<D, MODE>(a, key, up, ll), part[threadIdx.x]);
    __syncthreads();   // part[] is reused by the next row
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static bool fpmc_width_ok(int d) { return d == 16 || d == 32 || d == 64 || d == 128; }
// d = 16: eight lane-groups make the loss phase's per-lane arrays seven long, and 50 rows beside them spill (20 bytes of scratch)
constexpr int fpmc_max_cpl(int d) { return d == 16 ? 33 : kFpmcMaxCpl; }

// the register layout of (d, C): GS lane-groups per tuple with CPL pair rows each; false: the streaming path
static bool fpmc_pick(int d, int C, int* gs, int* cpl) {
  static const int buckets[] = {1, 2, 3, 4, 6, 8, 13, 17, 25, 33, kFpmcMaxCpl};
  if (!fpmc_width_ok(d) || C < 2) return false;
  const int G = 128 / d;
  for (int g = 2; g < G; g <<= 1)   // few candidates: several tuples per wave
    if (C <= g) {
      *gs = g;
      *cpl = 1;
      return true;
    }
  const int need = (C + G - 1) / G;
  for (int b : buckets)
    if (need <= b && b <= fpmc_max_cpl(d)) {
      *gs = G;
      *cpl = b;
      return true;
    }
  return false;
}

template <int D, int GS, int CPL>
static int launch_fpmc_reg(const FpmcArgs& a, hipStream_t s) {
  constexpr int TPB = (64 / ((D / 2) * GS)) * (kBlock / 64);
  const int blocks = (a.B + TPB - 1) / TPB;
  hipLaunchKernelGGL((fpmc_fwd_bwd_kernel<D, GS, CPL>), dim3(blocks), dim3(kBlock), 0, s, a);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

template <int D>
static int dispatch_fpmc_reg(const FpmcArgs& a, int gs, int cpl, hipStream_t s) {
  constexpr int G = 128 / D;
  static const char* who = "rc_fpmc_fwd_bwd";
  if (gs < G)   // (cpl == 1)
    return dispatch_or_fail<2, 4>(who, "lane-groups per tuple", gs, [&](auto GS) -> int {
      if constexpr (GS() < G) return launch_fpmc_reg<D, GS(), 1>(a, s);
      else return fail(RC_ERR_UNSUPPORTED, "%s: no layout", who);
    });
  return dispatch_or_fail<1, 2, 3, 4, 6, 8, 13, 17, 25, 33, kFpmcMaxCpl>(who, "rows per lane-group", cpl, [&](auto CPL) -> int {
    if constexpr (CPL() <= fpmc_max_cpl(D)) return launch_fpmc_reg<D, G, CPL()>(a, s);
    else return fail(RC_ERR_UNSUPPORTED, "%s: no layout", who);
  });
}

static int fpmc_common_check(const char* who, const void* UI, const void* LI, const void* IU, const void* IL, const void* uid,
                             const void* lid, const void* iid, int B, int C, int d, int min_c) {
  RC_REQUIRE(UI && LI && IU && IL && uid && lid && iid, "%s: null pointer", who);
  RC_REQUIRE(fpmc_width_ok(d), "%s: emb_size d=%d has no kernel (16, 32, 64, 128)", who, d);
  RC_REQUIRE(B > 0 && C >= min_c, "%s: need B >= 1 and C >= %d, got B=%d C=%d", who, min_c, B, C);
  RC_REQUIRE(aligned16(UI, LI, IU, IL), "%s: tables must be 16-byte aligned", who);
  return RC_OK;
}

static int fpmc_scores_impl(const float* UI, const float* LI, const float* IU, const float* IL, const int64_t* uid, const int64_t* lid,
                            const int64_t* iid, int B, int C, int d, float* pred, rc_stream_t stream) {
  static const char* who = "rc_fpmc_scores";
  if (B == 0) return RC_OK;
  RC_TRY(fpmc_common_check(who, UI, LI, IU, IL, uid, lid, iid, B, C, d, 1));
  RC_REQUIRE(pred != nullptr, "%s: null pointer", who);
  FpmcArgs a;
  memset(&a, 0, sizeof(a));
  a.UI = UI; a.LI = LI; a.IU = IU; a.IL = IL; a.uid = uid; a.lid = lid; a.iid = iid; a.B = B; a.C = C; a.pred = pred;
  hipStream_t s = as_stream(stream);
  return dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", d, [&](auto D) -> int {
    constexpr int CPB = (kBlock / 64) * (128 / D()) * kScoreU;
    const int64_t chunks = ((int64_t)C + CPB - 1) / CPB;
    const int64_t blocks = chunks * B;
    if (blocks > kMaxGridX) return fail(RC_ERR_UNSUPPORTED, "%s: grid too large (B=%d C=%d)", who, B, C);
    hipLaunchKernelGGL((fpmc_scores_kernel<D()>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a, (int)chunks);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

static int fpmc_fwd_bwd_impl(const float* UI, const float* LI, const float* IU, const float* IL, const int64_t* uid, const int64_t* lid,
                             const int64_t* iid, int B, int C, int d, float inv_b, float* pred, float* loss_vec, float* gpred,
                             float* ugrad, float* lgrad, rc_stream_t stream) {
  static const char* who = "rc_fpmc_fwd_bwd";
  if (B == 0) return RC_OK;
  RC_TRY(fpmc_common_check(who, UI, LI, IU, IL, uid, lid, iid, B, C, d, 2));
  RC_REQUIRE(loss_vec && gpred && ugrad && lgrad, "%s: null pointer", who);
  RC_REQUIRE(aligned16(ugrad, lgrad), "%s: ugrad / lgrad must be 16-byte aligned", who);
  FpmcArgs a;
  memset(&a, 0, sizeof(a));
  a.UI = UI; a.LI = LI; a.IU = IU; a.IL = IL; a.uid = uid; a.lid = lid; a.iid = iid; a.B = B; a.C = C; a.inv_b = inv_b;
  a.pred = pred; a.loss_vec = loss_vec; a.gpred = gpred; a.ugrad = ugrad; a.lgrad = lgrad;
  hipStream_t s = as_stream(stream);
  int gs = 0, cpl = 0;
  const bool reg = fpmc_pick(d, C, &gs, &cpl);
  return dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", d, [&](auto D) -> int {
    if (reg) return dispatch_fpmc_reg<D()>(a, gs, cpl, s);
    const int blocks = (B + (kBlock / 64) - 1) / (kBlock / 64);
    hipLaunchKernelGGL((fpmc_fwd_bwd_stream_kernel<D()>), dim3(blocks), dim3(kBlock), 0, s, a);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

struct FpmcWs {
  uint32_t* n_long;
  uint32_t* long_list;
  uint32_t long_cap;
  size_t total;
};

static FpmcWs carve_fpmc_ws(void* base, int64_t n_occ) {
  Carver cv(base);
  FpmcWs w;
  w.long_cap = (uint32_t)(n_occ / (kFpmcLongSeg + 1)) + 1;   // rows with more than kFpmcLongSeg occurrences
  w.n_long = cv.take<uint32_t>(1);
  w.long_list = cv.take<uint32_t>(w.long_cap);
  w.total = cv.off;
  return w;
}

static int fpmc_item_update_impl(float* IU, float* mIU, float* vIU, float* IL, float* mIL, float* vIL, int d, const uint32_t* keys,
                                 const uint32_t* perm, int64_t n_occ, const float* gpred, const float* UI, const float* LI,
                                 const int64_t* uid, const int64_t* lid, int C, const rc_opt_hyper* h, float* dense_grad_iu,
                                 float* dense_grad_il, const uint32_t* heads, const uint32_t* n_heads, void* ws, size_t ws_bytes,
                                 rc_stream_t stream) {
  static const char* who = "rc_fpmc_item_update";
  if (n_occ == 0) return RC_OK;
  RC_REQUIRE((dense_grad_iu != nullptr) == (dense_grad_il != nullptr), "%s: both dense gradients or none", who);
  const bool dense = dense_grad_iu != nullptr;
  RC_REQUIRE(keys && perm && gpred && UI && LI && uid && lid && ws, "%s: null pointer", who);
  RC_REQUIRE(heads && n_heads, "%s: the head list of rc_segment_heads is required", who);
  RC_REQUIRE(dense || (IU && IL), "%s: no output (IU and IL, or the dense gradients)", who);
  RC_REQUIRE(fpmc_width_ok(d), "%s: emb_size d=%d has no kernel (16, 32, 64, 128)", who, d);
  RC_REQUIRE(C >= 1 && n_occ > 0 && n_occ < ((int64_t)1 << 31), "%s: bad shape C=%d n_occ=%lld", who, C, (long long)n_occ);
  RC_REQUIRE(dense || (UI != IU && UI != IL && LI != IU && LI != IL && IU != IL), "%s: the four tables must be distinct", who);
  FpmcUpd a;
  memset(&a, 0, sizeof(a));
  int mode = MODE_DENSE_GRAD;
  if (!dense) {
    RC_TRY(fill_opt_scalars(who, h, &a.o));
    mode = mode_of(h);
    RC_TRY(opt_state_check(who, mode, mIU != nullptr && mIL != nullptr, vIU != nullptr && vIL != nullptr));
    RC_REQUIRE(aligned16(IU, mIU, vIU, IL, mIL, vIL), "%s: tables must be 16-byte aligned", who);
  } else {
    RC_REQUIRE(aligned16(dense_grad_iu, dense_grad_il), "%s: dense gradients must be 16-byte aligned", who);
  }
  RC_REQUIRE(aligned16(UI, LI), "%s: tables must be 16-byte aligned", who);
  const FpmcWs w = carve_fpmc_ws(ws, n_occ);
  if (ws_bytes < w.total) return fail(RC_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, w.total);
  a.W[0] = IU; a.W[1] = IL; a.M[0] = mIU; a.M[1] = mIL; a.V[0] = vIU; a.V[1] = vIL;
  a.dense[0] = dense_grad_iu; a.dense[1] = dense_grad_il;
  a.Q[0] = UI; a.Q[1] = LI; a.qid[0] = uid; a.qid[1] = lid;
  a.keys = keys; a.perm = perm; a.n_occ = n_occ; a.gpred = gpred; a.C = C; a.heads = heads; a.n_heads = n_heads;
  a.n_long = w.n_long; a.long_list = w.long_list; a.long_cap = w.long_cap;
  hipStream_t s = as_stream(stream);
  RC_HIP(hipMemsetAsync(w.n_long, 0, sizeof(uint32_t), s));
  return dispatch_or_fail<MODE_DENSE_GRAD, MODE_SGD, MODE_ADAM, MODE_ADAGRAD>(who, "update mode", mode, [&](auto M) -> int {
    return dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", d, [&](auto D) -> int {
      constexpr int GPB = kFpmcHpg * (kBlock / (D() / 2));   // heads per workgroup
      const int64_t blocks = (n_occ + GPB - 1) / GPB;       // upper bound on the listed heads: every position
      if (blocks > kMaxGridX) return fail(RC_ERR_UNSUPPORTED, "%s: grid too large", who);
      hipLaunchKernelGGL((fpmc_item_update_kernel<D(), M()>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
      RC_LAUNCH_CHECK();
      if (n_occ > kFpmcLongSeg) {   // otherwise no segment can be long
        const unsigned long_blocks = a.long_cap < 2048u ? a.long_cap : 2048u;
        hipLaunchKernelGGL((fpmc_item_update_long_kernel<D(), M()>), dim3(long_blocks), dim3(kBlock), 0, s, a);
        RC_LAUNCH_CHECK();
      }
      return RC_OK;
    });
  });
}

}  // namespace rc

using namespace rc;

extern "C" enum rc_status rc_fpmc_check_shape(int d, int C) {
  if (!fpmc_width_ok(d))
    return (enum rc_status)fail(RC_ERR_INVALID_ARG, "rc_fpmc_check_shape: emb_size d=%d has no kernel (16, 32, 64, 128)", d);
  if (C < 1) return (enum rc_status)fail(RC_ERR_INVALID_ARG, "rc_fpmc_check_shape: need C >= 1 candidates, got %d", C);
  return RC_OK;
}

extern "C" size_t rc_fpmc_fwd_bwd_layout(int d, int C) {
  int gs = 0, cpl = 0;
  return fpmc_pick(d, C, &gs, &cpl) ? (size_t)(gs * 256 + cpl) : 0;
}

extern "C" enum rc_status rc_fpmc_scores(const float* UI, const float* LI, const float* IU, const float* IL, const int64_t* uid,
                                         const int64_t* lid, const int64_t* iid, int B, int C, int d, float* pred,
                                         rc_stream_t stream) {
  return (enum rc_status)fpmc_scores_impl(UI, LI, IU, IL, uid, lid, iid, B, C, d, pred, stream);
}

extern "C" enum rc_status rc_fpmc_fwd_bwd(const float* UI, const float* LI, const float* IU, const float* IL, const int64_t* uid,
                                          const int64_t* lid, const int64_t* iid, int B, int C, int d, float inv_b, float* pred,
                                          float* loss_vec, float* gpred, float* ugrad, float* lgrad, rc_stream_t stream) {
  return (enum rc_status)fpmc_fwd_bwd_impl(UI, LI, IU, IL, uid, lid, iid, B, C, d, inv_b, pred, loss_vec, gpred, ugrad, lgrad, stream);
}

extern "C" size_t rc_fpmc_item_update_workspace_bytes(int64_t n_occ, int d) {
  (void)d;
  if (n_occ < 1) n_occ = 1;
  return carve_fpmc_ws(nullptr, n_occ).total;
}

extern "C" enum rc_status rc_fpmc_item_update(float* IU, float* mIU, float* vIU, float* IL, float* mIL, float* vIL, int d,
                                              const uint32_t* keys, const uint32_t* perm, int64_t n_occ, const float* gpred,
                                              const float* UI, const float* LI, const int64_t* uid, const int64_t* lid, int C,
                                              const rc_opt_hyper* h, float* dense_grad_iu, float* dense_grad_il, const uint32_t* heads,
                                              const uint32_t* n_heads, void* ws, size_t ws_bytes, rc_stream_t stream) {
  return (enum rc_status)fpmc_item_update_impl(IU, mIU, vIU, IL, mIL, vIL, d, keys, perm, n_occ, gpred, UI, LI, uid, lid, C, h,
                                               dense_grad_iu, dense_grad_il, heads, n_heads, ws, ws_bytes, stream);
}
