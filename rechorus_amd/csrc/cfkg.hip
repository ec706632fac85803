// cfkg.hip -- CFKG (Zhang et al., SIGIR 2018; reference models/general/CFKG.py:57-76): a TransE translation distance on ONE entity
// table E [n_rows, d] (users first, then the other entities) and a relation table R [n_rel, d],
//     pred[b, c] = -|| E[head[b, c]] + R[rel[b, c]] - E[tail[b, c]] ||^2,
// trained with MarginRankingLoss on a fixed quadruple per row: (h, r, t) against (h, r, t') and against (h', r, t).
//
// Lane algebra: LPR = d / 4 consecutive lanes own one translation; each lane holds one float4 of every row involved, so a row is
// one coalesced 4 d-byte segment and the squared distance is one DPP row reduction.  The ids of a lane-group's work are read
// first, then EVERY row load is issued before any of them is consumed (no id -> row -> id chains).
//
//   cfkg_scores_kernel      any [B, C] id triple; a wave whose candidates share one head and one relation (the evaluation feed)
//                           reads E[head] + R[rel] once (a wave-uniform comparison of the ids, no second entry point)
//   cfkg_fwd_bwd_kernel     the training step's front for the quadruple layout: a, b, c formed once, both hinges, the four
//                           gradient rows stored as float4, and the relation gradient summed WITHOUT atomics: each lane keeps NR <= 8
//                           register accumulators of its float4 (selected by r == k, no dynamic indexing), the lane-groups of a wave
//                           combine by a fixed xor butterfly, the four waves through LDS in wave order, and the workgroup writes
//                           one [n_rel, d] partial to the workspace
//   cfkg_relation_reduce_kernel   sums the partials per relation in workgroup order (fixed strides, fixed LDS order) into GR
//   cfkg_scores_bwd_kernel  G[o, :] = -2 gpred[o] (E[head[o]] + R[rel[o]] - E[tail[o]]) for the dense autograd node
// No floating-point atomics; every sum has a fixed order, so results are bit-identical from run to run.
#include "common.hpp"

namespace rc {

constexpr int kCfkgIter = 4;      // rows one lane-group takes in cfkg_fwd_bwd_kernel (fewer, larger relation partials)
constexpr int kCfkgScoreU = 4;    // candidates per lane-group in flight in the score kernels
constexpr int kCfkgMaxRel = 8;

struct CfkgScoreArgs {
  const float* E;
  const float* R;
  const int64_t* head;
  const int64_t* tail;
  const int64_t* rel;
  int B, C;
  float* pred;
  const float* gpred;   // scores_bwd only
  float* G;             // scores_bwd only
};

struct CfkgStepArgs {
  const float* E;
  const float* R;
  const int64_t* h;
  const int64_t* t;
  const int64_t* hn;
  const int64_t* tn;
  const int64_t* r;
  int B, n_rel;
  float margin, inv_b;
  float* loss_vec;
  float* pred;
  float* grows;
  float* partial;   // [blocks, n_rel, d]
};

template <int D>
__device__ __forceinline__ float4 row4(const float* W, int64_t row, int l) {
  return reinterpret_cast<const float4*>(W + row * D)[l];
}

__device__ __forceinline__ float4 add4(const float4& x, const float4& y) { return make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w); }
__device__ __forceinline__ float4 sub4(const float4& x, const float4& y) { return make_float4(x.x - y.x, x.y - y.y, x.z - y.z, x.w - y.w); }
__device__ __forceinline__ float4 scale4(float s, const float4& x) { return make_float4(s * x.x, s * x.y, s * x.z, s * x.w); }

// ---- scores ---------------------------------------------------------------------------------------------------------------------
// A workgroup takes one row b and CPB = 4 waves * G lane-groups * kCfkgScoreU candidates of it.
template <int D>
__global__ __launch_bounds__(kBlock) void cfkg_scores_kernel(CfkgScoreArgs a, int chunks) {
  constexpr int LPR = D / 4, G = 64 / LPR;
  constexpr int CPB = (kBlock / 64) * G * kCfkgScoreU;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane / LPR, l = lane % LPR;
  const int64_t b = blockIdx.x / chunks;
  const int c0 = (int)(blockIdx.x % chunks) * CPB + wave * (G * kCfkgScoreU);
  if (c0 >= a.C) return;   // wave-uniform; no workgroup barrier in this kernel
  const int64_t base = b * a.C;
  int64_t hd[kCfkgScoreU], tl[kCfkgScoreU], rl[kCfkgScoreU];
#pragma unroll
  for (int u = 0; u < kCfkgScoreU; ++u) {
    const int c = c0 + u * G + grp;
    const int64_t o = base + (c < a.C ? c : c0);   // slots past C re-read the wave's first candidate; masked at the store
    hd[u] = a.head[o];
    tl[u] = a.tail[o];
    rl[u] = a.rel[o];
  }
  const int64_t h0 = a.head[base + c0], r0 = a.rel[base + c0];
  bool same = true;
#pragma unroll
  for (int u = 0; u < kCfkgScoreU; ++u) same = same && hd[u] == h0 && rl[u] == r0;
  float4 v[kCfkgScoreU];
  if (__all(same)) {   // the evaluation feed: one head and one relation for the whole wave
    const float4 hq = row4<D>(a.E, h0, l), rq = row4<D>(a.R, r0, l);
    float4 tv[kCfkgScoreU];
#pragma unroll
    for (int u = 0; u < kCfkgScoreU; ++u) tv[u] = load_stream4(reinterpret_cast<const float4*>(a.E + tl[u] * D) + l);
    const float4 q = add4(hq, rq);
#pragma unroll
    for (int u = 0; u < kCfkgScoreU; ++u) v[u] = sub4(q, tv[u]);
  } else {
    float4 hv[kCfkgScoreU], rv[kCfkgScoreU], tv[kCfkgScoreU];
#pragma unroll
    for (int u = 0; u < kCfkgScoreU; ++u) {
      hv[u] = row4<D>(a.E, hd[u], l);
      tv[u] = row4<D>(a.E, tl[u], l);
      rv[u] = row4<D>(a.R, rl[u], l);
    }
#pragma unroll
    for (int u = 0; u < kCfkgScoreU; ++u) v[u] = sub4(add4(hv[u], rv[u]), tv[u]);
  }
#pragma unroll
  for (int u = 0; u < kCfkgScoreU; ++u) {
    const int c = c0 + u * G + grp;
    const float s = row_allreduce_sum<LPR>(dot4(v[u], v[u]));
    if (l == 0 && c < a.C) a.pred[base + c] = -s;
  }
}

// ---- the dense node's backward: one gradient row per (b, c) --------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kBlock) void cfkg_scores_bwd_kernel(CfkgScoreArgs a, int64_t n) {
  constexpr int LPR = D / 4, GPB = kBlock / LPR;
  const int l = threadIdx.x % LPR;
  const int64_t o0 = ((int64_t)blockIdx.x * GPB + threadIdx.x / LPR) * kCfkgScoreU;
  if (o0 >= n) return;   // no cross-lane operation in this kernel
  int64_t hd[kCfkgScoreU], tl[kCfkgScoreU], rl[kCfkgScoreU];
  float g[kCfkgScoreU];
#pragma unroll
  for (int u = 0; u < kCfkgScoreU; ++u) {
    const int64_t o = o0 + u < n ? o0 + u : o0;
    hd[u] = a.head[o];
    tl[u] = a.tail[o];
    rl[u] = a.rel[o];
    g[u] = a.gpred[o];
  }
  float4 hv[kCfkgScoreU], rv[kCfkgScoreU], tv[kCfkgScoreU];
#pragma unroll
  for (int u = 0; u < kCfkgScoreU; ++u) {
    hv[u] = row4<D>(a.E, hd[u], l);
    tv[u] = row4<D>(a.E, tl[u], l);
    rv[u] = row4<D>(a.R, rl[u], l);
  }
#pragma unroll
  for (int u = 0; u < kCfkgScoreU; ++u) {
    if (o0 + u >= n) break;
    reinterpret_cast<float4*>(a.G + (o0 + u) * D)[l] = scale4(-2.0f * g[u], sub4(add4(hv[u], rv[u]), tv[u]));
  }
}

// ---- fused forward / hinge loss / backward for the quadruple layout -------------------------------------------------------------------
// Workgroup `blk` takes rows [blk * RPB, (blk + 1) * RPB), RPB = kCfkgIter * GPB; lane-group g takes row blk * RPB + it * GPB + g
// in trip `it`.  Rows past B are clamped for the loads and masked out of every store and sum, so all lanes stay in the shuffles.
template <int D, int NR>
__global__ __launch_bounds__(kBlock) void cfkg_fwd_bwd_kernel(CfkgStepArgs a) {
  constexpr int LPR = D / 4, GPB = kBlock / LPR, NW = kBlock / 64;
  __shared__ float4 part[NW * NR * LPR];
  const int l = threadIdx.x % LPR, g = threadIdx.x / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 racc[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) racc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t row0 = (int64_t)blockIdx.x * (kCfkgIter * GPB);

  for (int it = 0; it < kCfkgIter; ++it) {
    const int64_t raw = row0 + (int64_t)it * GPB + g;
    const bool live = raw < a.B;
    const int64_t b = live ? raw : (int64_t)a.B - 1;
    // ids first, then all five rows in flight
    const int64_t ih = a.h[b], it_ = a.t[b], ihn = a.hn[b], itn = a.tn[b], ir = a.r[b];
    const float4 vh = load_stream4(reinterpret_cast<const float4*>(a.E + ih * D) + l);
    const float4 vt = load_stream4(reinterpret_cast<const float4*>(a.E + it_ * D) + l);
    const float4 vhn = load_stream4(reinterpret_cast<const float4*>(a.E + ihn * D) + l);
    const float4 vtn = load_stream4(reinterpret_cast<const float4*>(a.E + itn * D) + l);
    const float4 vr = row4<D>(a.R, ir, l);

    const float4 hr = add4(vh, vr);
    const float4 va = sub4(hr, vt);                  // a = h + r - t   (the expression of cfkg_scores_kernel, bit for bit)
    const float4 vb = sub4(hr, vtn);                 // b = h + r - t'
    const float4 vc = sub4(add4(vhn, vr), vt);       // c = h' + r - t
    const float na = row_allreduce_sum<LPR>(dot4(va, va));
    const float nb = row_allreduce_sum<LPR>(dot4(vb, vb));
    const float nc = row_allreduce_sum<LPR>(dot4(vc, vc));
    // MarginRankingLoss: max(0, -(pos - neg) + margin), pos = -na; the backward of clamp_min(0) passes at a tie (x >= 0)
    const float x1 = (na - nb) + a.margin, x2 = (na - nc) + a.margin;
    const float s1 = (live && x1 >= 0.f) ? 1.f : 0.f, s2 = (live && x2 >= 0.f) ? 1.f : 0.f;
    if (live && l == 0) {
      a.loss_vec[b] = 0.5f * (s1 * x1 + s2 * x2);
      if (a.pred != nullptr) reinterpret_cast<float4*>(a.pred)[b] = make_float4(-na, -na, -nb, -nc);
    }
    const float w = a.inv_b;
    const float4 ga = scale4(w * (s1 + s2), va);     // w (s1 + s2) a
    const float4 gb = scale4(w * s1, vb);            // w s1 b   = g_t'
    const float4 gc = scale4(w * s2, vc);            // w s2 c   = -g_h'
    const float4 gh = sub4(ga, gb);
    if (live) {
      float4* out = reinterpret_cast<float4*>(a.grows + b * (4 * D)) + l;
      out[0 * LPR] = gh;
      out[1 * LPR] = sub4(gc, ga);
      out[2 * LPR] = make_float4(-gc.x, -gc.y, -gc.z, -gc.w);
      out[3 * LPR] = gb;
    }
    const float4 gr = sub4(gh, gc);                  // exactly 0 on a masked row (s1 = s2 = 0, finite rows)
    const int rk = live ? (int)ir : -1;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const bool hit = rk == k;
      racc[k].x += hit ? gr.x : 0.f;
      racc[k].y += hit ? gr.y : 0.f;
      racc[k].z += hit ? gr.z : 0.f;
      racc[k].w += hit ? gr.w : 0.f;
    }
  }

  // lane-groups of a wave: xor butterfly (a fixed tree); waves: LDS, added in wave order
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    racc[k].x = groups_allreduce_sum<LPR, 64>(racc[k].x);
    racc[k].y = groups_allreduce_sum<LPR, 64>(racc[k].y);
    racc[k].z = groups_allreduce_sum<LPR, 64>(racc[k].z);
    racc[k].w = groups_allreduce_sum<LPR, 64>(racc[k].w);
    if (lane < LPR) part[(wave * NR + k) * LPR + l] = racc[k];
  }
  __syncthreads();
  if ((int)threadIdx.x < a.n_rel * LPR) {   // thread j = k * LPR + l
    float4 s = part[threadIdx.x];
#pragma unroll
    for (int wv = 1; wv < NW; ++wv) s = add4(s, part[wv * NR * LPR + threadIdx.x]);
    reinterpret_cast<float4*>(a.partial + (int64_t)blockIdx.x * a.n_rel * D)[threadIdx.x] = s;
  }
}

// One workgroup per relation k: lane-group g sums the partials of workgroups g, g + GPB, ... in that order (four loads in flight),
// then lane-group 0's lanes add the GPB sums in group order.
template <int D>
__global__ __launch_bounds__(kBlock) void cfkg_relation_reduce_kernel(const float* partial, int n_blocks, int n_rel, float* GR) {
  constexpr int LPR = D / 4, GPB = kBlock / LPR;
  __shared__ float4 part[kBlock];
  const int l = threadIdx.x % LPR, g = threadIdx.x / LPR;
  const int k = blockIdx.x;
  const float4* p = reinterpret_cast<const float4*>(partial) + (int64_t)k * LPR + l;
  const int64_t stride = (int64_t)n_rel * LPR;
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
      if (i0 + q * GPB < n_blocks) acc = add4(acc, v[q]);
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  if (g == 0) {
    float4 s = part[l];
    for (int q = 1; q < GPB; ++q) s = add4(s, part[q * LPR + l]);
    reinterpret_cast<float4*>(GR + (int64_t)k * D)[l] = s;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static bool cfkg_width_ok(int d) { return d == 16 || d == 32 || d == 64 || d == 128; }
static int cfkg_rows_per_block(int d) { return kCfkgIter * (kBlock / (d / 4)); }

static int cfkg_shape_check(const char* who, int d, int C, int n_rel) {
  RC_REQUIRE(cfkg_width_ok(d), "%s: emb_size d=%d has no kernel (16, 32, 64, 128)", who, d);
  RC_REQUIRE(C >= 1, "%s: need C >= 1 candidates, got %d", who, C);
  RC_REQUIRE(n_rel >= 1 && n_rel <= kCfkgMaxRel, "%s: n_rel=%d outside 1..8 relations", who, n_rel);
  return RC_OK;
}

static int cfkg_score_args(const char* who, CfkgScoreArgs* a, const float* E, const float* R, const int64_t* head, const int64_t* tail,
                           const int64_t* rel, int B, int C, int d, int64_t n_rows, int n_rel) {
  RC_REQUIRE(E && R && head && tail && rel, "%s: null pointer", who);
  RC_TRY(cfkg_shape_check(who, d, C, n_rel));
  RC_REQUIRE(B > 0 && n_rows > 0, "%s: need B >= 1 and n_rows >= 1, got B=%d n_rows=%lld", who, B, (long long)n_rows);
  RC_REQUIRE(aligned16(E, R), "%s: tables must be 16-byte aligned", who);
  memset(a, 0, sizeof(*a));
  a->E = E; a->R = R; a->head = head; a->tail = tail; a->rel = rel; a->B = B; a->C = C;
  return RC_OK;
}

static int cfkg_scores_impl(const float* E, const float* R, const int64_t* head, const int64_t* tail, const int64_t* rel, int B, int C,
                            int d, int64_t n_rows, int n_rel, float* pred, rc_stream_t stream) {
  static const char* who = "rc_cfkg_scores";
  if (B == 0) return RC_OK;
  CfkgScoreArgs a;
  RC_TRY(cfkg_score_args(who, &a, E, R, head, tail, rel, B, C, d, n_rows, n_rel));
  RC_REQUIRE(pred != nullptr, "%s: null pointer", who);
  a.pred = pred;
  hipStream_t s = as_stream(stream);
  return dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", d, [&](auto D) -> int {
    constexpr int CPB = (kBlock / 64) * (256 / D()) * kCfkgScoreU;
    const int64_t chunks = ((int64_t)C + CPB - 1) / CPB;
    const int64_t blocks = chunks * B;
    if (blocks > kMaxGridX) return fail(RC_ERR_UNSUPPORTED, "%s: grid too large (B=%d C=%d)", who, B, C);
    hipLaunchKernelGGL((cfkg_scores_kernel<D()>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a, (int)chunks);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

static int cfkg_scores_bwd_impl(const float* E, const float* R, const int64_t* head, const int64_t* tail, const int64_t* rel,
                                const float* gpred, int B, int C, int d, int64_t n_rows, int n_rel, float* G, rc_stream_t stream) {
  static const char* who = "rc_cfkg_scores_bwd";
  if (B == 0) return RC_OK;
  CfkgScoreArgs a;
  RC_TRY(cfkg_score_args(who, &a, E, R, head, tail, rel, B, C, d, n_rows, n_rel));
  RC_REQUIRE(gpred && G, "%s: null pointer", who);
  RC_REQUIRE(aligned16(G), "%s: G must be 16-byte aligned", who);
  a.gpred = gpred;
  a.G = G;
  const int64_t n = (int64_t)B * C;
  hipStream_t s = as_stream(stream);
  return dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", d, [&](auto D) -> int {
    constexpr int OPB = (kBlock / (D() / 4)) * kCfkgScoreU;
    const int64_t blocks = (n + OPB - 1) / OPB;
    if (blocks > kMaxGridX) return fail(RC_ERR_UNSUPPORTED, "%s: grid too large (B=%d C=%d)", who, B, C);
    hipLaunchKernelGGL((cfkg_scores_bwd_kernel<D()>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a, n);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

static size_t cfkg_ws_bytes(int64_t B, int d, int n_rel) {
  if (!cfkg_width_ok(d) || n_rel < 1 || n_rel > kCfkgMaxRel) return 0;
  if (B < 1) B = 1;
  const int rpb = cfkg_rows_per_block(d);
  const int64_t blocks = (B + rpb - 1) / rpb;
  return align_up((size_t)blocks * n_rel * d * sizeof(float), 256);
}

static int cfkg_fwd_bwd_impl(const float* E, const float* R, const int64_t* h, const int64_t* t, const int64_t* hn, const int64_t* tn,
                             const int64_t* r, int B, int d, int64_t n_rows, int n_rel, float margin, float inv_b, float* loss_vec,
                             float* pred, float* grows, float* GR, void* ws, size_t ws_bytes, rc_stream_t stream) {
  static const char* who = "rc_cfkg_fwd_bwd";
  if (B == 0) return RC_OK;
  RC_REQUIRE(E && R && h && t && hn && tn && r && loss_vec && grows && GR && ws, "%s: null pointer", who);
  RC_TRY(cfkg_shape_check(who, d, 4, n_rel));
  RC_REQUIRE(B > 0 && n_rows > 0, "%s: need B >= 1 and n_rows >= 1, got B=%d n_rows=%lld", who, B, (long long)n_rows);
  RC_REQUIRE(aligned16(E, R, grows, GR, pred, ws), "%s: tables, pred, grows, GR and the workspace must be 16-byte aligned", who);
  const size_t need = cfkg_ws_bytes(B, d, n_rel);
  if (ws_bytes < need) return fail(RC_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, need);
  CfkgStepArgs a;
  memset(&a, 0, sizeof(a));
  a.E = E; a.R = R; a.h = h; a.t = t; a.hn = hn; a.tn = tn; a.r = r; a.B = B; a.n_rel = n_rel; a.margin = margin; a.inv_b = inv_b;
  a.loss_vec = loss_vec; a.pred = pred; a.grows = grows; a.partial = reinterpret_cast<float*>(ws);
  const int rpb = cfkg_rows_per_block(d);
  const int blocks = (B + rpb - 1) / rpb;
  const int nr = n_rel <= 1 ? 1 : (n_rel <= 2 ? 2 : (n_rel <= 4 ? 4 : 8));   // register accumulators per lane
  hipStream_t s = as_stream(stream);
  return dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", d, [&](auto D) -> int {
    RC_TRY((dispatch_or_fail<1, 2, 4, 8>(who, "relation accumulators", nr, [&](auto NR) -> int {
      hipLaunchKernelGGL((cfkg_fwd_bwd_kernel<D(), NR()>), dim3(blocks), dim3(kBlock), 0, s, a);
      RC_LAUNCH_CHECK();
      return RC_OK;
    })));
    hipLaunchKernelGGL((cfkg_relation_reduce_kernel<D()>), dim3(n_rel), dim3(kBlock), 0, s, a.partial, blocks, n_rel, GR);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

}  // namespace rc

using namespace rc;

extern "C" enum rc_status rc_cfkg_check_shape(int d, int C, int n_rel) {
  return (enum rc_status)cfkg_shape_check("rc_cfkg_check_shape", d, C, n_rel);
}

extern "C" size_t rc_cfkg_fwd_bwd_rows_per_block(int d) { return cfkg_width_ok(d) ? (size_t)cfkg_rows_per_block(d) : 0; }

extern "C" enum rc_status rc_cfkg_scores(const float* E, const float* R, const int64_t* head, const int64_t* tail, const int64_t* rel,
                                         int B, int C, int d, int64_t n_rows, int n_rel, float* pred, rc_stream_t stream) {
  return (enum rc_status)cfkg_scores_impl(E, R, head, tail, rel, B, C, d, n_rows, n_rel, pred, stream);
}

extern "C" enum rc_status rc_cfkg_scores_bwd(const float* E, const float* R, const int64_t* head, const int64_t* tail,
                                             const int64_t* rel, const float* gpred, int B, int C, int d, int64_t n_rows, int n_rel,
                                             float* G, rc_stream_t stream) {
  return (enum rc_status)cfkg_scores_bwd_impl(E, R, head, tail, rel, gpred, B, C, d, n_rows, n_rel, G, stream);
}

extern "C" size_t rc_cfkg_fwd_bwd_workspace_bytes(int64_t B, int d, int n_rel) { return cfkg_ws_bytes(B, d, n_rel); }

extern "C" enum rc_status rc_cfkg_fwd_bwd(const float* E, const float* R, const int64_t* h, const int64_t* t, const int64_t* hn,
                                          const int64_t* tn, const int64_t* r, int B, int d, int64_t n_rows, int n_rel, float margin,
                                          float inv_b, float* loss_vec, float* pred, float* grows, float* GR, void* ws,
                                          size_t ws_bytes, rc_stream_t stream) {
  return (enum rc_status)cfkg_fwd_bwd_impl(E, R, h, t, hn, tn, r, B, d, n_rows, n_rel, margin, inv_b, loss_vec, pred, grows, GR, ws,
                                           ws_bytes, stream);
}
