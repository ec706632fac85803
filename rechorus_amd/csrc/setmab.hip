// setmab.hip -- one post-norm multihead attention block (MAB) whose query rows are not its key rows (reference:
// models/reranker/SetRank.py:29-56 `MAB`, used twice per induced block, :67-80 `IMSAB`: h = MAB1(I, x, x; pad), x' = MAB2(x, h, h))
//
//   Qs [B, nq, d] list-major, or ONE shared [nq, d] (the learned inducing points I), Ks [B, nk, d], pad uint8 [B, nk] or null
//   q = Qs Wq^T + bq,  k = Ks Wk^T + bk,  v = Ks Wv^T + bv  (Win [3d, d] = Wq | Wk | Wv),
//   P_h = softmax_j(q_h . k_h / sqrt(dk)) over the keys j < nk with pad == 0,
//   A = concat_h(P_h V_h) Wo^T + bo,  X1 = LN1(Qs + A),  Y = LN2(X1 + relu(X1 W1^T + b1) W2^T + b2)          Y [B, nq, d]
//
// The layout is listenc.hip's (its device helpers are listenc_dev.hpp) with two row sets: a workgroup of four waves owns one list at a
// time and walks the batch with the grid as its stride; the query-side rows padded to NQP = 16 QT and the key-side rows padded to
// NKP = 16 KT (QT, KT = 1..4) and every intermediate live in LDS; all products run on v_mfma_f32_16x16x4_f32 with the weights as the
// B operand straight from global memory.
//   attn    a job is (head, 16-row query tile): scores against all NKP keys into the wave's own [16][NKP + 4] scratch, a
//           4-lanes-per-row softmax, then P V.  Keys past nk and keys with pad == 1 get -inf.
//   shared  forward: the workgroup projects q = I Wq^T + bq ONCE, before its first list, into an LDS buffer nothing else writes (the
//           heads' outputs have a buffer of their own), and re-reads only the [nq, d] residual rows per list.  backward: I is loaded
//           once; q is recomputed per list, because its LDS is the feed-forward's in between (as q | k | v is in listenc.hip).  dQs of a
//           shared source is a sum over all lists: the workgroup adds its lists' shares into its partial (plain loads and stores, the
//           first list stores without loading) and the fixed-order reduce adds the partials.
//   bwd     listenc.hip's phases on the query-side rows (recompute, LN2 / FFN / LN1 / out-projection backward), then q, k | v again,
//           the attention backward (a wave owns a head and walks the query tiles: dV, dS, the softmax backward in place over P, dQ over
//           the head's dA columns, dK), then dWq = dQ^T Qs, dWk | dWv = [dK | dV]^T Ks, dQs = d(Qs + A) + dQ Wq, dKs = [dK | dV] Wkv.
//   wgrad   as listenc.hip: at d = 64, d_ff = 128 the 128 weight-gradient tiles stay in registers across the lists a workgroup walks.
//   reduce  listenc's reduce kernel over the twelve gradients, plus one thread per element of a shared dQs; workgroup order, in double.
// The number of workgroups (= partials) is min(B, 256, 128 MB / bytes of one partial).  No float atomics: reruns are bitwise identical.
#include "listenc_dev.hpp"

namespace rc {

struct SmGeom {      // everything derived from (nq, nk, d, H, d_ff); host side, copied into the kernel arguments
  int nq, nk, d, H, dk, dff;
  int NQP, QT, NKP, KT;             // query-side and key-side rows padded to 16-row tiles
  int XS, KS, FS, SS;               // LDS row strides: d, 2d, d_ff, NKP, each + 4
  int RF, RB;                       // floats of the region k | v (and Ks, or dK | dV and q) share with the feed-forward's buffers
  int64_t P, PS;                    // floats of one partial (the twelve gradients, then [nq][d] of a shared dQs), and its stride
  size_t lds_fwd, lds_bwd;
};

struct SmArgs {
  const float* Qs;
  const float* Ks;
  const uint8_t* pad;  // null: no key is masked
  LeWeights w;
  float* Y;            // forward
  const float* dY;     // backward
  float* dQs;
  float* dKs;
  float* part;
  int64_t B;
  int shared;          // Qs is [nq, d], the same rows for every list
  SmGeom g;
};

static SmGeom sm_geometry(int nq, int nk, int d, int H, int dff) {
  SmGeom g{};
  g.nq = nq, g.nk = nk, g.d = d, g.H = H, g.dk = d / H, g.dff = dff;
  g.NQP = (nq + 15) / 16 * 16, g.QT = g.NQP / 16;
  g.NKP = (nk + 15) / 16 * 16, g.KT = g.NKP / 16;
  g.XS = d + 4, g.KS = 2 * d + 4, g.FS = dff + 4, g.SS = g.NKP + 4;
  const int kvf = g.NKP * (g.XS + g.KS), hf = g.NQP * g.FS;
  g.RF = kvf > hf ? kvf : hf;
  const int attn = g.NQP * g.XS + 2 * g.NKP * g.KS, ffn = g.NQP * (2 * g.XS + g.FS);
  g.RB = attn > ffn ? attn : ffn;
  g.P = le_offsets(d, dff).end + (int64_t)nq * d;
  g.PS = (g.P + 63) / 64 * 64;
  g.lds_fwd = ((size_t)3 * g.NQP * g.XS + g.RF + 64 * (size_t)g.SS + g.NKP) * sizeof(float);
  g.lds_bwd = ((size_t)3 * g.NQP * g.XS + (size_t)g.NKP * g.XS + g.RB + 64 * (size_t)g.SS + g.NKP + g.NQP) * sizeof(float);
  return g;
}

static int sm_blocks_bwd(const SmGeom& g, int64_t B) {
  int64_t b = B < kLeMaxBlocksBwd ? B : kLeMaxBlocksBwd;
  int64_t cap = (int64_t)(kLePartialBudget / ((size_t)g.PS * sizeof(float)));
  if (cap < 1) cap = 1;
  return (int)(b < cap ? b : cap);
}

// ---- device pieces -----------------------------------------------------------------------------------------------------------------
// rows [0, n) of one row set -> dst [NP][XS], zero rows past n
__device__ __forceinline__ void sm_load_rows(const float* X, int n, int NP, int d, int XS, float* dst, int tid) {
  const int Q4 = d / 4;
  for (int idx = tid; idx < NP * Q4; idx += 256) {
    const int row = idx / Q4, c = 4 * (idx - row * Q4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < n) v = load_stream4(reinterpret_cast<const float4*>(X + (int64_t)row * d + c));
    *reinterpret_cast<float4*>(&dst[row * XS + c]) = v;
  }
}

__device__ __forceinline__ void sm_mask(const SmGeom& g, const uint8_t* pad, float* madd, int tid) {
  if (tid < g.NKP) madd[tid] = (tid < g.nk && (pad == nullptr || pad[tid] == 0)) ? 0.f : -INFINITY;
}

// S[16][SS] = q_h . k_h * scale + madd over all 16 KT keys, for the query rows of tile rt; Q [..][qs], K [..][ks]
template <int KT>
__device__ __forceinline__ void sm_scores(const float* Q, int qs, const float* K, int ks, int dk, int h, int rt, float scale,
                                          const float* madd, float* S, int SS, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const float* qp = Q + (16 * rt + i) * qs + h * dk + g;
#pragma unroll
  for (int ct = 0; ct < KT; ++ct) {
    const float* kp = K + (16 * ct + i) * ks + h * dk + g;
    le_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < dk; k0 += 4) acc = LE_MFMA(qp[k0], kp[k0], acc);
    const float m = madd[16 * ct + i];
#pragma unroll
    for (int v = 0; v < 4; ++v) S[(4 * g + v) * SS + 16 * ct + i] = acc[v] * scale + m;
  }
}

// the attention of every (head, query tile) job: Q [NQP][XS], KV [NKP][KS] (k | v) -> out [NQP][XS]; ends synchronised
template <int QT, int KT>
__device__ __forceinline__ void sm_attention(const SmGeom& g, const float* Q, const float* KV, const float* madd, float* Sw, float* out,
                                             int wave, int lane) {
  const float scale = 1.f / sqrtf((float)g.dk);
  const int jobs = g.H * QT;
  for (int job0 = 0; job0 < jobs; job0 += 4) {
    const int job = job0 + wave;
    const bool act = job < jobs;        // (wave-uniform; the barriers are reached by every wave)
    const int h = job / QT, rt = job - h * QT;
    if (act) sm_scores<KT>(Q, g.XS, KV, g.KS, g.dk, h, rt, scale, madd, Sw, g.SS, lane);
    __syncthreads();
    if (act) le_softmax(Sw, g.SS, 16 * KT, lane);
    __syncthreads();
    if (act) le_pv(Sw, g.SS, 16 * KT, KV + g.d, g.KS, g.dk, h, rt, out, g.XS, lane);
    __syncthreads();
  }
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <int QT, int KT>
__global__ __launch_bounds__(256) void setmab_fwd_kernel(SmArgs a) {
  const SmGeom& g = a.g;
  constexpr int NQP = 16 * QT, NKP = 16 * KT;
  extern __shared__ __attribute__((aligned(16))) float sm_lds[];
  float* bX = sm_lds;                  // [NQP][XS]: Qs, then Qs + A, X1, X1 + F
  float* bQ = bX + NQP * g.XS;         // [NQP][XS]: q (a shared source: written once, before the first list)
  float* bA = bQ + NQP * g.XS;         // [NQP][XS]: the heads' outputs
  float* bR = bA + NQP * g.XS;         // Ks and k | v, then relu(X1 W1^T + b1)
  float* bK = bR;                      // [NKP][XS]
  float* bKV = bK + NKP * g.XS;        // [NKP][KS]
  float* bH = bR;                      // [NQP][FS]
  float* bS = bR + g.RF;               // [4 waves][16][SS]
  float* madd = bS + 64 * g.SS;        // [NKP]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int d = g.d, XS = g.XS;
  const bool shared = a.shared != 0;
  if (shared) {
    sm_load_rows(a.Qs, g.nq, NQP, d, XS, bX, tid);
    __syncthreads();
    le_linear<QT, 0>(bX, XS, d, a.w.Win, a.w.bin, d, bQ, XS, nullptr, 0, wave, lane);
  }
  for (int64_t list = blockIdx.x; list < a.B; list += gridDim.x) {
    __syncthreads();   // every wave is done with the previous list's LDS (and with Qs as the shared projection's input)
    sm_load_rows(shared ? a.Qs : a.Qs + list * g.nq * d, g.nq, NQP, d, XS, bX, tid);
    sm_load_rows(a.Ks + list * g.nk * d, g.nk, NKP, d, XS, bK, tid);
    sm_mask(g, a.pad == nullptr ? nullptr : a.pad + list * g.nk, madd, tid);
    __syncthreads();
    if (!shared) le_linear<QT, 0>(bX, XS, d, a.w.Win, a.w.bin, d, bQ, XS, nullptr, 0, wave, lane);
    le_linear<KT, 0>(bK, XS, d, a.w.Win + (int64_t)d * d, a.w.bin + d, 2 * d, bKV, g.KS, nullptr, 0, wave, lane);
    __syncthreads();
    sm_attention<QT, KT>(g, bQ, bKV, madd, bS + wave * 16 * g.SS, bA, wave, lane);
    le_linear<QT, 2>(bA, XS, d, a.w.Wo, a.w.bo, d, bX, XS, bX, XS, wave, lane);            // (a lane re-reads only what it writes)
    __syncthreads();
    for (int row = wave; row < NQP; row += 4) {
      float x[2], mu, rstd;
      le_row_stats(bX + row * XS, d, lane, x, mu, rstd);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = lane + 64 * u;
        if (c < d) bX[row * XS + c] = (x[u] - mu) * rstd * a.w.g1[c] + a.w.be1[c];
      }
    }
    __syncthreads();
    le_linear<QT, 1>(bX, XS, d, a.w.W1, a.w.b1, g.dff, bH, g.FS, nullptr, 0, wave, lane);     // Ks and k | v are dead
    __syncthreads();
    le_linear<QT, 2>(bH, g.FS, g.dff, a.w.W2, a.w.b2, d, bX, XS, bX, XS, wave, lane);
    __syncthreads();
    float* Y = a.Y + list * g.nq * d;
    for (int row = wave; row < g.nq; row += 4) {
      float x[2], mu, rstd;
      le_row_stats(bX + row * XS, d, lane, x, mu, rstd);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = lane + 64 * u;
        if (c < d) Y[(int64_t)row * d + c] = (x[u] - mu) * rstd * a.w.g2[c] + a.w.be2[c];
      }
    }
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// DT = d / 16, FT = d_ff / 16 when the weight-gradient tiles stay in registers, 0 when they go through the partial
template <int QT, int KT, int DT, int FT>
__global__ __launch_bounds__(256) void setmab_bwd_kernel(SmArgs a) {
  const SmGeom& g = a.g;
  constexpr int NQP = 16 * QT, NKP = 16 * KT;
  constexpr bool RES = DT > 0;
  extern __shared__ __attribute__((aligned(16))) float sm_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, gq = lane >> 4;
  const int d = g.d, dff = g.dff, dk = g.dk, XS = g.XS, KS = g.KS, FS = g.FS, SS = g.SS;
  float* bX = sm_lds;                  // [NQP][XS]: Qs (a shared source: loaded once)
  float* bA = bX + NQP * XS;           // [NQP][XS]: the heads' outputs, then dA, then dQ
  float* bG = bA + NQP * XS;           // [NQP][XS]: X1 + F, d(X1 + F), dX1, d(Qs + A)
  float* bK = bG + NQP * XS;           // [NKP][XS]: Ks
  float* bR = bK + NKP * XS;           // [RB]: q, k | v and dK | dV, or X1, x-hat of LN1 and H
  float* bQ = bR;                      // [NQP][XS]
  float* bKV = bQ + NQP * XS;          // [NKP][KS]
  float* bdKV = bKV + NKP * KS;        // [NKP][KS]
  float* bX1 = bR;                     // [NQP][XS]
  float* bXh = bX1 + NQP * XS;         // [NQP][XS]
  float* bH = bXh + NQP * XS;          // [NQP][FS]
  float* bS = bR + g.RB;               // [4 waves][16][SS]
  float* madd = bS + 64 * SS;          // [NKP]
  float* rstd1 = madd + NKP;           // [NQP]
  const int dt = d / 16, ft = dff / 16;
  const LeOffsets o = le_offsets(d, dff);
  float* part = a.part + (int64_t)blockIdx.x * g.PS;
  float* Sw = bS + wave * 16 * SS;
  const float scale = 1.f / sqrtf((float)dk);
  const bool shared = a.shared != 0;
  const float* Wkv = a.w.Win + (int64_t)d * d;

  constexpr int NQ = RES ? (DT * DT + 3) / 4 : 1, NKV = RES ? (2 * DT * DT + 3) / 4 : 1, NF = RES ? (FT * DT + 3) / 4 : 1;
  le_f32x4 wQ[NQ], wKV[NKV], wO[NQ], w1[NF], w2[NF];
  if constexpr (RES) {
#pragma unroll
    for (int t = 0; t < NQ; ++t) wQ[t] = wO[t] = le_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NKV; ++t) wKV[t] = le_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NF; ++t) w1[t] = w2[t] = le_f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float sb2 = 0.f, sb1 = 0.f, sbo = 0.f, sbin[2] = {0.f, 0.f};                         // columns tid (and tid + 256)
  float sg1[2] = {0.f, 0.f}, sbe1[2] = {0.f, 0.f}, sg2[2] = {0.f, 0.f}, sbe2[2] = {0.f, 0.f};   // columns lane, lane + 64; this wave's rows
  bool first = true;

  if (shared) sm_load_rows(a.Qs, g.nq, NQP, d, XS, bX, tid);
  for (int64_t list = blockIdx.x; list < a.B; list += gridDim.x) {
    __syncthreads();
    if (!shared) sm_load_rows(a.Qs + list * g.nq * d, g.nq, NQP, d, XS, bX, tid);
    sm_load_rows(a.Ks + list * g.nk * d, g.nk, NKP, d, XS, bK, tid);
    sm_mask(g, a.pad == nullptr ? nullptr : a.pad + list * g.nk, madd, tid);
    __syncthreads();
    // ---- the block again, from Qs and Ks ----
    le_linear<QT, 0>(bX, XS, d, a.w.Win, a.w.bin, d, bQ, XS, nullptr, 0, wave, lane);
    le_linear<KT, 0>(bK, XS, d, Wkv, a.w.bin + d, 2 * d, bKV, KS, nullptr, 0, wave, lane);
    __syncthreads();
    sm_attention<QT, KT>(g, bQ, bKV, madd, Sw, bA, wave, lane);
    le_linear<QT, 2>(bA, XS, d, a.w.Wo, a.w.bo, d, bX1, XS, bX, XS, wave, lane);       // q, k | v are dead until the attention backward
    __syncthreads();
    for (int row = wave; row < NQP; row += 4) {
      float x[2], mu, rstd;
      le_row_stats(bX1 + row * XS, d, lane, x, mu, rstd);
      if (lane == 0) rstd1[row] = rstd;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = lane + 64 * u;
        if (c < d) {
          const float xh = (x[u] - mu) * rstd;
          bXh[row * XS + c] = xh;
          bX1[row * XS + c] = xh * a.w.g1[c] + a.w.be1[c];
        }
      }
    }
    __syncthreads();
    le_linear<QT, 1>(bX1, XS, d, a.w.W1, a.w.b1, dff, bH, FS, nullptr, 0, wave, lane);
    __syncthreads();
    le_linear<QT, 2>(bH, FS, dff, a.w.W2, a.w.b2, d, bG, XS, bX1, XS, wave, lane);
    __syncthreads();
    // ---- LN2 backward, a wave per row: bG = d(X1 + F); dY rows past nq are zero ----
    {
      const float* dY = a.dY + list * g.nq * d;
      for (int row = wave; row < NQP; row += 4) {
        float x[2], mu, rstd, gdy[2], xh[2];
        le_row_stats(bG + row * XS, d, lane, x, mu, rstd);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int c = lane + 64 * u;
          gdy[u] = xh[u] = 0.f;
          if (c < d) {
            const float dy = row < g.nq ? dY[(int64_t)row * d + c] : 0.f;
            xh[u] = (x[u] - mu) * rstd;
            sg2[u] = fmaf(dy, xh[u], sg2[u]);
            sbe2[u] += dy;
            gdy[u] = dy * a.w.g2[c];
            s1 += gdy[u];
            s2 = fmaf(gdy[u], xh[u], s2);
          }
        }
        s1 = wave_allreduce_sum(s1) / (float)d;
        s2 = wave_allreduce_sum(s2) / (float)d;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int c = lane + 64 * u;
          if (c < d) bG[row * XS + c] = rstd * (gdy[u] - s1 - xh[u] * s2);
        }
      }
    }
    __syncthreads();
    // ---- FFN backward ----
    le_wgrad<DT, FT>(bG, XS, bH, FS, NQP, dt, ft, part + o.W2, first, w2, wave, lane);         // dW2 [d, d_ff] = dF^T H
    if (tid < d) sb2 += le_colsum(bG, XS, NQP, tid);
    __syncthreads();
    for (int ct = wave; ct < ft; ct += 4) {      // dH = (dF W2) where H > 0, in place
      le_f32x4 acc[QT];
      le_zero<QT>(acc);
      le_mm_kn<QT>(bG, XS, d, a.w.W2, dff, 16 * ct, acc, lane);
#pragma unroll
      for (int rt = 0; rt < QT; ++rt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float* p = bH + (16 * rt + 4 * gq + v) * FS + 16 * ct + i;
          *p = *p > 0.f ? acc[rt][v] : 0.f;
        }
    }
    __syncthreads();
    le_wgrad<FT, DT>(bH, FS, bX1, XS, NQP, ft, dt, part + o.W1, first, w1, wave, lane);        // dW1 [d_ff, d] = dH^T X1
    if (tid < dff) sb1 += le_colsum(bH, FS, NQP, tid);
    for (int ct = wave; ct < dt; ct += 4) {      // dX1 = dF + dH W1, in place
      le_f32x4 acc[QT];
      le_zero<QT>(acc);
      le_mm_kn<QT>(bH, FS, dff, a.w.W1, d, 16 * ct, acc, lane);
#pragma unroll
      for (int rt = 0; rt < QT; ++rt)
#pragma unroll
        for (int v = 0; v < 4; ++v) bG[(16 * rt + 4 * gq + v) * XS + 16 * ct + i] += acc[rt][v];
    }
    __syncthreads();
    // ---- LN1 backward: bG = d(Qs + A) ----
    for (int row = wave; row < NQP; row += 4) {
      const float rstd = rstd1[row];
      float gdy[2], xh[2], s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = lane + 64 * u;
        gdy[u] = xh[u] = 0.f;
        if (c < d) {
          const float dy = bG[row * XS + c];
          xh[u] = bXh[row * XS + c];
          sg1[u] = fmaf(dy, xh[u], sg1[u]);
          sbe1[u] += dy;
          gdy[u] = dy * a.w.g1[c];
          s1 += gdy[u];
          s2 = fmaf(gdy[u], xh[u], s2);
        }
      }
      s1 = wave_allreduce_sum(s1) / (float)d;
      s2 = wave_allreduce_sum(s2) / (float)d;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = lane + 64 * u;
        if (c < d) bG[row * XS + c] = rstd * (gdy[u] - s1 - xh[u] * s2);
      }
    }
    __syncthreads();
    // ---- out-projection backward ----
    le_wgrad<DT, DT>(bG, XS, bA, XS, NQP, dt, dt, part + o.Wo, first, wO, wave, lane);         // dWo = dA^T (heads' outputs)
    if (tid < d) sbo += le_colsum(bG, XS, NQP, tid);
    __syncthreads();
    for (int ct = wave; ct < dt; ct += 4) {      // dA -> bA
      le_f32x4 acc[QT];
      le_zero<QT>(acc);
      le_mm_kn<QT>(bG, XS, d, a.w.Wo, d, 16 * ct, acc, lane);
#pragma unroll
      for (int rt = 0; rt < QT; ++rt)
#pragma unroll
        for (int v = 0; v < 4; ++v) bA[(16 * rt + 4 * gq + v) * XS + 16 * ct + i] = acc[rt][v];
    }
    le_linear<QT, 0>(bX, XS, d, a.w.Win, a.w.bin, d, bQ, XS, nullptr, 0, wave, lane);          // X1, x-hat and H are dead
    le_linear<KT, 0>(bK, XS, d, Wkv, a.w.bin + d, 2 * d, bKV, KS, nullptr, 0, wave, lane);
    __syncthreads();
    // ---- attention backward: a wave owns head h and walks the query tiles ----
    for (int h0 = 0; h0 < g.H; h0 += 4) {
      const int h = h0 + wave;
      const bool act = h < g.H;        // (wave-uniform; the barriers are reached by every wave)
      const float* Qh = bQ + h * dk;
      const float* Kh = bKV + h * dk;
      const float* Vh = bKV + d + h * dk;
      float* dAh = bA + h * dk;
      float* dKh = bdKV + h * dk;
      float* dVh = bdKV + d + h * dk;
#pragma unroll 1
      for (int rt = 0; rt < QT; ++rt) {
        if (act) sm_scores<KT>(bQ, XS, bKV, KS, dk, h, rt, scale, madd, Sw, SS, lane);
        __syncthreads();
        if (act) le_softmax(Sw, SS, NKP, lane);
        __syncthreads();
        if (act) {
          // dV_h[key][c] += sum_q P[q][key] dA[16 rt + q][c]
          for (int c0 = 0; c0 < dk; c0 += 16) {
            const bool ok = c0 + i < dk;
            const int cc = ok ? c0 + i : 0;
#pragma unroll
            for (int ct = 0; ct < KT; ++ct) {
              le_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int q0 = 0; q0 < 16; q0 += 4)
                acc = LE_MFMA(Sw[(q0 + gq) * SS + 16 * ct + i], ok ? dAh[(16 * rt + q0 + gq) * XS + cc] : 0.f, acc);
              if (ok) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                  float* p = dVh + (16 * ct + 4 * gq + v) * KS + cc;
                  *p = rt == 0 ? acc[v] : *p + acc[v];
                }
              }
            }
          }
          // dS[q][key] = dA[16 rt + q] . V[key]; D[q] = sum_key P dS; dS <- P (dS - D) scale, in place over P
          le_f32x4 ds[KT];
          float Drow[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ct = 0; ct < KT; ++ct) {
            ds[ct] = le_f32x4{0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < dk; k0 += 4)
              ds[ct] = LE_MFMA(dAh[(16 * rt + i) * XS + k0 + gq], Vh[(16 * ct + i) * KS + k0 + gq], ds[ct]);
#pragma unroll
            for (int v = 0; v < 4; ++v) Drow[v] = fmaf(Sw[(4 * gq + v) * SS + 16 * ct + i], ds[ct][v], Drow[v]);
          }
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            float t = Drow[v];
            t += __shfl_xor(t, 1, 64);
            t += __shfl_xor(t, 2, 64);
            t += __shfl_xor(t, 4, 64);
            t += __shfl_xor(t, 8, 64);
            Drow[v] = t;
          }
#pragma unroll
          for (int ct = 0; ct < KT; ++ct)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              float* p = Sw + (4 * gq + v) * SS + 16 * ct + i;
              *p = *p * (ds[ct][v] - Drow[v]) * scale;
            }
        }
        __syncthreads();
        if (act) {
          for (int c0 = 0; c0 < dk; c0 += 16) {
            const bool ok = c0 + i < dk;
            const int cc = ok ? c0 + i : 0;
            // dQ[16 rt + q][c] = sum_key dS[q][key] K[key][c], over the head's dA columns of this tile (consumed above)
            le_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int j0 = 0; j0 < NKP; j0 += 4) acc = LE_MFMA(Sw[i * SS + j0 + gq], ok ? Kh[(j0 + gq) * KS + cc] : 0.f, acc);
            if (ok) {
#pragma unroll
              for (int v = 0; v < 4; ++v) dAh[(16 * rt + 4 * gq + v) * XS + cc] = acc[v];
            }
            // dK_h[key][c] += sum_q dS[q][key] Q[16 rt + q][c]
#pragma unroll
            for (int ct = 0; ct < KT; ++ct) {
              le_f32x4 kacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int q0 = 0; q0 < 16; q0 += 4)
                kacc = LE_MFMA(Sw[(q0 + gq) * SS + 16 * ct + i], ok ? Qh[(16 * rt + q0 + gq) * XS + cc] : 0.f, kacc);
              if (ok) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                  float* p = dKh + (16 * ct + 4 * gq + v) * KS + cc;
                  *p = rt == 0 ? kacc[v] : *p + kacc[v];
                }
              }
            }
          }
        }
        __syncthreads();
      }
    }
    // ---- in-projection backward: dWq = dQ^T Qs, dWk | dWv = [dK | dV]^T Ks, dQs = d(Qs + A) + dQ Wq, dKs = [dK | dV] Wkv ----
    le_wgrad<DT, DT>(bA, XS, bX, XS, NQP, dt, dt, part + o.Win, first, wQ, wave, lane);
    le_wgrad<2 * DT, DT>(bdKV, KS, bK, XS, NKP, 2 * dt, dt, part + o.Win + (int64_t)d * d, first, wKV, wave, lane);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = tid + 256 * u;
      if (c < d) sbin[u] += le_colsum(bA, XS, NQP, c);
      else if (c < 3 * d) sbin[u] += le_colsum(bdKV, KS, NKP, c - d);
    }
    {
      float* dQs = shared ? part + o.end : a.dQs + list * g.nq * d;
      float* dKs = a.dKs + list * g.nk * d;
      for (int ct = wave; ct < dt; ct += 4) {
        le_f32x4 acc[QT];
        le_zero<QT>(acc);
        le_mm_kn<QT>(bA, XS, d, a.w.Win, d, 16 * ct, acc, lane);
#pragma unroll
        for (int rt = 0; rt < QT; ++rt)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int row = 16 * rt + 4 * gq + v, col = 16 * ct + i;
            if (row < g.nq) {
              const float val = bG[row * XS + col] + acc[rt][v];
              float* p = dQs + (int64_t)row * d + col;
              *p = (shared && !first) ? *p + val : val;
            }
          }
        le_f32x4 kacc[KT];
        le_zero<KT>(kacc);
        le_mm_kn<KT>(bdKV, KS, 2 * d, Wkv, d, 16 * ct, kacc, lane);
#pragma unroll
        for (int rt = 0; rt < KT; ++rt)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int row = 16 * rt + 4 * gq + v, col = 16 * ct + i;
            if (row < g.nk) dKs[(int64_t)row * d + col] = kacc[rt][v];
          }
      }
    }
    first = false;
  }
  // ---- this workgroup's partial, written once ----
  if constexpr (RES) {
    le_wflush<DT, DT>(part + o.Win, wQ, wave, lane);
    le_wflush<2 * DT, DT>(part + o.Win + (int64_t)d * d, wKV, wave, lane);
    le_wflush<DT, DT>(part + o.Wo, wO, wave, lane);
    le_wflush<FT, DT>(part + o.W1, w1, wave, lane);
    le_wflush<DT, FT>(part + o.W2, w2, wave, lane);
  }
  if (tid < d) part[o.b2 + tid] = sb2, part[o.bo + tid] = sbo;
  if (tid < dff) part[o.b1 + tid] = sb1;
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (tid + 256 * u < 3 * d) part[o.bin + tid + 256 * u] = sbin[u];
  // the LayerNorm gradients: the four waves' row shares in wave order
  __syncthreads();
  float* red = bA;       // [4 vectors][4 waves][d]: 16 d floats, within the two [NQP][d + 4] buffers after Qs
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = lane + 64 * u;
    if (c < d) {
      red[(0 * 4 + wave) * d + c] = sg1[u];
      red[(1 * 4 + wave) * d + c] = sbe1[u];
      red[(2 * 4 + wave) * d + c] = sg2[u];
      red[(3 * 4 + wave) * d + c] = sbe2[u];
    }
  }
  __syncthreads();
  if (tid < d) {
    const int64_t at[4] = {o.g1, o.be1, o.g2, o.be2};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      part[at[k] + tid] = ((red[(k * 4 + 0) * d + tid] + red[(k * 4 + 1) * d + tid]) + red[(k * 4 + 2) * d + tid]) + red[(k * 4 + 3) * d + tid];
  }
}

// a shared query source's gradient: one thread per element, the workgroups' partials in workgroup order, in double
__global__ __launch_bounds__(kBlock) void setmab_dqs_reduce_kernel(const float* __restrict__ part, int blocks, int64_t PS, int n,
                                                                   float* __restrict__ dQs) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= n) return;
  double acc = 0.0;
  for (int p = 0; p < blocks; ++p) acc += (double)part[p * PS + e];
  dQs[e] = (float)acc;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
// the one statement of the envelope: every entry point checks it, rc_setmab_check_shape reports it to the host
static int sm_shape(const char* fn, int nq, int nk, int d, int H, int dff, SmGeom* out) {
  const bool ok = nq >= 1 && nq <= 64 && nk >= 1 && nk <= 64 && d % 16 == 0 && d >= 16 && d <= 128 && H >= 1 && d % H == 0 &&
                  (d / H) % 4 == 0 && dff % 16 == 0 && dff >= 16 && dff <= 256;
  if (!ok)
    return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (query rows and key rows in [1, 64], width a multiple of 16 in [16, 128], "
                "heads a divisor of the width with width / heads a multiple of 4, feed-forward width a multiple of 16 in [16, 256]): "
                "nq=%d nk=%d d=%d heads=%d d_ff=%d", fn, nq, nk, d, H, dff);
  const SmGeom g = sm_geometry(nq, nk, d, H, dff);
  if (g.lds_fwd > kLeLdsBudget || g.lds_bwd > kLeLdsBudget)
    return fail(RC_ERR_UNSUPPORTED, "%s: %d query rows (padded to %d) and %d key rows (padded to %d) at width %d, d_ff %d need %zu bytes "
                "of LDS in the backward, %zu are there", fn, nq, g.NQP, nk, g.NKP, d, dff, g.lds_bwd > g.lds_fwd ? g.lds_bwd : g.lds_fwd,
                kLeLdsBudget);
  *out = g;
  return RC_OK;
}

static int sm_check(const char* fn, int64_t B, int nq, int nk, int d, int H, int dff, SmGeom* g) {
  RC_TRY(sm_shape(fn, nq, nk, d, H, dff, g));
  if (B < 1 || B > ((int64_t)1 << 24))
    return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (lists in [1, 2^24]): lists=%lld", fn, (long long)B);
  return RC_OK;
}

template <int QT, int KT>
static int sm_run_qk(const SmArgs& a, bool bwd, int blocks, hipStream_t st) {
  if (!bwd) return le_launch(setmab_fwd_kernel<QT, KT>, 0, a, a.g.lds_fwd, blocks, st);
  if (a.g.d == 64 && a.g.dff == 128) return le_launch(setmab_bwd_kernel<QT, KT, 4, 8>, 0, a, a.g.lds_bwd, blocks, st);
  return le_launch(setmab_bwd_kernel<QT, KT, 0, 0>, 0, a, a.g.lds_bwd, blocks, st);
}

template <int QT>
static int sm_run_q(const SmArgs& a, bool bwd, int blocks, hipStream_t st) {
  switch (a.g.KT) {
    case 1: return sm_run_qk<QT, 1>(a, bwd, blocks, st);
    case 2: return sm_run_qk<QT, 2>(a, bwd, blocks, st);
    case 3: return sm_run_qk<QT, 3>(a, bwd, blocks, st);
    default: return sm_run_qk<QT, 4>(a, bwd, blocks, st);
  }
}

static int sm_run(const SmArgs& a, bool bwd, int blocks, hipStream_t st) {
  switch (a.g.QT) {
    case 1: return sm_run_q<1>(a, bwd, blocks, st);
    case 2: return sm_run_q<2>(a, bwd, blocks, st);
    case 3: return sm_run_q<3>(a, bwd, blocks, st);
    default: return sm_run_q<4>(a, bwd, blocks, st);
  }
}

static int sm_fwd_impl(const float* Qs, const float* Ks, const uint8_t* pad, const LeWeights& w, int64_t B, int nq, int nk, int d, int H,
                       int dff, int shared, float* Y, rc_stream_t stream) {
  const char* fn = "rc_setmab_fwd";
  SmGeom g;
  RC_TRY(sm_check(fn, B, nq, nk, d, H, dff, &g));
  RC_REQUIRE(Qs != nullptr && Ks != nullptr && Y != nullptr && le_weights_ok(w) && aligned16(Qs, Ks, Y),
             "%s: null pointer, or a float tensor that is not 16-byte aligned", fn);
  SmArgs a{Qs, Ks, pad, w, Y, nullptr, nullptr, nullptr, nullptr, B, shared != 0, g};
  return sm_run(a, false, (int)(B < kLeMaxBlocksFwd ? B : kLeMaxBlocksFwd), as_stream(stream));
}

static int sm_bwd_impl(const float* dY, const float* Qs, const float* Ks, const uint8_t* pad, const LeWeights& w, int64_t B, int nq,
                       int nk, int d, int H, int dff, int shared, void* workspace, size_t ws_bytes, float* dQs, float* dKs,
                       const LeGrads& gr, rc_stream_t stream) {
  const char* fn = "rc_setmab_bwd";
  SmGeom g;
  RC_TRY(sm_check(fn, B, nq, nk, d, H, dff, &g));
  RC_REQUIRE(dY != nullptr && Qs != nullptr && Ks != nullptr && dQs != nullptr && dKs != nullptr && le_weights_ok(w) &&
             aligned16(dY, Qs, Ks, dQs, dKs), "%s: null pointer, or a float tensor that is not 16-byte aligned", fn);
  RC_REQUIRE(gr.Win != nullptr && gr.bin != nullptr && gr.Wo != nullptr && gr.bo != nullptr && gr.g1 != nullptr && gr.be1 != nullptr &&
             gr.W1 != nullptr && gr.b1 != nullptr && gr.W2 != nullptr && gr.b2 != nullptr && gr.g2 != nullptr && gr.be2 != nullptr,
             "%s: null gradient pointer", fn);
  RC_REQUIRE(workspace != nullptr && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "%s: workspace must be 256-byte aligned", fn);
  const int blocks = sm_blocks_bwd(g, B);
  Carver c(workspace);
  float* part = c.take<float>((size_t)blocks * g.PS);
  if (ws_bytes < c.off) return fail(RC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, c.off);
  const hipStream_t st = as_stream(stream);
  SmArgs a{Qs, Ks, pad, w, nullptr, dY, dQs, dKs, part, B, shared != 0, g};
  RC_TRY(sm_run(a, true, blocks, st));
  const LeOffsets o = le_offsets(d, dff);
  hipLaunchKernelGGL(listenc_grad_reduce_kernel, dim3((unsigned)((o.end + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, part, blocks, g.PS,
                     o, gr);
  RC_LAUNCH_CHECK();
  if (shared) {
    hipLaunchKernelGGL(setmab_dqs_reduce_kernel, dim3((unsigned)((nq * d + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, part + o.end,
                       blocks, g.PS, nq * d, dQs);
    RC_LAUNCH_CHECK();
  }
  return RC_OK;
}

}  // namespace rc

extern "C" enum rc_status rc_setmab_check_shape(int nq, int nk, int d, int heads, int d_ff) {
  rc::SmGeom g;
  return (enum rc_status)rc::sm_shape("rc_setmab_check_shape", nq, nk, d, heads, d_ff, &g);
}

extern "C" size_t rc_setmab_bwd_workspace_bytes(int64_t B, int nq, int nk, int d, int heads, int d_ff) {
  using namespace rc;
  SmGeom g;
  if (sm_check("rc_setmab_bwd_workspace_bytes", B, nq, nk, d, heads, d_ff, &g) != RC_OK) return 0;
  Carver c(nullptr);
  c.take<float>((size_t)sm_blocks_bwd(g, B) * g.PS);
  return c.off;
}

extern "C" enum rc_status rc_setmab_fwd(const float* Qs, const float* Ks, const uint8_t* pad, const float* Win, const float* bin,
                                        const float* Wo, const float* bo, const float* g1, const float* be1, const float* W1,
                                        const float* b1, const float* W2, const float* b2, const float* g2, const float* be2, int64_t B,
                                        int nq, int nk, int d, int heads, int d_ff, int shared_q, float* Y, rc_stream_t stream) {
  const rc::LeWeights w{Win, bin, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2};
  return (enum rc_status)rc::sm_fwd_impl(Qs, Ks, pad, w, B, nq, nk, d, heads, d_ff, shared_q, Y, stream);
}

extern "C" enum rc_status rc_setmab_bwd(const float* dY, const float* Qs, const float* Ks, const uint8_t* pad, const float* Win,
                                        const float* bin, const float* Wo, const float* bo, const float* g1, const float* be1,
                                        const float* W1, const float* b1, const float* W2, const float* b2, const float* g2,
                                        const float* be2, int64_t B, int nq, int nk, int d, int heads, int d_ff, int shared_q,
                                        void* workspace, size_t ws_bytes, float* dQs, float* dKs, float* dWin, float* dbin, float* dWo,
                                        float* dbo, float* dg1, float* dbe1, float* dW1, float* db1, float* dW2, float* db2, float* dg2,
                                        float* dbe2, rc_stream_t stream) {
  const rc::LeWeights w{Win, bin, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2};
  const rc::LeGrads gr{dWin, dbin, dWo, dbo, dg1, dbe1, dW1, db1, dW2, db2, dg2, dbe2};
  return (enum rc_status)rc::sm_bwd_impl(dY, Qs, Ks, pad, w, B, nq, nk, d, heads, d_ff, shared_q, workspace, ws_bytes, dQs, dKs, gr, stream);
}
