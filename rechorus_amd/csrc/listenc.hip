// listenc.hip -- one post-norm transformer encoder block over short candidate lists (reference: models/reranker/PRM.py:64,90-92,
// i.e. nn.TransformerEncoderLayer(d, H, d_ff, dropout=0), norm_first=False, ReLU, eps 1e-5, with a key-padding mask)
//
//   X [B, n, d] list-major, pad uint8 [B, n] (1 = padded slot: masked as a KEY only; as a query it is a row like any other)
//   QKV = X Win^T + bin (Win [3d, d], q | k | v),  P_h = softmax_j(q_h . k_h / sqrt(dk)) over the keys with pad == 0,
//   A = concat_h(P_h V_h) Wo^T + bo,  X1 = LN1(X + A),  Y = LN2(X1 + relu(X1 W1^T + b1) W2^T + b2)
//
// Launches: the forward is ONE launch per block; the backward is TWO (the list kernel and the fixed-order reduce of its partials).
//   list    a workgroup of four waves owns one list at a time and walks the batch with the grid as its stride.  The list's rows,
//           padded with zero rows to NP = 16 RT (RT = 1..4 row tiles), and every intermediate live in LDS as [NP][width + 4].
//   MFMA    all six products run on v_mfma_f32_16x16x4_f32: the rows are the A operand out of LDS, the weights the B operand straight
//           from global memory (one block's weights are 128 KB at d = 64, d_ff = 128: L2-resident and read by every workgroup).  A
//           wave takes 16-wide output column tiles and keeps RT accumulators per tile, so a weight operand is used RT times.
//   attn    a job is (head, 16-row query tile): scores against all NP keys into the wave's own [16][NP + 4] scratch, a 4-lanes-per-row
//           softmax, then P V.  Keys past n and keys with pad == 1 get -inf.  The forward writes the head's output over its own Q
//           columns (nobody else reads them).
//   bwd     recomputes the block from X and runs in phases (barriers between): QKV, attention, LN1 (x-hat kept), FFN, LN2 backward,
//           FFN backward, LN1 backward, out-projection backward, QKV again (its LDS was the FFN's in between), attention backward
//           (a wave owns a head and walks the query tiles: dV, dS, the softmax backward in place over P, dQ over the head's dA
//           columns, dK), in-projection backward.  dX is written once.
//   wgrad   weight gradients are rank-NP updates dOut^T In on the same MFMA.  At d = 64, d_ff = 128 (the default) the 128 16x16 tiles of
//           Win, Wo, W1, W2 are 32 accumulator tiles = 128 registers per lane and stay in REGISTERS across all the lists a workgroup
//           walks; they are stored to the workgroup's partial once, at the end.  Other shapes add into the partial in global memory
//           per list (plain loads and stores: nobody else touches it; the first list stores without loading).  Bias and LayerNorm
//           gradients are per-thread register sums over the lists in both cases.
//   reduce  one thread per weight-gradient element adds the workgroups' partials in workgroup order, in double.
// The number of workgroups (= partials) is min(B, 256, 128 MB / bytes of one partial): independent of B past 256 lists.
// No float atomics anywhere: every sum has a fixed order, results are bitwise reproducible run to run.
#include "listenc_dev.hpp"

namespace rc {

struct LeGeom {      // everything derived from (n, d, H, d_ff); host side, copied into the kernel arguments
  int n, d, H, dk, dff;
  int NP, RT;                       // rows padded to 16-row tiles
  int XS, QS, KS, FS, WS, SS;       // LDS row strides: d, 3d, 2d, d_ff, max(3d, d_ff), NP, each + 4
  int RW;                           // backward: floats per row of the region QKV | dKV share with X1 | x-hat | H
  int64_t P, PS;                    // floats of one partial, and its stride (256-byte multiple)
  size_t lds_fwd, lds_bwd;
};

struct LeArgs {
  const float* X;
  const uint8_t* pad;
  LeWeights w;
  float* Y;            // forward
  const float* dY;     // backward
  float* dX;
  float* part;
  int64_t B;
  LeGeom g;
};

static LeGeom le_geometry(int n, int d, int H, int dff) {
  LeGeom g{};
  g.n = n, g.d = d, g.H = H, g.dk = d / H, g.dff = dff;
  g.NP = (n + 15) / 16 * 16, g.RT = g.NP / 16;
  g.XS = d + 4, g.QS = 3 * d + 4, g.KS = 2 * d + 4, g.FS = dff + 4, g.SS = g.NP + 4;
  g.WS = (3 * d > dff ? 3 * d : dff) + 4;
  const int attn = g.QS + g.KS, ffn = 2 * g.XS + g.FS;
  g.RW = attn > ffn ? attn : ffn;
  g.P = le_offsets(d, dff).end;
  g.PS = (g.P + 63) / 64 * 64;
  const size_t NP = (size_t)g.NP;
  g.lds_fwd = (NP * g.XS + NP * g.WS + 64 * (size_t)g.SS + NP) * sizeof(float);
  g.lds_bwd = (3 * NP * g.XS + NP * g.RW + 64 * (size_t)g.SS + 2 * NP) * sizeof(float);
  return g;
}

static int le_blocks_bwd(const LeGeom& g, int64_t B) {
  int64_t b = B < kLeMaxBlocksBwd ? B : kLeMaxBlocksBwd;
  int64_t cap = (int64_t)(kLePartialBudget / ((size_t)g.PS * sizeof(float)));
  if (cap < 1) cap = 1;
  return (int)(b < cap ? b : cap);
}

// rows [0, n) of one list -> dst [NP][XS], zero rows past n
__device__ __forceinline__ void le_load_rows(const LeGeom& g, const float* X, float* dst, int tid) {
  const int Q4 = g.d / 4;
  for (int idx = tid; idx < g.NP * Q4; idx += 256) {
    const int row = idx / Q4, c = 4 * (idx - row * Q4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < g.n) v = load_stream4(reinterpret_cast<const float4*>(X + (int64_t)row * g.d + c));
    *reinterpret_cast<float4*>(&dst[row * g.XS + c]) = v;
  }
}

// S[16][SS] = q_h . k_h * scale + madd over all NP keys, for the query rows of tile rt
template <int RT>
__device__ __forceinline__ void le_scores(const float* Q, const float* K, int qs, int dk, int h, int rt, float scale, const float* madd,
                                          float* S, int SS, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const float* qp = Q + (16 * rt + i) * qs + h * dk + g;
#pragma unroll
  for (int ct = 0; ct < RT; ++ct) {
    const float* kp = K + (16 * ct + i) * qs + h * dk + g;
    le_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < dk; k0 += 4) acc = LE_MFMA(qp[k0], kp[k0], acc);
    const float m = madd[16 * ct + i];
#pragma unroll
    for (int v = 0; v < 4; ++v) S[(4 * g + v) * SS + 16 * ct + i] = acc[v] * scale + m;
  }
}

// the attention of every (head, query tile) job: QKV [NP][qs] (q | k | v) -> out [NP][os]; ends synchronised
template <int RT>
__device__ __forceinline__ void le_attention(const LeGeom& g, const float* QKV, const float* madd, float* Sw, float* out, int os, int wave,
                                             int lane) {
  const float scale = 1.f / sqrtf((float)g.dk);
  const int jobs = g.H * RT;
  for (int job0 = 0; job0 < jobs; job0 += 4) {
    const int job = job0 + wave;
    const bool act = job < jobs;        // (wave-uniform; the barriers are reached by every wave)
    const int h = job / RT, rt = job - h * RT;
    if (act) le_scores<RT>(QKV, QKV + g.d, g.QS, g.dk, h, rt, scale, madd, Sw, g.SS, lane);
    __syncthreads();
    if (act) le_softmax(Sw, g.SS, g.NP, lane);
    __syncthreads();
    if (act) le_pv(Sw, g.SS, g.NP, QKV + 2 * g.d, g.QS, g.dk, h, rt, out, os, lane);
    __syncthreads();
  }
}

__device__ __forceinline__ void le_mask(const LeGeom& g, const uint8_t* pad, float* madd, int tid) {
  if (tid < g.NP) madd[tid] = (tid < g.n && pad[tid] == 0) ? 0.f : -INFINITY;
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <int RT>
__global__ __launch_bounds__(256) void listenc_fwd_kernel(LeArgs a) {
  const LeGeom& g = a.g;
  constexpr int NP = 16 * RT;
  extern __shared__ __attribute__((aligned(16))) float le_lds[];
  float* bX = le_lds;                  // [NP][XS]: X, then X + A, X1, X1 + F
  float* bW = bX + NP * g.XS;          // [NP][WS]: q | k | v (the heads' outputs over q), then relu(X1 W1^T + b1)
  float* bS = bW + NP * g.WS;          // [4 waves][16][SS]
  float* madd = bS + 64 * g.SS;        // [NP]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int d = g.d;
  for (int64_t list = blockIdx.x; list < a.B; list += gridDim.x) {
    __syncthreads();   // every wave is done with the previous list's LDS
    le_load_rows(g, a.X + list * g.n * d, bX, tid);
    le_mask(g, a.pad + list * g.n, madd, tid);
    __syncthreads();
    le_linear<RT, 0>(bX, g.XS, d, a.w.Win, a.w.bin, 3 * d, bW, g.QS, nullptr, 0, wave, lane);
    __syncthreads();
    le_attention<RT>(g, bW, madd, bS + wave * 16 * g.SS, bW, g.QS, wave, lane);
    le_linear<RT, 2>(bW, g.QS, d, a.w.Wo, a.w.bo, d, bX, g.XS, bX, g.XS, wave, lane);      // (a lane re-reads only what it writes)
    __syncthreads();
    for (int row = wave; row < NP; row += 4) {
      float x[2], mu, rstd;
      le_row_stats(bX + row * g.XS, d, lane, x, mu, rstd);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = lane + 64 * u;
        if (c < d) bX[row * g.XS + c] = (x[u] - mu) * rstd * a.w.g1[c] + a.w.be1[c];
      }
    }
    __syncthreads();
    le_linear<RT, 1>(bX, g.XS, d, a.w.W1, a.w.b1, g.dff, bW, g.FS, nullptr, 0, wave, lane);
    __syncthreads();
    le_linear<RT, 2>(bW, g.FS, g.dff, a.w.W2, a.w.b2, d, bX, g.XS, bX, g.XS, wave, lane);
    __syncthreads();
    float* Y = a.Y + list * g.n * d;
    for (int row = wave; row < g.n; row += 4) {
      float x[2], mu, rstd;
      le_row_stats(bX + row * g.XS, d, lane, x, mu, rstd);
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
template <int RT, int DT, int FT>
__global__ __launch_bounds__(256) void listenc_bwd_kernel(LeArgs a) {
  const LeGeom& g = a.g;
  constexpr int NP = 16 * RT;
  constexpr bool RES = DT > 0;
  extern __shared__ __attribute__((aligned(16))) float le_lds[];
  float* bX = le_lds;                  // [NP][XS]: X
  float* bA = bX + NP * g.XS;          // [NP][XS]: the heads' outputs, then dA, then dQ
  float* bG = bA + NP * g.XS;          // [NP][XS]: X1 + F, d(X1 + F), dX1, d(X + A)
  float* bR = bG + NP * g.XS;          // [NP][RW]: q | k | v and dK | dV, or X1, x-hat of LN1 and H
  float* bQKV = bR;                    // [NP][QS]
  float* bKV = bR + NP * g.QS;         // [NP][KS]: dK | dV
  float* bX1 = bR;                     // [NP][XS]
  float* bXh = bX1 + NP * g.XS;        // [NP][XS]
  float* bH = bXh + NP * g.XS;         // [NP][FS]
  float* bS = bR + NP * g.RW;          // [4 waves][16][SS]
  float* madd = bS + 64 * g.SS;        // [NP]
  float* rstd1 = madd + NP;            // [NP]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, gq = lane >> 4;
  const int d = g.d, dff = g.dff, dk = g.dk, XS = g.XS, QS = g.QS, KS = g.KS, FS = g.FS, SS = g.SS;
  const int dt = d / 16, ft = dff / 16;
  const LeOffsets o = le_offsets(d, dff);
  float* part = a.part + (int64_t)blockIdx.x * g.PS;
  float* Sw = bS + wave * 16 * SS;
  const float scale = 1.f / sqrtf((float)dk);

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

  for (int64_t list = blockIdx.x; list < a.B; list += gridDim.x) {
    __syncthreads();
    le_load_rows(g, a.X + list * g.n * d, bX, tid);
    le_mask(g, a.pad + list * g.n, madd, tid);
    __syncthreads();
    // ---- the block again, from X ----
    le_linear<RT, 0>(bX, XS, d, a.w.Win, a.w.bin, 3 * d, bQKV, QS, nullptr, 0, wave, lane);
    __syncthreads();
    le_attention<RT>(g, bQKV, madd, Sw, bA, XS, wave, lane);
    le_linear<RT, 2>(bA, XS, d, a.w.Wo, a.w.bo, d, bX1, XS, bX, XS, wave, lane);       // q | k | v are dead until the attention backward
    __syncthreads();
    for (int row = wave; row < NP; row += 4) {
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
    le_linear<RT, 1>(bX1, XS, d, a.w.W1, a.w.b1, dff, bH, FS, nullptr, 0, wave, lane);
    __syncthreads();
    le_linear<RT, 2>(bH, FS, dff, a.w.W2, a.w.b2, d, bG, XS, bX1, XS, wave, lane);
    __syncthreads();
    // ---- LN2 backward, a wave per row: bG = d(X1 + F); dY rows past n are zero ----
    {
      const float* dY = a.dY + list * g.n * d;
      for (int row = wave; row < NP; row += 4) {
        float x[2], mu, rstd, gdy[2], xh[2];
        le_row_stats(bG + row * XS, d, lane, x, mu, rstd);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int c = lane + 64 * u;
          gdy[u] = xh[u] = 0.f;
          if (c < d) {
            const float dy = row < g.n ? dY[(int64_t)row * d + c] : 0.f;
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
    le_wgrad<DT, FT>(bG, XS, bH, FS, NP, dt, ft, part + o.W2, first, w2, wave, lane);          // dW2 [d, d_ff] = dF^T H
    if (tid < d) sb2 += le_colsum(bG, XS, NP, tid);
    __syncthreads();
    for (int ct = wave; ct < ft; ct += 4) {      // dH = (dF W2) where H > 0, in place
      le_f32x4 acc[RT];
      le_zero<RT>(acc);
      le_mm_kn<RT>(bG, XS, d, a.w.W2, dff, 16 * ct, acc, lane);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float* p = bH + (16 * rt + 4 * gq + v) * FS + 16 * ct + i;
          *p = *p > 0.f ? acc[rt][v] : 0.f;
        }
    }
    __syncthreads();
    le_wgrad<FT, DT>(bH, FS, bX1, XS, NP, ft, dt, part + o.W1, first, w1, wave, lane);         // dW1 [d_ff, d] = dH^T X1
    if (tid < dff) sb1 += le_colsum(bH, FS, NP, tid);
    for (int ct = wave; ct < dt; ct += 4) {      // dX1 = dF + dH W1, in place
      le_f32x4 acc[RT];
      le_zero<RT>(acc);
      le_mm_kn<RT>(bH, FS, dff, a.w.W1, d, 16 * ct, acc, lane);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int v = 0; v < 4; ++v) bG[(16 * rt + 4 * gq + v) * XS + 16 * ct + i] += acc[rt][v];
    }
    __syncthreads();
    // ---- LN1 backward: bG = d(X + A) ----
    for (int row = wave; row < NP; row += 4) {
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
    le_wgrad<DT, DT>(bG, XS, bA, XS, NP, dt, dt, part + o.Wo, first, wO, wave, lane);          // dWo = dA^T (heads' outputs)
    if (tid < d) sbo += le_colsum(bG, XS, NP, tid);
    __syncthreads();
    for (int ct = wave; ct < dt; ct += 4) {      // dA -> bA
      le_f32x4 acc[RT];
      le_zero<RT>(acc);
      le_mm_kn<RT>(bG, XS, d, a.w.Wo, d, 16 * ct, acc, lane);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int v = 0; v < 4; ++v) bA[(16 * rt + 4 * gq + v) * XS + 16 * ct + i] = acc[rt][v];
    }
    le_linear<RT, 0>(bX, XS, d, a.w.Win, a.w.bin, 3 * d, bQKV, QS, nullptr, 0, wave, lane);    // X1, x-hat and H are dead
    __syncthreads();
    // ---- attention backward: a wave owns head h and walks the query tiles ----
    for (int h0 = 0; h0 < g.H; h0 += 4) {
      const int h = h0 + wave;
      const bool act = h < g.H;        // (wave-uniform; the barriers are reached by every wave)
      const float* Qh = bQKV + h * dk;
      const float* Kh = bQKV + d + h * dk;
      const float* Vh = bQKV + 2 * d + h * dk;
      float* dAh = bA + h * dk;
      float* dKh = bKV + h * dk;
      float* dVh = bKV + d + h * dk;
#pragma unroll 1
      for (int rt = 0; rt < RT; ++rt) {
        if (act) le_scores<RT>(bQKV, bQKV + d, QS, dk, h, rt, scale, madd, Sw, SS, lane);
        __syncthreads();
        if (act) le_softmax(Sw, SS, NP, lane);
        __syncthreads();
        if (act) {
          // dV_h[key][c] += sum_q P[q][key] dA[16 rt + q][c]
          for (int c0 = 0; c0 < dk; c0 += 16) {
            const bool ok = c0 + i < dk;
            const int cc = ok ? c0 + i : 0;
#pragma unroll
            for (int ct = 0; ct < RT; ++ct) {
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
          le_f32x4 ds[RT];
          float Drow[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ct = 0; ct < RT; ++ct) {
            ds[ct] = le_f32x4{0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < dk; k0 += 4)
              ds[ct] = LE_MFMA(dAh[(16 * rt + i) * XS + k0 + gq], Vh[(16 * ct + i) * QS + k0 + gq], ds[ct]);
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
          for (int ct = 0; ct < RT; ++ct)
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
            for (int j0 = 0; j0 < NP; j0 += 4) acc = LE_MFMA(Sw[i * SS + j0 + gq], ok ? Kh[(j0 + gq) * QS + cc] : 0.f, acc);
            if (ok) {
#pragma unroll
              for (int v = 0; v < 4; ++v) dAh[(16 * rt + 4 * gq + v) * XS + cc] = acc[v];
            }
            // dK_h[key][c] += sum_q dS[q][key] Q[16 rt + q][c]
#pragma unroll
            for (int ct = 0; ct < RT; ++ct) {
              le_f32x4 kacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int q0 = 0; q0 < 16; q0 += 4)
                kacc = LE_MFMA(Sw[(q0 + gq) * SS + 16 * ct + i], ok ? Qh[(16 * rt + q0 + gq) * QS + cc] : 0.f, kacc);
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
    // ---- in-projection backward: dWin = [dQ | dK | dV]^T X, dX = d(X + A) + [dQ | dK | dV] Win ----
    le_wgrad<DT, DT>(bA, XS, bX, XS, NP, dt, dt, part + o.Win, first, wQ, wave, lane);
    le_wgrad<2 * DT, DT>(bKV, KS, bX, XS, NP, 2 * dt, dt, part + o.Win + (int64_t)d * d, first, wKV, wave, lane);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = tid + 256 * u;
      if (c < d) sbin[u] += le_colsum(bA, XS, NP, c);
      else if (c < 3 * d) sbin[u] += le_colsum(bKV, KS, NP, c - d);
    }
    {
      float* dX = a.dX + list * g.n * d;
      for (int ct = wave; ct < dt; ct += 4) {
        le_f32x4 acc[RT];
        le_zero<RT>(acc);
        le_mm_kn<RT>(bA, XS, d, a.w.Win, d, 16 * ct, acc, lane);
        le_mm_kn<RT>(bKV, KS, 2 * d, a.w.Win + (int64_t)d * d, d, 16 * ct, acc, lane);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int row = 16 * rt + 4 * gq + v, col = 16 * ct + i;
            if (row < g.n) dX[(int64_t)row * d + col] = bG[row * XS + col] + acc[rt][v];
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
  float* red = bX;       // [4 vectors][4 waves][d]: 16 d floats, within the three [NP][d + 4] row buffers
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

// ---- host --------------------------------------------------------------------------------------------------------------------------
// the one statement of the envelope: every entry point checks it, rc_listenc_check_shape reports it to the host
static int le_shape(const char* fn, int n, int d, int H, int dff, LeGeom* out) {
  const bool ok = n >= 1 && n <= 64 && d % 16 == 0 && d >= 16 && d <= 128 && H >= 1 && d % H == 0 && (d / H) % 4 == 0 && dff % 16 == 0 &&
                  dff >= 16 && dff <= 256;
  if (!ok)
    return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (list length in [1, 64], width a multiple of 16 in [16, 128], heads a divisor "
                "of the width with width / heads a multiple of 4, feed-forward width a multiple of 16 in [16, 256]): n=%d d=%d heads=%d "
                "d_ff=%d", fn, n, d, H, dff);
  const LeGeom g = le_geometry(n, d, H, dff);
  if (g.lds_fwd > kLeLdsBudget || g.lds_bwd > kLeLdsBudget)
    return fail(RC_ERR_UNSUPPORTED, "%s: a list of %d rows (padded to %d) at width %d, d_ff %d needs %zu bytes of LDS in the backward, "
                "%zu are there", fn, n, g.NP, d, dff, g.lds_bwd > g.lds_fwd ? g.lds_bwd : g.lds_fwd, kLeLdsBudget);
  *out = g;
  return RC_OK;
}

static int le_check(const char* fn, int64_t B, int n, int d, int H, int dff, LeGeom* g) {
  RC_TRY(le_shape(fn, n, d, H, dff, g));
  if (B < 1 || B > ((int64_t)1 << 24))
    return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (lists in [1, 2^24]): lists=%lld", fn, (long long)B);
  return RC_OK;
}

template <int RT>
static int le_run_rt(const LeArgs& a, bool bwd, int blocks, hipStream_t st) {
  if (!bwd) return le_launch(listenc_fwd_kernel<RT>, RT - 1, a, a.g.lds_fwd, blocks, st);
  if (a.g.d == 64 && a.g.dff == 128) return le_launch(listenc_bwd_kernel<RT, 4, 8>, 4 + RT - 1, a, a.g.lds_bwd, blocks, st);
  return le_launch(listenc_bwd_kernel<RT, 0, 0>, 8 + RT - 1, a, a.g.lds_bwd, blocks, st);
}

static int le_run(const LeArgs& a, bool bwd, int blocks, hipStream_t st) {
  switch (a.g.RT) {
    case 1: return le_run_rt<1>(a, bwd, blocks, st);
    case 2: return le_run_rt<2>(a, bwd, blocks, st);
    case 3: return le_run_rt<3>(a, bwd, blocks, st);
    default: return le_run_rt<4>(a, bwd, blocks, st);
  }
}


static int le_fwd_impl(const float* X, const uint8_t* pad, const LeWeights& w, int64_t B, int n, int d, int H, int dff, float* Y,
                       rc_stream_t stream) {
  const char* fn = "rc_listenc_block_fwd";
  LeGeom g;
  RC_TRY(le_check(fn, B, n, d, H, dff, &g));
  RC_REQUIRE(X != nullptr && pad != nullptr && Y != nullptr && le_weights_ok(w) && aligned16(X, Y),
             "%s: null pointer, or a float tensor that is not 16-byte aligned", fn);
  LeArgs a{X, pad, w, Y, nullptr, nullptr, nullptr, B, g};
  return le_run(a, false, (int)(B < kLeMaxBlocksFwd ? B : kLeMaxBlocksFwd), as_stream(stream));
}

static int le_bwd_impl(const float* dY, const float* X, const uint8_t* pad, const LeWeights& w, int64_t B, int n, int d, int H, int dff,
                       void* workspace, size_t ws_bytes, float* dX, const LeGrads& gr, rc_stream_t stream) {
  const char* fn = "rc_listenc_block_bwd";
  LeGeom g;
  RC_TRY(le_check(fn, B, n, d, H, dff, &g));
  RC_REQUIRE(dY != nullptr && X != nullptr && pad != nullptr && dX != nullptr && le_weights_ok(w) && aligned16(dY, X, dX),
             "%s: null pointer, or a float tensor that is not 16-byte aligned", fn);
  RC_REQUIRE(gr.Win != nullptr && gr.bin != nullptr && gr.Wo != nullptr && gr.bo != nullptr && gr.g1 != nullptr && gr.be1 != nullptr &&
             gr.W1 != nullptr && gr.b1 != nullptr && gr.W2 != nullptr && gr.b2 != nullptr && gr.g2 != nullptr && gr.be2 != nullptr,
             "%s: null gradient pointer", fn);
  RC_REQUIRE(workspace != nullptr && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "%s: workspace must be 256-byte aligned", fn);
  const int blocks = le_blocks_bwd(g, B);
  Carver c(workspace);
  float* part = c.take<float>((size_t)blocks * g.PS);
  if (ws_bytes < c.off) return fail(RC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, c.off);
  const hipStream_t st = as_stream(stream);
  LeArgs a{X, pad, w, nullptr, dY, dX, part, B, g};
  RC_TRY(le_run(a, true, blocks, st));
  hipLaunchKernelGGL(listenc_grad_reduce_kernel, dim3((unsigned)((g.P + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, part, blocks, g.PS,
                     le_offsets(d, dff), gr);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

}  // namespace rc

extern "C" enum rc_status rc_listenc_check_shape(int n, int d, int heads, int d_ff) {
  rc::LeGeom g;
  return (enum rc_status)rc::le_shape("rc_listenc_check_shape", n, d, heads, d_ff, &g);
}

extern "C" size_t rc_listenc_block_bwd_workspace_bytes(int64_t B, int n, int d, int heads, int d_ff) {
  using namespace rc;
  LeGeom g;
  if (le_check("rc_listenc_block_bwd_workspace_bytes", B, n, d, heads, d_ff, &g) != RC_OK) return 0;
  Carver c(nullptr);
  c.take<float>((size_t)le_blocks_bwd(g, B) * g.PS);
  return c.off;
}

extern "C" enum rc_status rc_listenc_block_fwd(const float* X, const uint8_t* pad, const float* Win, const float* bin, const float* Wo,
                                               const float* bo, const float* g1, const float* be1, const float* W1, const float* b1,
                                               const float* W2, const float* b2, const float* g2, const float* be2, int64_t B, int n, int d,
                                               int heads, int d_ff, float* Y, rc_stream_t stream) {
  const rc::LeWeights w{Win, bin, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2};
  return (enum rc_status)rc::le_fwd_impl(X, pad, w, B, n, d, heads, d_ff, Y, stream);
}

extern "C" enum rc_status rc_listenc_block_bwd(const float* dY, const float* X, const uint8_t* pad, const float* Win, const float* bin,
                                               const float* Wo, const float* bo, const float* g1, const float* be1, const float* W1,
                                               const float* b1, const float* W2, const float* b2, const float* g2, const float* be2,
                                               int64_t B, int n, int d, int heads, int d_ff, void* workspace, size_t ws_bytes, float* dX,
                                               float* dWin, float* dbin, float* dWo, float* dbo, float* dg1, float* dbe1, float* dW1,
                                               float* db1, float* dW2, float* db2, float* dg2, float* dbe2, rc_stream_t stream) {
  const rc::LeWeights w{Win, bin, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2};
  const rc::LeGrads gr{dWin, dbin, dWo, dbo, dg1, dbe1, dW1, db1, dW2, db2, dg2, dbe2};
  return (enum rc_status)rc::le_bwd_impl(dY, X, pad, w, B, n, d, heads, d_ff, workspace, ws_bytes, dX, gr, stream);
}
