// autoint.hip -- AutoInt's interacting layer: multi-head self-attention across the fields of one instance, linear residual, ReLU
// (reference: models/context/AutoInt.py:49-80, utils/layers.py:9-63)
//
//   X [N, F, Din], N = batch * candidates instances of F fields;  Wq, Wk, Wv, Wr [A, Din], br [A];  H heads of dk = A / H columns
//   Q | K | V = X W^T (no bias),  R = X Wr^T + br
//   per instance and head:  S = Q_h K_h^T / sqrt(dk) [F, F],  P = softmax over the key axis,  O_h = P V_h  (no output projection)
//   Y = relu(O + R) [N, F, A]
// The reference subtracts the GLOBAL maximum of the score tensor before its softmax and replaces NaN by 0 afterwards
// (layers.py:60-61).  Without a mask and for finite inputs the global shift is a mathematical no-op (torch's softmax subtracts the
// row maximum again) and the NaN branch is unreachable, so the kernels use the row maximum.  Finite inputs are part of the envelope.
//
// Launches (one forward, one backward + one reduce per layer):
//   fwd     a workgroup owns a tile of whole instances, TR = 128 / 64 / 32 stacked field rows (TR / F instances), and walks the
//           batch with the grid as its stride.  X [TR][DP + 4] (DP = Din rounded up to 32, zero padded) and the stacked weight
//           block [Wq; Wk; Wv; Wr] (each part in AP = A rounded up to 4 rows) sit in LDS; Q | K | V | R = X W^T on
//           v_mfma_f32_32x32x2_f32 (operand and accumulator maps as in buir.hip: a wave owns 32 stacked rows of one 32-wide output
//           tile, the rows on the lanes, the outputs in the accumulator registers) land in an LDS block [TR][WP], WP = 32 NOT + 4.
//           One lane per (row, head) then forms its F scores, the softmax and P V_h with plain FMAs out of that block (O takes Q's
//           place, which only that lane reads); bias, residual add and ReLU happen before the single coalesced store of Y.
//           The rows of instance i are skewed by 4 i floats so that the lanes of one wave, which read the same K / V row of
//           DIFFERENT instances at the same time, fall on different banks.
//   bwd     recomputes Q, K, V from X.  dZ = dY * (Y > 0) = dR = dO goes into the R columns of a second block G [TR][WP].
//           Pass 1, one lane per (row f, head): P's row, dP = dO_h V_h^T, D = rowsum(dP * P), dS = P (dP - D) / sqrt(dk),
//           dQ_h = dS K_h into G; (row maximum, 1 / row sum, D) into LDS.  Pass 2, one lane per (row j, head): column j of P and dS
//           from those three numbers, dK_h = dS^T Q_h and dV_h = P^T dO_h into G.  Then dX = G [Wq; Wk; Wv; Wr] (G the B operand)
//           is written once, dW += G^T X stays in registers over the workgroup's tiles, dbr is the column sum of G's R columns.
//   reduce  one thread per element of dWq | dWk | dWv | dWr | dbr adds the workgroups' partials in workgroup order.
// When the stacked weight block does not fit beside the rest in 160 KB it is staged in chunks of whole 32-row tiles.
// No float atomics anywhere: every sum has a fixed order, results are bitwise reproducible run to run.
#include "common.hpp"

namespace rc {

typedef float ai_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kAiMaxBlocks = 512;       // workgroups of the tile kernels = partials the reduce adds per element
constexpr int kAiMaxF = 32;
constexpr size_t kAiLdsBudget = 160 * 1024;
constexpr int kAiSkew = 256;            // floats behind a [TR][WP] block for the instance skew (4 floats x at most 64 instances)

struct AiGeom {       // everything derived from (F, Din, A, H) and the pass; host side, copied into the kernel arguments
  int F, d, A, H, dk, AP, DP, SX, NOT, WP, nkt;
  int TR, TI, WCT;    // tile rows, instances per tile, 32-row weight tiles staged at once
  size_t lds;
};

struct AiArgs {
  const float *X, *Wq, *Wk, *Wv, *Wr, *br;
  const float *Y, *dY;              // backward
  float *Yout;                      // forward
  float *dX, *dW_part, *db_part;    // backward
  int64_t N;
  AiGeom g;
  float scale;
};

static size_t ai_lds_bytes(const AiGeom& g, int TR, int WCT, bool bwd) {
  size_t f = (size_t)TR * g.SX + (size_t)WCT * 32 * g.SX + ((size_t)TR * g.WP + kAiSkew) * (bwd ? 2 : 1) + 128 + 64;
  if (bwd) f += (size_t)TR * g.H * 3;
  return f * sizeof(float);
}

// the tile: the largest of 128 / 64 / 32 rows that fits with the whole weight block resident; else the weight block is staged in
// chunks of whole 32-row tiles and the choice is the largest such tile height for which at least one chunk tile fits, with the
// largest chunk that fits beside it (a tall tile with a small chunk restages more often per tile than a lower one would: the
// order favours rows per tile; no shape of the MIND family is chunked).  F <= 32: a tile of 32 rows still holds an instance
static bool ai_geometry(int F, int d, int A, int H, bool bwd, AiGeom* out) {
  AiGeom g{};
  g.F = F, g.d = d, g.A = A, g.H = H, g.dk = A / H;
  g.AP = (A + 3) / 4 * 4;
  g.DP = (d + 31) / 32 * 32;
  g.SX = g.DP + 4;
  g.NOT = (4 * g.AP + 31) / 32;
  g.WP = 32 * g.NOT + 4;
  g.nkt = g.DP / 32;
  const int whole[3] = {128, 64, 32}, chunked[3] = {128, 64, 32};
  for (int TR : whole)
    if (TR >= F && ai_lds_bytes(g, TR, g.NOT, bwd) <= kAiLdsBudget) {
      g.TR = TR, g.WCT = g.NOT;
      goto found;
    }
  for (int TR : chunked)
    for (int WCT = g.NOT - 1; WCT >= 1; --WCT)
      if (TR >= F && ai_lds_bytes(g, TR, WCT, bwd) <= kAiLdsBudget) {
        g.TR = TR, g.WCT = WCT;
        goto found;
      }
  return false;
found:
  g.TI = g.TR / F;
  g.lds = ai_lds_bytes(g, g.TR, g.WCT, bwd);
  *out = g;
  return true;
}

static int ai_blocks(const AiGeom& g, int64_t N) {
  const int64_t tiles = (N + g.TI - 1) / g.TI;
  return (int)(tiles < kAiMaxBlocks ? tiles : kAiMaxBlocks);
}

// ---- device pieces -----------------------------------------------------------------------------------------------------------------
template <int CW>
struct AiVec {
  float v[CW];
};
template <int CW>
__device__ __forceinline__ AiVec<CW> ai_ld(const float* p) {
  AiVec<CW> r;
  if constexpr (CW == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <int CW>
__device__ __forceinline__ void ai_st(float* p, const AiVec<CW>& r) {
  if constexpr (CW == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else *p = r.v[0];
}
template <int CW>
__device__ __forceinline__ float ai_dot(const AiVec<CW>& a, const AiVec<CW>& b, float acc) {
#pragma unroll
  for (int u = 0; u < CW; ++u) acc = fmaf(a.v[u], b.v[u], acc);
  return acc;
}
template <int CW>
__device__ __forceinline__ void ai_axpy(float s, const AiVec<CW>& x, AiVec<CW>& y) {
#pragma unroll
  for (int u = 0; u < CW; ++u) y.v[u] = fmaf(s, x.v[u], y.v[u]);
}

// rows [32 t0, 32 (t0 + nt)) of the stacked block [Wq; Wk; Wv; Wr] (part p in rows p AP .. p AP + A, zeros elsewhere) -> ws
__device__ __forceinline__ void ai_stage_w(const AiArgs& a, float* ws, int t0, int nt, int tid) {
  const AiGeom& g = a.g;
  const int Q4 = g.DP / 4;
  for (int idx = tid; idx < nt * 32 * Q4; idx += 256) {
    const int lr = idx / Q4, c4 = idx - lr * Q4;
    const int o = 32 * t0 + lr, part = o / g.AP, ai = o - part * g.AP;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (part < 4 && ai < g.A && 4 * c4 < g.d) {
      const float* W = part == 0 ? a.Wq : part == 1 ? a.Wk : part == 2 ? a.Wv : a.Wr;
      v = *reinterpret_cast<const float4*>(W + (int64_t)ai * g.d + 4 * c4);
    }
    *reinterpret_cast<float4*>(&ws[lr * g.SX + 4 * c4]) = v;
  }
}

__device__ __forceinline__ void ai_load_x(const AiArgs& a, float* xs, int64_t row0, int rows_valid, int tid) {
  const AiGeom& g = a.g;
  const int Q4 = g.DP / 4;
  for (int idx = tid; idx < g.TR * Q4; idx += 256) {
    const int row = idx / Q4, c4 = idx - row * Q4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < rows_valid && 4 * c4 < g.d) v = load_stream4(reinterpret_cast<const float4*>(a.X + (row0 + row) * g.d + 4 * c4));
    *reinterpret_cast<float4*>(&xs[row * g.SX + 4 * c4]) = v;
  }
}

// dst[row][o] = sum_k xs[row][k] W[o][k] (+ br on the R columns) for the output tiles [0, n_ot).  A wave takes (row block, tile) pairs.
// Lane l: h = l >> 5, li = l & 31; step t: k = h DP / 2 + t on both operands, A = W[32 ot + li][k], B = X[32 rb + li][k];
// accumulator register r: dst[32 rb + li][32 ot + (r & 3) + 8 (r >> 2) + 4 h].  Ends with every wave's stores issued, not yet synced.
__device__ __forceinline__ void ai_project(const AiArgs& a, const float* xs, float* ws, float* dst, const int* rowoff, const float* bs,
                                           int n_ot, bool bias, int tid) {
  const AiGeom& g = a.g;
  const int wave = tid >> 6, lane = tid & 63, h = lane >> 5, li = lane & 31;
  const int KH = g.DP / 2, nrb = g.TR / 32;
  const bool resident = g.WCT >= g.NOT;
  for (int c0 = 0; c0 < n_ot; c0 += g.WCT) {
    const int nct = n_ot - c0 < g.WCT ? n_ot - c0 : g.WCT;
    if (!resident) {
      __syncthreads();   // every wave is done with the chunk before
      ai_stage_w(a, ws, c0, nct, tid);
      __syncthreads();
    }
    for (int p = wave; p < nrb * nct; p += 4) {
      const int rb = p % nrb, otl = p / nrb;
      const int s = 32 * rb + li;
      ai_f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float* xp = xs + s * g.SX + h * KH;
      const float* wp = ws + (32 * otl + li) * g.SX + h * KH;
#pragma unroll 2
      for (int t = 0; t < KH; t += 4) {
        const float4 x = *reinterpret_cast<const float4*>(xp + t);
        const float4 w = *reinterpret_cast<const float4*>(wp + t);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, x.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, x.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, x.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, x.w, acc, 0, 0, 0);
      }
      float* drow = dst + rowoff[s];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int o = 32 * (c0 + otl) + 8 * q + 4 * h;      // four outputs of one part (AP % 4 == 0)
        float4 v = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
        if (bias && o >= 3 * g.AP && o < 4 * g.AP) {
          const float4 b4 = *reinterpret_cast<const float4*>(&bs[o - 3 * g.AP]);
          v.x += b4.x, v.y += b4.y, v.z += b4.z, v.w += b4.w;
        }
        *reinterpret_cast<float4*>(drow + o) = v;
      }
    }
  }
}

// scores of row `ro` against the F rows of its instance (first row at `base`), head columns at hc: s[j] = <Q[ro], K[j]> (unscaled)
template <int CW>
__device__ __forceinline__ void ai_row_dots(const float* lhs, const float* rhs0, int WP, int F, int dk, float (&s)[kAiMaxF]) {
#pragma unroll
  for (int j = 0; j < kAiMaxF; ++j) s[j] = 0.f;
  for (int c = 0; c < dk; c += CW) {
    const AiVec<CW> q = ai_ld<CW>(lhs + c);
#pragma unroll
    for (int j = 0; j < kAiMaxF; ++j)
      if (j < F) s[j] = ai_dot<CW>(q, ai_ld<CW>(rhs0 + j * WP + c), s[j]);
  }
}

// p[j] = softmax_j(scale s[j]) in place; returns the row maximum and 1 / row sum
__device__ __forceinline__ void ai_softmax(float (&s)[kAiMaxF], int F, float scale, float* m_out, float* inv_out) {
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < kAiMaxF; ++j)
    if (j < F) {
      s[j] *= scale;
      m = fmaxf(m, s[j]);
    }
  float l = 0.f;
#pragma unroll
  for (int j = 0; j < kAiMaxF; ++j)
    if (j < F) {
      s[j] = expf(s[j] - m);
      l += s[j];
    }
  const float inv = 1.f / l;
#pragma unroll
  for (int j = 0; j < kAiMaxF; ++j)
    if (j < F) s[j] *= inv;
  *m_out = m, *inv_out = inv;
}

// out[c .. c + CW) = sum_j w[j] rows[j][c ..] for the head's dk columns
template <int CW>
__device__ __forceinline__ void ai_mix_rows(const float (&w)[kAiMaxF], const float* rows0, int WP, int F, int dk, float* out) {
  for (int c = 0; c < dk; c += CW) {
    AiVec<CW> acc;
#pragma unroll
    for (int u = 0; u < CW; ++u) acc.v[u] = 0.f;
#pragma unroll
    for (int j = 0; j < kAiMaxF; ++j)
      if (j < F) ai_axpy<CW>(w[j], ai_ld<CW>(rows0 + j * WP + c), acc);
    ai_st<CW>(out + c, acc);
  }
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(256) void autoint_fwd_kernel(AiArgs a) {
  const AiGeom& g = a.g;
  extern __shared__ __attribute__((aligned(16))) float ai_lds[];
  float* xs = ai_lds;                               // [TR][SX]
  float* ws = xs + g.TR * g.SX;                     // [32 WCT][SX]
  float* qs = ws + g.WCT * 32 * g.SX;               // [TR][WP] + skew: Q | K | V | R, O over Q
  int* rowoff = reinterpret_cast<int*>(qs + g.TR * g.WP + kAiSkew);   // [128]
  float* bs = reinterpret_cast<float*>(rowoff + 128);                  // [64]
  const int tid = threadIdx.x;
  const int F = g.F, A = g.A, H = g.H, dk = g.dk, AP = g.AP, WP = g.WP;
  if (tid < 128) rowoff[tid] = tid * WP + 4 * (tid / F);
  if (tid < 64) bs[tid] = tid < A ? a.br[tid] : 0.f;
  if (g.WCT >= g.NOT) ai_stage_w(a, ws, 0, g.NOT, tid);
  const int64_t ntiles = (a.N + g.TI - 1) / g.TI;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t n0 = tile * g.TI;
    const int rows_valid = (int)((a.N - n0 < g.TI ? a.N - n0 : g.TI) * F);
    __syncthreads();   // every wave is done with the previous tile's LDS (and, the first time, the tables above are written)
    ai_load_x(a, xs, n0 * F, rows_valid, tid);
    __syncthreads();
    ai_project(a, xs, ws, qs, rowoff, bs, g.NOT, true, tid);
    __syncthreads();
    for (int idx = tid; idx < rows_valid * H; idx += 256) {
      const int r = idx / H, hd = idx - r * H;
      const int i = r / F;
      const float* base = qs + rowoff[i * F] + hd * dk;
      float* qrow = qs + rowoff[r] + hd * dk;
      float p[kAiMaxF];
      ai_row_dots<CW>(qrow, base + AP, WP, F, dk, p);
      float m, inv;
      ai_softmax(p, F, a.scale, &m, &inv);
      ai_mix_rows<CW>(p, base + 2 * AP, WP, F, dk, qrow);     // O_h over Q_h: no other lane reads this row's head columns
    }
    __syncthreads();
    float* yout = a.Yout + n0 * F * A;
    if constexpr (CW == 4) {
      const int A4 = A / 4;
      for (int idx = tid; idx < rows_valid * A4; idx += 256) {
        const int r = idx / A4, c = 4 * (idx - r * A4);
        const float4 o = *reinterpret_cast<const float4*>(qs + rowoff[r] + c);
        const float4 rr = *reinterpret_cast<const float4*>(qs + rowoff[r] + 3 * AP + c);
        *reinterpret_cast<float4*>(yout + (int64_t)r * A + c) =
            make_float4(fmaxf(o.x + rr.x, 0.f), fmaxf(o.y + rr.y, 0.f), fmaxf(o.z + rr.z, 0.f), fmaxf(o.w + rr.w, 0.f));
      }
    } else {
      for (int idx = tid; idx < rows_valid * A; idx += 256) {
        const int r = idx / A, c = idx - r * A;
        yout[idx] = fmaxf(qs[rowoff[r] + c] + qs[rowoff[r] + 3 * AP + c], 0.f);
      }
    }
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(256) void autoint_bwd_kernel(AiArgs a) {
  const AiGeom& g = a.g;
  extern __shared__ __attribute__((aligned(16))) float ai_lds[];
  float* xs = ai_lds;                               // [TR][SX]
  float* ws = xs + g.TR * g.SX;                     // [32 WCT][SX]
  float* qs = ws + g.WCT * 32 * g.SX;               // [TR][WP] + skew: Q | K | V
  float* gs = qs + g.TR * g.WP + kAiSkew;           // [TR][WP] + skew: dQ | dK | dV | dZ, zero in the padding and the rows past the batch
  int* rowoff = reinterpret_cast<int*>(gs + g.TR * g.WP + kAiSkew);    // [128]
  float* bs = reinterpret_cast<float*>(rowoff + 128);                   // [64] (unused here; keeps one layout)
  float* stats = bs + 64;                                               // [TR * H][3]: row maximum, 1 / row sum, D
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, li = lane & 31;
  const int F = g.F, A = g.A, H = g.H, dk = g.dk, AP = g.AP, WP = g.WP, d = g.d, SX = g.SX;
  const int nrb = g.TR / 32, nkt = g.nkt, NOT = g.NOT;
  const bool resident = g.WCT >= NOT;
  if (tid < 128) rowoff[tid] = tid * WP + 4 * (tid / F);
  if (resident) ai_stage_w(a, ws, 0, NOT, tid);

  ai_f32x16 dwacc[8];      // dW tiles (ot, kt), tile index = wave + 4 j
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) dwacc[j][r] = 0.f;
  float dbacc = 0.f;

  const int64_t ntiles = (a.N + g.TI - 1) / g.TI;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t n0 = tile * g.TI;
    const int rows_valid = (int)((a.N - n0 < g.TI ? a.N - n0 : g.TI) * F);
    __syncthreads();
    ai_load_x(a, xs, n0 * F, rows_valid, tid);
    {   // G: dZ = dY * (Y > 0) in the R columns of the batch's rows, zeros everywhere else
      const float* yin = a.Y + n0 * F * A;
      const float* dyin = a.dY + n0 * F * A;
      const int W4 = 8 * NOT;
      for (int idx = tid; idx < g.TR * W4; idx += 256) {
        const int r = idx / W4, c = 4 * (idx - r * W4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const int ca = c - 3 * AP;
        if (r < rows_valid && ca >= 0 && ca < A) {
          if constexpr (CW == 4) {
            const float4 y = *reinterpret_cast<const float4*>(yin + (int64_t)r * A + ca);
            const float4 dy = load_stream4(reinterpret_cast<const float4*>(dyin + (int64_t)r * A + ca));
            v = make_float4(y.x > 0.f ? dy.x : 0.f, y.y > 0.f ? dy.y : 0.f, y.z > 0.f ? dy.z : 0.f, y.w > 0.f ? dy.w : 0.f);
          } else {
            float t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
              t[u] = (ca + u < A && yin[(int64_t)r * A + ca + u] > 0.f) ? dyin[(int64_t)r * A + ca + u] : 0.f;
            v = make_float4(t[0], t[1], t[2], t[3]);
          }
        }
        *reinterpret_cast<float4*>(gs + rowoff[r] + c) = v;
      }
    }
    __syncthreads();
    ai_project(a, xs, ws, qs, rowoff, bs, (3 * AP + 31) / 32, false, tid);
    __syncthreads();

    // ---- pass 1: one lane per (row f, head): dQ_h, and (m, 1 / l, D) for pass 2
    for (int idx = tid; idx < rows_valid * H; idx += 256) {
      const int r = idx / H, hd = idx - r * H;
      const int i = r / F;
      const int boff = rowoff[i * F] + hd * dk, roff = rowoff[r] + hd * dk;
      float p[kAiMaxF], dp[kAiMaxF];
      ai_row_dots<CW>(qs + roff, qs + boff + AP, WP, F, dk, p);
      float m, inv;
      ai_softmax(p, F, a.scale, &m, &inv);
      ai_row_dots<CW>(gs + roff + 3 * AP, qs + boff + 2 * AP, WP, F, dk, dp);     // dP[j] = <dO[f], V[j]>
      float D = 0.f;
#pragma unroll
      for (int j = 0; j < kAiMaxF; ++j)
        if (j < F) D = fmaf(p[j], dp[j], D);
#pragma unroll
      for (int j = 0; j < kAiMaxF; ++j)
        if (j < F) dp[j] = p[j] * (dp[j] - D) * a.scale;                          // dS[f][j] / sqrt(dk)
      stats[3 * idx] = m, stats[3 * idx + 1] = inv, stats[3 * idx + 2] = D;
      ai_mix_rows<CW>(dp, qs + boff + AP, WP, F, dk, gs + roff);                   // dQ[f] = sum_j dS[f][j] K[j]
    }
    __syncthreads();
    // ---- pass 2: one lane per (row j, head): column j of P and dS -> dK_h, dV_h
    for (int idx = tid; idx < rows_valid * H; idx += 256) {
      const int r = idx / H, hd = idx - r * H;
      const int i = r / F;
      const int boff = rowoff[i * F] + hd * dk, roff = rowoff[r] + hd * dk;
      float pc[kAiMaxF], ds[kAiMaxF];
      // pc[f] = <Q[f], K[j]>, ds[f] = <dO[f], V[j]>: the operands in pass 1's order, so the scores repeat bit for bit
#pragma unroll
      for (int f = 0; f < kAiMaxF; ++f) pc[f] = 0.f, ds[f] = 0.f;
      for (int c = 0; c < dk; c += CW) {
        const AiVec<CW> kv = ai_ld<CW>(qs + roff + AP + c), vv = ai_ld<CW>(qs + roff + 2 * AP + c);
#pragma unroll
        for (int f = 0; f < kAiMaxF; ++f)
          if (f < F) {
            pc[f] = ai_dot<CW>(ai_ld<CW>(qs + boff + f * WP + c), kv, pc[f]);
            ds[f] = ai_dot<CW>(ai_ld<CW>(gs + boff + 3 * AP + f * WP + c), vv, ds[f]);
          }
      }
      const float* st = stats + 3 * ((i * F) * H + hd);
#pragma unroll
      for (int f = 0; f < kAiMaxF; ++f)
        if (f < F) {
          const float pf = expf(pc[f] * a.scale - st[3 * f * H]) * st[3 * f * H + 1];
          ds[f] = pf * (ds[f] - st[3 * f * H + 2]) * a.scale;
          pc[f] = pf;
        }
      ai_mix_rows<CW>(ds, qs + boff, WP, F, dk, gs + roff + AP);                   // dK[j] = sum_f dS[f][j] Q[f]
      ai_mix_rows<CW>(pc, gs + boff + 3 * AP, WP, F, dk, gs + roff + 2 * AP);      // dV[j] = sum_f P[f][j] dO[f]
    }
    __syncthreads();

    // ---- dX = G [Wq; Wk; Wv; Wr]: a wave takes (row block, 32-wide k tile) pairs, pair index = wave + 4 jj.  Steps of 8 stacked
    // outputs: lane half h contracts o0 + 4 h + u; A = W[o][32 kt + li], B = G[32 rb + li][o]; register r: dX[row][32 kt + jr(r, h)]
    {
      ai_f32x16 dxa[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int r = 0; r < 16; ++r) dxa[jj][r] = 0.f;
      for (int c0 = 0; c0 < NOT; c0 += g.WCT) {
        const int nct = NOT - c0 < g.WCT ? NOT - c0 : g.WCT;
        if (!resident) {
          __syncthreads();
          ai_stage_w(a, ws, c0, nct, tid);
          __syncthreads();
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int p = wave + 4 * jj;
          if (p < nrb * nkt) {     // (wave-uniform)
            const int rb = p % nrb, kt = p / nrb;
            const float* grow = gs + rowoff[32 * rb + li] + 32 * c0 + 4 * h;
            const float* wcol = ws + (4 * h) * SX + 32 * kt + li;
            for (int o0 = 0; o0 < 32 * nct; o0 += 8) {
              const float4 gv = *reinterpret_cast<const float4*>(grow + o0);
              dxa[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(wcol[(o0 + 0) * SX], gv.x, dxa[jj], 0, 0, 0);
              dxa[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(wcol[(o0 + 1) * SX], gv.y, dxa[jj], 0, 0, 0);
              dxa[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(wcol[(o0 + 2) * SX], gv.z, dxa[jj], 0, 0, 0);
              dxa[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(wcol[(o0 + 3) * SX], gv.w, dxa[jj], 0, 0, 0);
            }
          }
        }
      }
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int p = wave + 4 * jj;
        if (p < nrb * nkt) {
          const int rb = p % nrb, kt = p / nrb;
          const int s = 32 * rb + li;
          float* dxrow = a.dX + (n0 * F + s) * d;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int k = 32 * kt + 8 * q + 4 * h;
            if (s < rows_valid && k < d)
              *reinterpret_cast<float4*>(dxrow + k) = make_float4(dxa[jj][4 * q], dxa[jj][4 * q + 1], dxa[jj][4 * q + 2], dxa[jj][4 * q + 3]);
          }
        }
      }
    }
    // ---- dW += G^T X over the tile's rows: step t contracts row 2 t + h; A = G[row][32 ot + li], B = X[row][32 kt + li];
    // register r: dW[32 ot + jr(r, h)][32 kt + li].  dbr += column sums of G's R columns
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int idx = wave + 4 * j;
      if (idx < NOT * nkt) {   // (wave-uniform)
        const int ot = idx / nkt, kt = idx - ot * nkt;
#pragma unroll 4
        for (int t = 0; t < g.TR / 2; ++t) {
          const int row = 2 * t + h;
          dwacc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(gs[rowoff[row] + 32 * ot + li], xs[row * SX + 32 * kt + li], dwacc[j], 0, 0, 0);
        }
      }
    }
    if (tid < A)
      for (int row = 0; row < rows_valid; ++row) dbacc += gs[rowoff[row] + 3 * AP + tid];
  }

  float* dWp = a.dW_part + (int64_t)blockIdx.x * 4 * A * d;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = wave + 4 * j;
    if (idx < NOT * nkt) {
      const int ot = idx / nkt, kt = idx - ot * nkt;
      const int k = 32 * kt + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = 32 * ot + (r & 3) + 8 * (r >> 2) + 4 * h;
        const int part = o / AP, ai = o - part * AP;
        if (part < 4 && ai < A && k < d) dWp[(part * A + ai) * d + k] = dwacc[j][r];
      }
    }
  }
  if (tid < A) a.db_part[(int64_t)blockIdx.x * A + tid] = dbacc;
}

// one thread per element of dWq | dWk | dWv | dWr | dbr: the workgroups' partials in workgroup order, in double
__global__ __launch_bounds__(kBlock) void autoint_grad_reduce_kernel(const float* __restrict__ dW_part, const float* __restrict__ db_part,
                                                                     int blocks, int A, int d, float* __restrict__ dWq,
                                                                     float* __restrict__ dWk, float* __restrict__ dWv,
                                                                     float* __restrict__ dWr, float* __restrict__ dbr) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  const int nW = A * d;
  if (e >= 4 * nW + A) return;
  const bool isW = e < 4 * nW;
  const float* src = isW ? dW_part + e : db_part + (e - 4 * nW);
  const int64_t stride = isW ? 4 * nW : A;
  double acc = 0.0;
  for (int p = 0; p < blocks; ++p) acc += (double)src[p * stride];
  if (!isW) {
    dbr[e - 4 * nW] = (float)acc;
    return;
  }
  const int part = e / nW, rest = e - part * nW;
  float* dst = part == 0 ? dWq : part == 1 ? dWk : part == 2 ? dWv : dWr;
  dst[rest] = (float)acc;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
// the one statement of the envelope: every entry point checks it, rc_autoint_check_shape reports it to the host
static int ai_shape(const char* fn, int F, int d, int A, int H) {
  if (F >= 2 && F <= kAiMaxF && d % 4 == 0 && d >= 4 && d <= 128 && A >= 4 && A <= 64 && H >= 1 && H <= A && A % H == 0) return RC_OK;
  return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (fields in [2, 32], input width a multiple of 4 in [4, 128], attention_size in "
              "[4, 64], num_heads a divisor of attention_size): fields=%d width=%d attention_size=%d num_heads=%d", fn, F, d, A, H);
}

static int ai_check(const char* fn, int64_t N, int F, int d, int A, int H, bool bwd, AiGeom* g) {
  RC_TRY(ai_shape(fn, F, d, A, H));
  if (N < 1 || N > ((int64_t)1 << 24))
    return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (instances in [1, 2^24]): instances=%lld", fn, (long long)N);
  if (!ai_geometry(F, d, A, H, bwd, g)) return fail(RC_ERR_UNSUPPORTED, "%s: no tile fits the LDS for this shape", fn);
  return RC_OK;
}

template <int CW>
static int ai_launch(const AiArgs& a, bool bwd, int blocks, hipStream_t st) {
  auto kern = bwd ? autoint_bwd_kernel<CW> : autoint_fwd_kernel<CW>;
  RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.g.lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), a.g.lds, st, a);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

static int ai_run(const AiArgs& a, bool bwd, int blocks, hipStream_t st) {
  return a.g.dk % 4 == 0 ? ai_launch<4>(a, bwd, blocks, st) : ai_launch<1>(a, bwd, blocks, st);
}

}  // namespace rc

extern "C" int rc_autoint_check_shape(int n_fields, int d_in, int attention_size, int num_heads) {
  using namespace rc;
  const char* fn = "rc_autoint_check_shape";
  RC_TRY(ai_shape(fn, n_fields, d_in, attention_size, num_heads));
  AiGeom g;
  if (!ai_geometry(n_fields, d_in, attention_size, num_heads, true, &g) || !ai_geometry(n_fields, d_in, attention_size, num_heads, false, &g))
    return fail(RC_ERR_UNSUPPORTED, "%s: no tile fits the LDS for this shape", fn);
  return RC_OK;
}

extern "C" size_t rc_autoint_workspace_bytes(int64_t n_instances, int n_fields, int d_in, int attention_size, int num_heads) {
  using namespace rc;
  AiGeom g;
  if (ai_check("rc_autoint_workspace_bytes", n_instances, n_fields, d_in, attention_size, num_heads, true, &g) != RC_OK) return 0;
  const int blocks = ai_blocks(g, n_instances);
  Carver c(nullptr);
  c.take<float>((size_t)blocks * 4 * attention_size * d_in);
  c.take<float>((size_t)blocks * attention_size);
  return c.off;
}

extern "C" int rc_autoint_layer_fwd(const float* X, const float* Wq, const float* Wk, const float* Wv, const float* Wr, const float* br,
                                    int64_t n_instances, int n_fields, int d_in, int attention_size, int num_heads, float* Y,
                                    rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_autoint_layer_fwd";
  AiGeom g;
  RC_TRY(ai_check(fn, n_instances, n_fields, d_in, attention_size, num_heads, false, &g));
  RC_REQUIRE(X != nullptr && Wq != nullptr && Wk != nullptr && Wv != nullptr && Wr != nullptr && br != nullptr && Y != nullptr,
             "%s: null pointer", fn);
  RC_REQUIRE(aligned16(X, Wq, Wk, Wv, Wr, Y), "%s: X, the weights and Y must be 16-byte aligned", fn);
  AiArgs a{X, Wq, Wk, Wv, Wr, br, nullptr, nullptr, Y, nullptr, nullptr, nullptr, n_instances, g, 1.f / sqrtf((float)g.dk)};
  return ai_run(a, false, ai_blocks(g, n_instances), as_stream(stream));
}

extern "C" int rc_autoint_layer_bwd(const float* X, const float* Wq, const float* Wk, const float* Wv, const float* Wr, const float* Y,
                                    const float* dY, int64_t n_instances, int n_fields, int d_in, int attention_size, int num_heads,
                                    void* workspace, size_t ws_bytes, float* dX, float* dWq, float* dWk, float* dWv, float* dWr,
                                    float* dbr, rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_autoint_layer_bwd";
  AiGeom g;
  RC_TRY(ai_check(fn, n_instances, n_fields, d_in, attention_size, num_heads, true, &g));
  RC_REQUIRE(X != nullptr && Wq != nullptr && Wk != nullptr && Wv != nullptr && Wr != nullptr && Y != nullptr && dY != nullptr &&
             dX != nullptr && dWq != nullptr && dWk != nullptr && dWv != nullptr && dWr != nullptr && dbr != nullptr, "%s: null pointer", fn);
  RC_REQUIRE(aligned16(X, Wq, Wk, Wv, Wr, Y, dY, dX), "%s: X, the weights, Y, dY and dX must be 16-byte aligned", fn);
  RC_REQUIRE(workspace != nullptr && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "%s: workspace must be 256-byte aligned", fn);
  const int blocks = ai_blocks(g, n_instances);
  Carver c(workspace);
  float* dW_part = c.take<float>((size_t)blocks * 4 * attention_size * d_in);
  float* db_part = c.take<float>((size_t)blocks * attention_size);
  if (ws_bytes < c.off) return fail(RC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, c.off);
  const hipStream_t st = as_stream(stream);
  AiArgs a{X, Wq, Wk, Wv, Wr, nullptr, Y, dY, nullptr, dX, dW_part, db_part, n_instances, g, 1.f / sqrtf((float)g.dk)};
  RC_TRY(ai_run(a, true, blocks, st));
  const int n = 4 * attention_size * d_in + attention_size;
  hipLaunchKernelGGL(autoint_grad_reduce_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dW_part, db_part, blocks,
                     attention_size, d_in, dWq, dWk, dWv, dWr, dbr);
  RC_LAUNCH_CHECK();
  return RC_OK;
}
