// contrarec.hip -- ContraRec's context-context contrastive loss  (reference: models/sequential/ContraRec.py:142-193 ContraLoss;
// the forward-indexed position embedding of its BERT4Rec encoder is rc_seq_embed_fwdpos_fwd / rc_seq_pos_grad_fwdpos in seq_layers.hip)
//
// The two views' encoder outputs va, vb [B, d] are stacked view-major (rows 0..B-1 view a, B..2B-1 view b: the reference's
// torch.cat(torch.unbind(features, 1))), N = 2B.  z_r = x_r / max(|x_r|, 1e-12), l_rc = z_r . z_c / t,
// pos_rc = [label(r mod B) == label(c mod B)] and c != r  (labels NULL: label = the sample index, InfoNCE):
//   m_r  = max_c l_rc  (diagonal included)         D_r = sum_{c != r} exp(l_rc - m_r) + 1e-10
//   P_r  = sum_c pos_rc                            A_r = sum_c pos_rc l_rc
//   loss = -(t / N) sum_r (A_r - P_r (m_r + log D_r)) / (P_r + 1e-10)
//   dz_r = -(1 / N) sum_{c != r} [pos_rc (a_r + a_c) - b_r exp(l_rc - lz_r) - b_c exp(l_rc - lz_c)] z_c
//          a_r = 1 / (P_r + 1e-10),  b_r = P_r a_r,  lz_r = m_r + log D_r
// Launches (forward): rows (normalise), stats sweep, finish (chunks combined, row terms), reduce (double, one workgroup).
// Backward: weight sweep, rows (chunks combined, back through the normalisation).  Both sweeps are owner-computes on
// v_mfma_f32_32x32x2_f32 with the operand layout of directau.hip: a wave owns 32 rows, the workgroup stages 32-row column blocks
// in LDS, the Gram tile G' = Z_cols Z_own^T has the column-block rows in the accumulator registers and the owned rows on the
// lanes.  The stats sweep keeps (m, D, A, P) per lane with an online maximum; the weight sweep turns the accumulator into the
// weight tile (lz, a, b of the column side staged beside the block, label equality evaluated from the two label vectors) and
// feeds it back as the B operand of G^T += Z_cols^T W'.  Large N is split into column chunks whose partials are combined in
// chunk order.  The N x N matrix is never stored, there are no float atomics, every sum has a fixed order: reruns are bitwise
// identical.
#include "common.hpp"

namespace rc {

typedef float con_f32x16 __attribute__((ext_vector_type(16)));

constexpr float kConEps = 1e-12f;      // F.normalize's default eps
constexpr float kConTiny = 1e-10f;     // the reference's guard of log(.) and of the positive count
constexpr int kConRowsPerWave = 32;
constexpr int kConRowsPerBlock = 128;
constexpr int kConTargetBlocks = 512;
constexpr int kConMaxChunks = 16;

struct ConLayout {   // the workspace, carved in this order
  int64_t B, N;
  int d, chunks, per_chunk;
  int64_t ncb;       // 32-row column blocks of the N stacked rows
  float* z;          // [N][d]
  float* den;        // [N]          max(|x|, eps)
  float* pm;         // [chunks][N]  per-chunk maximum
  float* pD;         // [chunks][N]  per-chunk sum of exp(l - pm), diagonal excluded
  float* pA;         // [chunks][N]  per-chunk sum of the positives' logits
  float* pP;         // [chunks][N]  per-chunk count of positives (exact in fp32: at most 2^20)
  float* lz;         // [N]          m + log D
  float* ca;         // [N]          1 / (P + 1e-10)
  float* cb;         // [N]          P / (P + 1e-10)
  float* term;       // [N]          (A - P lz) / (P + 1e-10)
  float* G;          // [chunks][N][d]  sum_c w_rc z_c of the chunk's columns
  size_t bytes;
};

static ConLayout con_layout(int d, int64_t B, void* base) {
  ConLayout L{};
  L.B = B;
  L.N = 2 * B;
  L.d = d;
  const int64_t ncb = (L.N + 31) / 32;
  L.ncb = ncb;
  const int64_t nwg = (L.N + kConRowsPerBlock - 1) / kConRowsPerBlock;
  int64_t want = (kConTargetBlocks + nwg - 1) / nwg;
  if (want > kConMaxChunks) want = kConMaxChunks;
  if (want > ncb) want = ncb;
  if (want < 1) want = 1;
  const int64_t per = (ncb + want - 1) / want;
  L.per_chunk = (int)per;
  L.chunks = (int)((ncb + per - 1) / per);
  Carver c(base);
  const size_t N = (size_t)L.N;
  L.z = c.take<float>(N * d);
  L.den = c.take<float>(N);
  L.pm = c.take<float>((size_t)L.chunks * N);
  L.pD = c.take<float>((size_t)L.chunks * N);
  L.pA = c.take<float>((size_t)L.chunks * N);
  L.pP = c.take<float>((size_t)L.chunks * N);
  L.lz = c.take<float>(N);
  L.ca = c.take<float>(N);
  L.cb = c.take<float>(N);
  L.term = c.take<float>(N);
  L.G = c.take<float>((size_t)L.chunks * N * d);
  L.bytes = c.off;
  return L;
}

template <int LPR>
__device__ __forceinline__ float con_group_sum(float x) {   // butterfly inside a lane group: every lane gets the same bits
#pragma unroll
  for (int off = LPR / 2; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

__device__ __forceinline__ float con_dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// label of stacked row j (both views of sample j mod B carry the sample's label; no labels: the sample index)
__device__ __forceinline__ int64_t con_label(const int64_t* __restrict__ labels, int64_t j, int64_t B) {
  const int64_t s = j < B ? j : j - B;
  return labels != nullptr ? labels[s] : s;
}

// ---- rows: LPR lanes per row (float4 each), 64 / LPR rows per wave ------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(kBlock) void con_rows_kernel(const float* __restrict__ va, const float* __restrict__ vb, ConLayout L) {
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int l = lane % LPR;
  const int d = L.d;
  const bool on = 4 * l < d;
  const int64_t stride = (int64_t)gridDim.x * (kBlock / 64) * G;
  for (int64_t r = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * G + lane / LPR; r < L.N; r += stride) {
    const float* src = r < L.B ? va + r * d : vb + (r - L.B) * d;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) x = *reinterpret_cast<const float4*>(src + 4 * l);
    const float den = fmaxf(sqrtf(con_group_sum<LPR>(con_dot4(x, x))), kConEps);
    if (on) *reinterpret_cast<float4*>(L.z + r * d + 4 * l) = make_float4(x.x / den, x.y / den, x.z / den, x.w / den);
    if (l == 0) L.den[r] = den;
  }
}

// ---- the two sweeps -----------------------------------------------------------------------------------------------------------
// grid (ceil(N / 128), chunks), 256 threads.  DP = d rounded up to a multiple of 32 (zero padded in LDS and registers).
// Lane l of wave w: h = l >> 5, owned row i = 128 blockIdx.x + 32 w + (l & 31).
//   Gram step t (t < DP / 2): k = h DP / 2 + t on both operands; A = Z_cols[l & 31][k] (LDS), B = Z_own[i][k] (registers)
//   accumulator register r of lane l: column-block row jr(r, h) = (r & 3) + 8 (r >> 2) + 4 h, owned row i
//   G^T tile ct, step r: A = Z_cols[jr(r, h)][32 ct + (l & 31)] (LDS), B = w[r] (k = jr(r, h) on both operands);
//   its register r of lane l holds G^T[32 ct + jr(r, h)][i]
template <int DP>
struct ConTile {
  static constexpr int SR = DP + 4;    // LDS row stride (floats)
  static constexpr int KH = DP / 2;    // k per lane half
  static constexpr int NL = DP / 32;   // float4 staged per thread per column block (32 rows x DP floats / 256 threads)

  static __device__ __forceinline__ void fetch(const float* __restrict__ Z, int64_t N, int d, int64_t cb, float4 (&pre)[NL]) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int idx = threadIdx.x + q * 256;
      const int row = idx / (DP / 4), c4 = idx % (DP / 4);
      const int64_t j = cb * 32 + row;
      pre[q] = (j < N && 4 * c4 < d) ? *reinterpret_cast<const float4*>(Z + j * d + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  static __device__ __forceinline__ void stage(float* xs, const float4 (&pre)[NL]) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int idx = threadIdx.x + q * 256;
      const int row = idx / (DP / 4), c4 = idx % (DP / 4);
      *reinterpret_cast<float4*>(&xs[row * SR + 4 * c4]) = pre[q];
    }
  }
  static __device__ __forceinline__ void own(const float* __restrict__ Z, int64_t i, bool iv, int d, int h, float (&breg)[KH]) {
#pragma unroll
    for (int t = 0; t < KH; ++t) {
      const int k = h * KH + t;
      breg[t] = (iv && k < d) ? Z[i * d + k] : 0.f;
    }
  }
  static __device__ __forceinline__ con_f32x16 gram(const float* xs, const float (&breg)[KH], int li, int h) {
    con_f32x16 g;
#pragma unroll
    for (int r = 0; r < 16; ++r) g[r] = 0.f;
#pragma unroll
    for (int t = 0; t < KH; t += 4) {
      const float4 a = *reinterpret_cast<const float4*>(&xs[li * SR + h * KH + t]);
      g = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, breg[t + 0], g, 0, 0, 0);
      g = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, breg[t + 1], g, 0, 0, 0);
      g = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, breg[t + 2], g, 0, 0, 0);
      g = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, breg[t + 3], g, 0, 0, 0);
    }
    return g;
  }
};

// first sweep: per owned row the chunk's (maximum, sum of exp, sum of the positives' logits, count of positives)
template <int DP>
__global__ __launch_bounds__(256) void con_stats_kernel(ConLayout L, const int64_t* __restrict__ labels, float inv_t) {
  using T = ConTile<DP>;
  const int64_t N = L.N, B = L.B;
  const int d = L.d;
  const int chunk = blockIdx.y;
  __shared__ __attribute__((aligned(16))) float xs[32 * T::SR];
  __shared__ int64_t labs[32];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31;
  const int64_t i = (int64_t)blockIdx.x * kConRowsPerBlock + wave * kConRowsPerWave + li;
  const bool iv = i < N;
  float breg[T::KH];
  T::own(L.z, i, iv, d, h, breg);
  const int64_t lab_i = iv ? con_label(labels, i, B) : 0;
  float m = -INFINITY, D = 0.f, A = 0.f, P = 0.f;

  const int64_t cb0 = (int64_t)chunk * L.per_chunk;
  const int64_t cb1 = cb0 + L.per_chunk < L.ncb ? cb0 + L.per_chunk : L.ncb;
  float4 pre[T::NL];
  if (cb0 < cb1) T::fetch(L.z, N, d, cb0, pre);
  for (int64_t cb = cb0; cb < cb1; ++cb) {
    __syncthreads();   // every wave is done with the previous block
    T::stage(xs, pre);
    if (threadIdx.x < 32) {
      const int64_t j = cb * 32 + threadIdx.x;
      labs[threadIdx.x] = j < N ? con_label(labels, j, B) : 0;
    }
    __syncthreads();
    if (cb + 1 < cb1) T::fetch(L.z, N, d, cb + 1, pre);   // the next block, while this one is computed
    con_f32x16 g = T::gram(xs, breg, li, h);
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jr = (r & 3) + 8 * (r >> 2) + 4 * h;
      g[r] *= inv_t;
      if (cb * 32 + jr < N) tmax = fmaxf(tmax, g[r]);
    }
    if (tmax > m) {   // online maximum (m = -inf before the first valid column: D is still 0)
      D *= expf(m - tmax);
      m = tmax;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jr = (r & 3) + 8 * (r >> 2) + 4 * h;
      const int64_t j = cb * 32 + jr;
      if (j < N && j != i) {
        D += expf(g[r] - m);
        if (labs[jr] == lab_i) {
          A += g[r];
          P += 1.f;
        }
      }
    }
  }
  // the two lane halves hold the two halves of every column block
  const float mo = __shfl_xor(m, 32, 64), Do = __shfl_xor(D, 32, 64), Ao = __shfl_xor(A, 32, 64), Po = __shfl_xor(P, 32, 64);
  const float mm = fmaxf(m, mo);
  const float lo_m = h == 0 ? m : mo, lo_D = h == 0 ? D : Do, hi_m = h == 0 ? mo : m, hi_D = h == 0 ? Do : D;
  const float DD = (lo_D > 0.f ? lo_D * expf(lo_m - mm) : 0.f) + (hi_D > 0.f ? hi_D * expf(hi_m - mm) : 0.f);
  if (iv && h == 0) {
    const int64_t at = (int64_t)chunk * N + i;
    L.pm[at] = mm;
    L.pD[at] = DD;
    L.pA[at] = A + Ao;
    L.pP[at] = P + Po;
  }
}

// chunk partials in chunk order -> lz, a, b and the row's term of the loss
__global__ __launch_bounds__(kBlock) void con_finish_kernel(ConLayout L) {
  const int64_t N = L.N;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < N; r += (int64_t)gridDim.x * kBlock) {
    float m = -INFINITY;
    for (int c = 0; c < L.chunks; ++c) m = fmaxf(m, L.pm[(int64_t)c * N + r]);
    float D = 0.f, A = 0.f, P = 0.f;
    for (int c = 0; c < L.chunks; ++c) {
      const float Dc = L.pD[(int64_t)c * N + r];
      if (Dc > 0.f) D += Dc * expf(L.pm[(int64_t)c * N + r] - m);
      A += L.pA[(int64_t)c * N + r];
      P += L.pP[(int64_t)c * N + r];
    }
    D += kConTiny;
    const float lz = m + logf(D);
    const float a = 1.f / (P + kConTiny);
    L.lz[r] = lz;
    L.ca[r] = a;
    L.cb[r] = P * a;
    L.term[r] = (float)(((double)A - (double)P * (double)lz) * (double)a);
  }
}

// one workgroup, double, fixed order: loss = -(t / N) sum_r term_r
__global__ __launch_bounds__(kBlock) void con_reduce_kernel(ConLayout L, float t, float* __restrict__ out) {
  __shared__ double red[kBlock];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int64_t r = tid; r < L.N; r += kBlock) a += (double)L.term[r];
  red[tid] = a;
  __syncthreads();
  for (int w = kBlock / 2; w >= 1; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) out[0] = (float)(-(double)t * red[0] / (double)L.N);
}

// second sweep: G_i = sum_{c != i} w_ic z_c over the chunk's columns, the weight tile straight from the accumulator
template <int DP>
__global__ __launch_bounds__(256) void con_weight_kernel(ConLayout L, const int64_t* __restrict__ labels, float inv_t) {
  using T = ConTile<DP>;
  constexpr int NCT = DP / 32;
  const int64_t N = L.N, B = L.B;
  const int d = L.d;
  const int chunk = blockIdx.y;
  __shared__ __attribute__((aligned(16))) float xs[32 * T::SR];
  __shared__ int64_t labs[32];
  __shared__ float lzs[32], cas[32], cbs[32];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31;
  const int64_t i = (int64_t)blockIdx.x * kConRowsPerBlock + wave * kConRowsPerWave + li;
  const bool iv = i < N;
  float breg[T::KH];
  T::own(L.z, i, iv, d, h, breg);
  const int64_t lab_i = iv ? con_label(labels, i, B) : 0;
  const float lz_i = iv ? L.lz[i] : 0.f, ca_i = iv ? L.ca[i] : 0.f, cb_i = iv ? L.cb[i] : 0.f;
  con_f32x16 acc[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;

  const int64_t cb0 = (int64_t)chunk * L.per_chunk;
  const int64_t cb1 = cb0 + L.per_chunk < L.ncb ? cb0 + L.per_chunk : L.ncb;
  float4 pre[T::NL];
  if (cb0 < cb1) T::fetch(L.z, N, d, cb0, pre);
  for (int64_t cb = cb0; cb < cb1; ++cb) {
    __syncthreads();
    T::stage(xs, pre);
    if (threadIdx.x < 32) {
      const int64_t j = cb * 32 + threadIdx.x;
      const bool jv = j < N;
      labs[threadIdx.x] = jv ? con_label(labels, j, B) : 0;
      lzs[threadIdx.x] = jv ? L.lz[j] : 0.f;
      cas[threadIdx.x] = jv ? L.ca[j] : 0.f;
      cbs[threadIdx.x] = jv ? L.cb[j] : 0.f;
    }
    __syncthreads();
    if (cb + 1 < cb1) T::fetch(L.z, N, d, cb + 1, pre);
    con_f32x16 g = T::gram(xs, breg, li, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jr = (r & 3) + 8 * (r >> 2) + 4 * h;
      const int64_t j = cb * 32 + jr;
      const float l = g[r] * inv_t;
      float w = 0.f;
      if (iv && j < N && j != i) {
        // p_rc = exp(l - lz_r) <= 1 and p_cr = exp(l - lz_c) <= 1: each row's D holds this very term
        w = (labs[jr] == lab_i ? ca_i + cas[jr] : 0.f) - cb_i * expf(l - lz_i) - cbs[jr] * expf(l - lzs[jr]);
      }
      g[r] = w;
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jr = (r & 3) + 8 * (r >> 2) + 4 * h;
        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[jr * T::SR + 32 * ct + li], g[r], acc[ct], 0, 0, 0);
      }
    }
  }
  if (iv) {
    float* Gi = L.G + ((int64_t)chunk * N + i) * d;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * ct + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (c < d) Gi[c] = acc[ct][r];
      }
  }
}

// ---- backward rows: chunks in chunk order, dz = -(g / N) G, back through F.normalize ------------------------------------------
template <int LPR>
__global__ __launch_bounds__(kBlock) void con_bwd_rows_kernel(ConLayout L, const float* __restrict__ gloss, float* __restrict__ dva,
                                                              float* __restrict__ dvb) {
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int l = lane % LPR;
  const int d = L.d;
  const bool on = 4 * l < d;
  const float s = -gloss[0] / (float)L.N;
  const int64_t stride = (int64_t)gridDim.x * (kBlock / 64) * G;
  for (int64_t r = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * G + lane / LPR; r < L.N; r += stride) {
    float4 z = make_float4(0.f, 0.f, 0.f, 0.f), g = z;
    if (on) {
      z = *reinterpret_cast<const float4*>(L.z + r * d + 4 * l);
      for (int c = 0; c < L.chunks; ++c) {
        const float4 a = *reinterpret_cast<const float4*>(L.G + ((int64_t)c * L.N + r) * d + 4 * l);
        g = make_float4(g.x + a.x, g.y + a.y, g.z + a.z, g.w + a.w);
      }
    }
    g = make_float4(s * g.x, s * g.y, s * g.z, s * g.w);
    // F.normalize's backward: past eps (g - z (z . g)) / |x|, else g / eps (den = max(|x|, eps))
    const float den = L.den[r];
    float4 o;
    if (den > kConEps) {
      const float p = con_group_sum<LPR>(con_dot4(z, g));
      o = make_float4((g.x - z.x * p) / den, (g.y - z.y * p) / den, (g.z - z.z * p) / den, (g.w - z.w * p) / den);
    } else {
      o = make_float4(g.x / kConEps, g.y / kConEps, g.z / kConEps, g.w / kConEps);
    }
    if (on) {
      float* dst = r < L.B ? dva + r * d : dvb + (r - L.B) * d;
      *reinterpret_cast<float4*>(dst + 4 * l) = o;
    }
  }
}

static unsigned con_row_grid(int64_t N, int lpr) {
  const int64_t rows_per_block = (kBlock / 64) * (64 / lpr);
  int64_t blocks = (N + rows_per_block - 1) / rows_per_block;
  if (blocks < 1) blocks = 1;
  if (blocks > 65536) blocks = 65536;
  return (unsigned)blocks;
}

static int con_lpr(int d) {
  const int dq = d / 4;
  int lpr = 1;
  while (lpr < dq) lpr <<= 1;
  return lpr;
}

#define CON_LPR_SWITCH(lpr, F) \
  switch (lpr) {               \
    case 1: F(1); break;       \
    case 2: F(2); break;       \
    case 4: F(4); break;       \
    case 8: F(8); break;       \
    case 16: F(16); break;     \
    case 32: F(32); break;     \
    default: F(64); break;     \
  }

#define CON_DP_SWITCH(dp, F) \
  switch (dp) {              \
    case 32: F(32); break;   \
    case 64: F(64); break;   \
    case 96: F(96); break;   \
    case 128: F(128); break; \
    case 160: F(160); break; \
    case 192: F(192); break; \
    case 224: F(224); break; \
    default: F(256); break;  \
  }

// the one statement of the envelope: every entry point checks it, rc_contra_check_shape reports it to the host
static int con_shape(const char* fn, int d, int64_t B) {
  if (d % 4 == 0 && d >= 4 && d <= 256 && B >= 1 && B <= ((int64_t)1 << 19)) return RC_OK;
  return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (emb_size a multiple of 4 in [4, 256], batch in [1, 524288]): "
              "emb_size=%d batch=%lld", fn, d, (long long)B);
}

static bool con_aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

static int con_workspace_check(const char* fn, int d, int64_t B, const void* ws, size_t ws_bytes, ConLayout* L) {
  RC_TRY(con_shape(fn, d, B));
  RC_REQUIRE(ws != nullptr && reinterpret_cast<uintptr_t>(ws) % 256 == 0, "%s: workspace must be 256-byte aligned", fn);
  *L = con_layout(d, B, const_cast<void*>(ws));
  RC_REQUIRE(ws_bytes >= L->bytes, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, L->bytes);
  return RC_OK;
}

}  // namespace rc

extern "C" int rc_contra_check_shape(int d, int64_t batch) { return rc::con_shape("rc_contra_check_shape", d, batch); }

extern "C" size_t rc_contra_workspace_bytes(int d, int64_t batch) {
  if (rc::con_shape("rc_contra_workspace_bytes", d, batch) != RC_OK) return 0;
  return rc::con_layout(d, batch, nullptr).bytes;
}

extern "C" int rc_contra_loss_fwd(const float* va, const float* vb, const int64_t* labels, int64_t batch, int d, float temperature,
                                  void* workspace, size_t ws_bytes, float* loss, rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_contra_loss_fwd";
  ConLayout L;
  RC_TRY(con_workspace_check(fn, d, batch, workspace, ws_bytes, &L));
  RC_REQUIRE(va != nullptr && vb != nullptr && loss != nullptr, "%s: null pointer", fn);
  RC_REQUIRE(con_aligned16(va) && con_aligned16(vb), "%s: the views must be 16-byte aligned", fn);
  RC_REQUIRE(temperature > 0.f, "%s: temperature must be positive, got %g", fn, (double)temperature);
  const hipStream_t st = as_stream(stream);
  const int lpr = con_lpr(d);
#define CON_ROWS(P) hipLaunchKernelGGL((con_rows_kernel<P>), dim3(con_row_grid(L.N, P)), dim3(kBlock), 0, st, va, vb, L)
  CON_LPR_SWITCH(lpr, CON_ROWS)
#undef CON_ROWS
  RC_LAUNCH_CHECK();
  const dim3 grid((unsigned)((L.N + kConRowsPerBlock - 1) / kConRowsPerBlock), (unsigned)L.chunks);
  const float inv_t = 1.f / temperature;
#define CON_STATS(P) hipLaunchKernelGGL((con_stats_kernel<P>), grid, dim3(256), 0, st, L, labels, inv_t)
  CON_DP_SWITCH((d + 31) / 32 * 32, CON_STATS)
#undef CON_STATS
  RC_LAUNCH_CHECK();
  int64_t fb = (L.N + kBlock - 1) / kBlock;
  if (fb > 4096) fb = 4096;
  hipLaunchKernelGGL(con_finish_kernel, dim3((unsigned)fb), dim3(kBlock), 0, st, L);
  RC_LAUNCH_CHECK();
  hipLaunchKernelGGL(con_reduce_kernel, dim3(1), dim3(kBlock), 0, st, L, temperature, loss);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

extern "C" int rc_contra_loss_bwd(const float* grad_out, const int64_t* labels, int64_t batch, int d, float temperature,
                                  void* workspace, size_t ws_bytes, float* grad_va, float* grad_vb, rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_contra_loss_bwd";
  ConLayout L;
  RC_TRY(con_workspace_check(fn, d, batch, workspace, ws_bytes, &L));
  RC_REQUIRE(grad_out != nullptr && grad_va != nullptr && grad_vb != nullptr, "%s: null pointer", fn);
  RC_REQUIRE(con_aligned16(grad_va) && con_aligned16(grad_vb), "%s: gradients must be 16-byte aligned", fn);
  RC_REQUIRE(temperature > 0.f, "%s: temperature must be positive, got %g", fn, (double)temperature);
  const hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((L.N + kConRowsPerBlock - 1) / kConRowsPerBlock), (unsigned)L.chunks);
  const float inv_t = 1.f / temperature;
#define CON_WEIGHT(P) hipLaunchKernelGGL((con_weight_kernel<P>), grid, dim3(256), 0, st, L, labels, inv_t)
  CON_DP_SWITCH((d + 31) / 32 * 32, CON_WEIGHT)
#undef CON_WEIGHT
  RC_LAUNCH_CHECK();
#define CON_BWD(P) \
  hipLaunchKernelGGL((con_bwd_rows_kernel<P>), dim3(con_row_grid(L.N, P)), dim3(kBlock), 0, st, L, grad_out, grad_va, grad_vb)
  CON_LPR_SWITCH(con_lpr(d), CON_BWD)
#undef CON_BWD
  RC_LAUNCH_CHECK();
  return RC_OK;
}
