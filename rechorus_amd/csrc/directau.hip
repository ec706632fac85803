// directau.hip -- DirectAU's alignment + uniformity loss  (reference: models/general/DirectAU.py:54-88)
//
//   x^ = x / max(|x|, 1e-12)                                   (F.normalize, per row)
//   align   = mean_b |u^_b - i^_b|^2
//   unif(X) = log( S / P ),  S = sum_{i<j} e_ij,  e_ij = exp(-2 |x^_i - x^_j|^2),  P = B (B - 1) / 2   (torch.pdist over the batch)
//   loss    = align + gamma (unif(U) + unif(I)) / 2
//
// With s_i = sum_{j != i} e_ij and M_i = sum_{j != i} e_ij x^_j the gradient of unif is -(4 / S) (s_i x^_i - M_i): forward and
// backward are ONE sweep over the pairs, the only global factor 1 / S is applied afterwards.  Launches:
//   rows      gather (optional ids), normalise, x^ / denominator / |x^|^2, per-row |u^ - i^|^2, optional prediction <u, i>
//   pairwise  per set, owner-computes on v_mfma_f32_32x32x2_f32: a wave owns 32 rows, the workgroup stages 32-row column blocks
//             in LDS and every wave sweeps them in a fixed order.  Per block: the Gram tile G' = X^_cols X^_own^T (columns j in
//             the accumulator rows, owned rows i on the lanes), the epilogue e = exp(-2 max(0, n_i + n_j - 2 G')) (diagonal and
//             rows past B masked), then M^T += X^_cols^T E' with E' straight from the accumulator as the B operand (its row index
//             is the product's k: the A operand is read from LDS in the same permuted k order).  Mid-size batches split the sweep
//             into column chunks whose s / M planes the backward pass adds in chunk order.  The B x B matrix is never stored.
//   reduce    one workgroup: sum of the alignment rows and of the per-wave S partials, in double, fixed order -> loss, stats
//   backward  per row: dx^ from the closed form, mapped back through the normalisation, per-occurrence row gradients [B, d]
// No float atomics anywhere: every sum has a fixed order, results are bitwise reproducible run to run.
#include "common.hpp"

namespace rc {

typedef float dau_f32x16 __attribute__((ext_vector_type(16)));

constexpr float kDauEps = 1e-12f;    // F.normalize's default eps
constexpr int kDauRowsPerWave = 32;  // rows a wave owns in the pairwise pass (one 32x32 MFMA tile)
constexpr int kDauRowsPerBlock = 128;
constexpr int kDauTargetBlocks = 512;
constexpr int kDauMaxChunks = 16;

struct DauLayout {  // the workspace, carved in this order
  int64_t B;
  int d, chunks, per_chunk;
  int64_t nrb;      // 32-row blocks
  float* xhat;      // [2][B][d]
  float* den;       // [2][B]   max(|x|, eps)
  float* nsq;       // [2][B]   |x^|^2
  float* align;     // [B]      |u^ - i^|^2
  float* s;         // [chunks][2][B]
  float* M;         // [chunks][2][B][d]
  float* spart;     // [chunks][2][nrb]
  double* stats;    // [4]: mean alignment, S_user, S_item, -
  size_t bytes;
};

static DauLayout dau_layout(int d, int64_t B, void* base) {
  DauLayout L{};
  L.B = B;
  L.d = d;
  const int64_t ncb = (B + 31) / 32;
  L.nrb = ncb;
  const int64_t nwg = (B + kDauRowsPerBlock - 1) / kDauRowsPerBlock;
  int64_t want = (kDauTargetBlocks + 2 * nwg - 1) / (2 * nwg);
  if (want > kDauMaxChunks) want = kDauMaxChunks;
  if (want > ncb) want = ncb;
  if (want < 1) want = 1;
  const int64_t per = (ncb + want - 1) / want;
  L.per_chunk = (int)per;
  L.chunks = (int)((ncb + per - 1) / per);
  Carver c(base);
  L.xhat = c.take<float>((size_t)2 * B * d);
  L.den = c.take<float>((size_t)2 * B);
  L.nsq = c.take<float>((size_t)2 * B);
  L.align = c.take<float>((size_t)B);
  L.s = c.take<float>((size_t)L.chunks * 2 * B);
  L.M = c.take<float>((size_t)L.chunks * 2 * B * d);
  L.spart = c.take<float>((size_t)L.chunks * 2 * L.nrb);
  L.stats = c.take<double>(4);
  L.bytes = c.off;
  return L;
}

template <int LPR>
__device__ __forceinline__ float dau_group_sum(float x) {   // butterfly inside a lane group: every lane gets the same bits
#pragma unroll
  for (int off = LPR / 2; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

__device__ __forceinline__ float4 dau_div4(float4 a, float s) { return make_float4(a.x / s, a.y / s, a.z / s, a.w / s); }
__device__ __forceinline__ float dau_dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// ---- row pass: LPR lanes per row (float4 each), 64 / LPR rows per wave ---------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(kBlock) void dau_rows_kernel(const float* __restrict__ utab, const int64_t* __restrict__ uid,
                                                          const float* __restrict__ itab, const int64_t* __restrict__ iid, int64_t B,
                                                          int d, DauLayout L, float* __restrict__ pred) {
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int l = lane % LPR;
  const bool on = 4 * l < d;
  const int64_t stride = (int64_t)gridDim.x * (kBlock / 64) * G;
  for (int64_t b = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * G + lane / LPR; b < B; b += stride) {
    const int64_t ru = uid ? uid[b] : b, ri = iid ? iid[b] : b;
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
    if (on) {
      u = *reinterpret_cast<const float4*>(utab + ru * d + 4 * l);
      v = *reinterpret_cast<const float4*>(itab + ri * d + 4 * l);
    }
    const float su = dau_group_sum<LPR>(dau_dot4(u, u));
    const float sv = dau_group_sum<LPR>(dau_dot4(v, v));
    const float dot = dau_group_sum<LPR>(dau_dot4(u, v));
    const float du = fmaxf(sqrtf(su), kDauEps), dv = fmaxf(sqrtf(sv), kDauEps);
    const float4 uh = dau_div4(u, du), vh = dau_div4(v, dv);
    const float4 df = make_float4(uh.x - vh.x, uh.y - vh.y, uh.z - vh.z, uh.w - vh.w);
    const float nu = dau_group_sum<LPR>(dau_dot4(uh, uh));
    const float nv = dau_group_sum<LPR>(dau_dot4(vh, vh));
    const float al = dau_group_sum<LPR>(dau_dot4(df, df));
    if (on) {
      *reinterpret_cast<float4*>(L.xhat + b * d + 4 * l) = uh;
      *reinterpret_cast<float4*>(L.xhat + (B + b) * d + 4 * l) = vh;
    }
    if (l == 0) {
      L.den[b] = du;
      L.den[B + b] = dv;
      L.nsq[b] = nu;
      L.nsq[B + b] = nv;
      L.align[b] = al;
      if (pred != nullptr) pred[b] = dot;
    }
  }
}

// ---- pairwise pass ----------------------------------------------------------------------------------------------------------------
// grid (ceil(B / 128), 2 sets, chunks), 256 threads.  DP = d rounded up to a multiple of 32 (zero padded in LDS and registers).
// Lane l of wave w: h = l >> 5, owned row i = 128 blockIdx.x + 32 w + (l & 31).
//   Gram step t (t < DP / 2): k = h DP / 2 + t on both operands; A = X_cols[l & 31][k] (LDS), B = X_own[i][k] (registers, loaded once)
//   accumulator register r of lane l: column-block row jr(r, h) = (r & 3) + 8 (r >> 2) + 4 h, owned row i
//   M^T tile ct, step r: A = X_cols[jr(r, h)][32 ct + (l & 31)] (LDS), B = e[r] (k = jr(r, h) on both operands);
//   its register r of lane l holds M^T[32 ct + jr(r, h)][i] (the same accumulator layout)
template <int DP>
__global__ __launch_bounds__(256) void dau_pair_kernel(DauLayout L, int sets) {
  const int set = blockIdx.y;
  if (!((sets >> set) & 1)) return;   // (workgroup-uniform, before any barrier)
  const int64_t B = L.B;
  const int d = L.d;
  const int chunk = blockIdx.z;
  const float* __restrict__ X = L.xhat + (int64_t)set * B * d;
  const float* __restrict__ N = L.nsq + (int64_t)set * B;
  constexpr int SR = DP + 4;            // LDS row stride (floats)
  constexpr int KH = DP / 2;            // k per lane half
  constexpr int NCT = DP / 32;          // M^T tiles
  constexpr int NL = DP / 32;           // float4 staged per thread per column block (32 rows x DP floats / 256 threads)
  __shared__ __attribute__((aligned(16))) float xs[32 * SR];
  __shared__ float ns[32];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31;
  const int64_t i = (int64_t)blockIdx.x * kDauRowsPerBlock + wave * kDauRowsPerWave + li;
  const bool iv = i < B;

  float breg[KH];
#pragma unroll
  for (int t = 0; t < KH; ++t) {
    const int k = h * KH + t;
    breg[t] = (iv && k < d) ? X[i * d + k] : 0.f;
  }
  const float ni = iv ? N[i] : 0.f;
  dau_f32x16 accM[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) accM[ct][r] = 0.f;
  float sl = 0.f;

  const int64_t ncb = L.nrb;
  const int64_t cb0 = (int64_t)chunk * L.per_chunk;
  const int64_t cb1 = cb0 + L.per_chunk < ncb ? cb0 + L.per_chunk : ncb;
  float4 pre[NL];
  auto fetch = [&](int64_t cb) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int idx = threadIdx.x + q * 256;
      const int row = idx / (DP / 4), c4 = idx % (DP / 4);
      const int64_t j = cb * 32 + row;
      pre[q] = (j < B && 4 * c4 < d) ? *reinterpret_cast<const float4*>(X + j * d + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  float nj_pre = 0.f;
  if (cb0 < cb1) {
    fetch(cb0);
    if (threadIdx.x < 32) nj_pre = cb0 * 32 + threadIdx.x < B ? N[cb0 * 32 + threadIdx.x] : 0.f;
  }
  for (int64_t cb = cb0; cb < cb1; ++cb) {
    __syncthreads();   // every wave is done with the previous block
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int idx = threadIdx.x + q * 256;
      const int row = idx / (DP / 4), c4 = idx % (DP / 4);
      *reinterpret_cast<float4*>(&xs[row * SR + 4 * c4]) = pre[q];
    }
    if (threadIdx.x < 32) ns[threadIdx.x] = nj_pre;
    __syncthreads();
    if (cb + 1 < cb1) {   // prefetch the next block into registers while this one is computed
      fetch(cb + 1);
      if (threadIdx.x < 32) nj_pre = (cb + 1) * 32 + threadIdx.x < B ? N[(cb + 1) * 32 + threadIdx.x] : 0.f;
    }
    dau_f32x16 g;
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
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jr = (r & 3) + 8 * (r >> 2) + 4 * h;
      const int64_t j = cb * 32 + jr;
      // Gram form of |x^_i - x^_j|^2: identical rows give ~0 with either sign, hence the clamp
      const float dist = fmaxf(ns[jr] + ni - 2.f * g[r], 0.f);
      const float e = (j < B && j != i) ? expf(-2.f * dist) : 0.f;
      g[r] = e;
      sl += e;
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jr = (r & 3) + 8 * (r >> 2) + 4 * h;
        accM[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[jr * SR + 32 * ct + li], g[r], accM[ct], 0, 0, 0);
      }
    }
  }

  const float si = sl + __shfl_xor(sl, 32, 64);   // the two lane halves hold the two halves of the column block rows
  const int64_t plane = (int64_t)chunk * 2 + set;
  if (iv) {
    if (h == 0) L.s[plane * B + i] = si;
    float* Mi = L.M + (plane * B + i) * d;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * ct + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (c < d) Mi[c] = accM[ct][r];
      }
  }
  // this wave's 32 rows: sum of s_i in a fixed butterfly order (rows past B count 0)
  float ws = (iv && h == 0) ? si : 0.f;
#pragma unroll
  for (int off = 16; off >= 1; off >>= 1) ws += __shfl_xor(ws, off, 64);
  const int64_t rb = (int64_t)blockIdx.x * (kDauRowsPerBlock / kDauRowsPerWave) + wave;
  if (lane == 0 && rb < L.nrb) L.spart[plane * L.nrb + rb] = ws;
}

// ---- reduce: one workgroup, double, fixed order ------------------------------------------------------------------------------------
// out[0] loss = align + gamma (unif_u + unif_i) / 2, out[1] align, out[2] unif_u, out[3] unif_i (a set not computed reads 0 there)
__global__ __launch_bounds__(kBlock) void dau_reduce_kernel(DauLayout L, int sets, float gamma, float* __restrict__ out) {
  __shared__ double red[3][kBlock];
  const int t = threadIdx.x;
  double a = 0.0, su = 0.0, si = 0.0;
  for (int64_t b = t; b < L.B; b += kBlock) a += (double)L.align[b];
  const int64_t np = (int64_t)L.chunks * L.nrb;
  for (int64_t p = t; p < np; p += kBlock) {
    const int64_t c = p / L.nrb, rb = p - c * L.nrb;
    if (sets & 1) su += (double)L.spart[(c * 2 + 0) * L.nrb + rb];
    if (sets & 2) si += (double)L.spart[(c * 2 + 1) * L.nrb + rb];
  }
  red[0][t] = a;
  red[1][t] = su;
  red[2][t] = si;
  __syncthreads();
  for (int w = kBlock / 2; w >= 1; w >>= 1) {
    if (t < w) {
      red[0][t] += red[0][t + w];
      red[1][t] += red[1][t + w];
      red[2][t] += red[2][t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double B = (double)L.B;
    const double align = red[0][0] / B;
    const double S_u = 0.5 * red[1][0], S_i = 0.5 * red[2][0];
    const double P = B * (B - 1.0) / 2.0;                  // B = 1: 0 / 0, NaN, as the mean of torch.pdist's empty result
    const double uu = (sets & 1) ? log(S_u / P) : 0.0;
    const double ui = (sets & 2) ? log(S_i / P) : 0.0;
    L.stats[0] = align;
    L.stats[1] = S_u;
    L.stats[2] = S_i;
    L.stats[3] = 0.0;
    out[0] = (float)(align + (double)gamma * (uu + ui) / 2.0);
    out[1] = (float)align;
    out[2] = (float)uu;
    out[3] = (float)ui;
  }
}

// ---- backward: per row, LPR lanes (float4 each) ------------------------------------------------------------------------------------
struct DauCoef {
  float align, unif_u, unif_i;   // d loss / d (align, unif_u, unif_i), times the upstream gradient read on the device
};

template <int LPR>
__device__ __forceinline__ float4 dau_unnormalise(float4 g, float4 xh, float den) {
  // F.normalize's backward: x / max(|x|, eps); past eps (g - x^ (x^ . g)) / |x|, else g / eps (den = max(|x|, eps))
  if (den > kDauEps) {
    const float p = dau_group_sum<LPR>(dau_dot4(xh, g));
    return make_float4((g.x - xh.x * p) / den, (g.y - xh.y * p) / den, (g.z - xh.z * p) / den, (g.w - xh.w * p) / den);
  }
  return dau_div4(g, kDauEps);
}

template <int LPR>
__global__ __launch_bounds__(kBlock) void dau_bwd_kernel(DauLayout L, const float* __restrict__ gloss, DauCoef cf,
                                                         float* __restrict__ gu, float* __restrict__ gi) {
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int l = lane % LPR;
  const bool on = 4 * l < L.d;
  const int64_t B = L.B;
  const int d = L.d;
  const float g0 = gloss[0];
  const float ca = g0 * cf.align * 2.f / (float)B;
  const bool pairs = B >= 2;   // B = 1: torch.pdist is empty, its backward contributes nothing
  const float cu = pairs && cf.unif_u != 0.f ? (float)(-4.0 * (double)(g0 * cf.unif_u) / L.stats[1]) : 0.f;
  const float ci = pairs && cf.unif_i != 0.f ? (float)(-4.0 * (double)(g0 * cf.unif_i) / L.stats[2]) : 0.f;
  const int64_t stride = (int64_t)gridDim.x * (kBlock / 64) * G;
  for (int64_t b = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * G + lane / LPR; b < B; b += stride) {
    float4 uh = make_float4(0.f, 0.f, 0.f, 0.f), vh = uh, Mu = uh, Mv = uh;
    float su = 0.f, sv = 0.f;
    if (on) {
      uh = *reinterpret_cast<const float4*>(L.xhat + b * d + 4 * l);
      vh = *reinterpret_cast<const float4*>(L.xhat + (B + b) * d + 4 * l);
    }
    for (int c = 0; c < L.chunks; ++c) {   // chunk partials in chunk order
      const int64_t pu = (int64_t)c * 2, pv = pu + 1;
      su += L.s[pu * B + b];
      sv += L.s[pv * B + b];
      if (on) {
        const float4 a = *reinterpret_cast<const float4*>(L.M + (pu * B + b) * d + 4 * l);
        const float4 e = *reinterpret_cast<const float4*>(L.M + (pv * B + b) * d + 4 * l);
        Mu = make_float4(Mu.x + a.x, Mu.y + a.y, Mu.z + a.z, Mu.w + a.w);
        Mv = make_float4(Mv.x + e.x, Mv.y + e.y, Mv.z + e.z, Mv.w + e.w);
      }
    }
    float4 du, dv;
    du.x = ca * (uh.x - vh.x) + (cu != 0.f ? cu * (su * uh.x - Mu.x) : 0.f);
    du.y = ca * (uh.y - vh.y) + (cu != 0.f ? cu * (su * uh.y - Mu.y) : 0.f);
    du.z = ca * (uh.z - vh.z) + (cu != 0.f ? cu * (su * uh.z - Mu.z) : 0.f);
    du.w = ca * (uh.w - vh.w) + (cu != 0.f ? cu * (su * uh.w - Mu.w) : 0.f);
    dv.x = -ca * (uh.x - vh.x) + (ci != 0.f ? ci * (sv * vh.x - Mv.x) : 0.f);
    dv.y = -ca * (uh.y - vh.y) + (ci != 0.f ? ci * (sv * vh.y - Mv.y) : 0.f);
    dv.z = -ca * (uh.z - vh.z) + (ci != 0.f ? ci * (sv * vh.z - Mv.z) : 0.f);
    dv.w = -ca * (uh.w - vh.w) + (ci != 0.f ? ci * (sv * vh.w - Mv.w) : 0.f);
    const float4 ou = dau_unnormalise<LPR>(du, uh, L.den[b]);
    const float4 ov = dau_unnormalise<LPR>(dv, vh, L.den[B + b]);
    if (on) {
      if (gu != nullptr) *reinterpret_cast<float4*>(gu + b * d + 4 * l) = ou;
      if (gi != nullptr) *reinterpret_cast<float4*>(gi + b * d + 4 * l) = ov;
    }
  }
}

static unsigned dau_row_grid(int64_t B, int lpr) {
  const int64_t rows_per_block = (kBlock / 64) * (64 / lpr);
  int64_t blocks = (B + rows_per_block - 1) / rows_per_block;
  if (blocks < 1) blocks = 1;
  if (blocks > 65536) blocks = 65536;
  return (unsigned)blocks;
}

static int dau_lpr(int d) {
  const int dq = d / 4;
  int lpr = 1;
  while (lpr < dq) lpr <<= 1;
  return lpr;
}

#define DAU_LPR_SWITCH(lpr, F) \
  switch (lpr) {               \
    case 1: F(1); break;       \
    case 2: F(2); break;       \
    case 4: F(4); break;       \
    case 8: F(8); break;       \
    case 16: F(16); break;     \
    case 32: F(32); break;     \
    default: F(64); break;     \
  }

// the one statement of the envelope: every entry point checks it, rc_directau_check_shape reports it to the host
static int dau_shape(const char* fn, int d, int64_t B) {
  if (d % 4 == 0 && d >= 4 && d <= 256 && B >= 1 && B <= ((int64_t)1 << 20)) return RC_OK;
  return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (emb_size a multiple of 4 in [4, 256], batch in [1, 1048576]): "
              "emb_size=%d batch=%lld", fn, d, (long long)B);
}

static bool dau_aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

static int dau_workspace_check(const char* fn, int d, int64_t B, const void* ws, size_t ws_bytes, DauLayout* L) {
  RC_TRY(dau_shape(fn, d, B));
  RC_REQUIRE(ws != nullptr && reinterpret_cast<uintptr_t>(ws) % 256 == 0, "%s: workspace must be 256-byte aligned", fn);
  *L = dau_layout(d, B, const_cast<void*>(ws));
  RC_REQUIRE(ws_bytes >= L->bytes, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, L->bytes);
  return RC_OK;
}

}  // namespace rc

extern "C" int rc_directau_check_shape(int d, int64_t batch) { return rc::dau_shape("rc_directau_check_shape", d, batch); }

extern "C" size_t rc_directau_workspace_bytes(int d, int64_t batch) {
  if (rc::dau_shape("rc_directau_workspace_bytes", d, batch) != RC_OK) return 0;
  return rc::dau_layout(d, batch, nullptr).bytes;
}

extern "C" int rc_directau_fwd(const float* user_tab, const int64_t* uid, const float* item_tab, const int64_t* iid, int64_t batch,
                               int d, float gamma, int sets, void* workspace, size_t ws_bytes, float* prediction, float* out,
                               rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_directau_fwd";
  DauLayout L;
  RC_TRY(dau_workspace_check(fn, d, batch, workspace, ws_bytes, &L));
  RC_REQUIRE(user_tab != nullptr && item_tab != nullptr && out != nullptr, "%s: null pointer", fn);
  RC_REQUIRE(dau_aligned16(user_tab) && dau_aligned16(item_tab), "%s: tables must be 16-byte aligned", fn);
  RC_REQUIRE(sets >= 0 && sets <= 3, "%s: sets is a bit mask of {1: users, 2: items}", fn);
  const hipStream_t st = as_stream(stream);
  const int lpr = dau_lpr(d);
#define DAU_ROWS(P)                                                                                                         \
  hipLaunchKernelGGL((dau_rows_kernel<P>), dim3(dau_row_grid(batch, P)), dim3(kBlock), 0, st, user_tab, uid, item_tab, iid, \
                     batch, d, L, prediction)
  DAU_LPR_SWITCH(lpr, DAU_ROWS)
#undef DAU_ROWS
  RC_LAUNCH_CHECK();
  if (sets != 0) {
    const dim3 grid((unsigned)((batch + kDauRowsPerBlock - 1) / kDauRowsPerBlock), 2, (unsigned)L.chunks);
    const int dp = (d + 31) / 32 * 32;
#define DAU_PAIR(P) hipLaunchKernelGGL((dau_pair_kernel<P>), grid, dim3(256), 0, st, L, sets)
    switch (dp) {
      case 32: DAU_PAIR(32); break;
      case 64: DAU_PAIR(64); break;
      case 96: DAU_PAIR(96); break;
      case 128: DAU_PAIR(128); break;
      case 160: DAU_PAIR(160); break;
      case 192: DAU_PAIR(192); break;
      case 224: DAU_PAIR(224); break;
      default: DAU_PAIR(256); break;
    }
#undef DAU_PAIR
    RC_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(dau_reduce_kernel, dim3(1), dim3(kBlock), 0, st, L, sets, gamma, out);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

extern "C" int rc_directau_bwd(const float* grad_out, int64_t batch, int d, float coef_align, float coef_unif_user,
                               float coef_unif_item, const void* workspace, size_t ws_bytes, float* grad_user, float* grad_item,
                               rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_directau_bwd";
  DauLayout L;
  RC_TRY(dau_workspace_check(fn, d, batch, workspace, ws_bytes, &L));
  RC_REQUIRE(grad_out != nullptr && (grad_user != nullptr || grad_item != nullptr), "%s: null pointer", fn);
  RC_REQUIRE((grad_user == nullptr || dau_aligned16(grad_user)) && (grad_item == nullptr || dau_aligned16(grad_item)),
             "%s: gradients must be 16-byte aligned", fn);
  const hipStream_t st = as_stream(stream);
  const DauCoef cf{coef_align, coef_unif_user, coef_unif_item};
#define DAU_BWD(P)                                                                                                          \
  hipLaunchKernelGGL((dau_bwd_kernel<P>), dim3(dau_row_grid(batch, P)), dim3(kBlock), 0, st, L, grad_out, cf, grad_user, \
                     grad_item)
  DAU_LPR_SWITCH(dau_lpr(d), DAU_BWD)
#undef DAU_BWD
  RC_LAUNCH_CHECK();
  return RC_OK;
}
