// dcnv2.hip -- DCNv2's mixed (mixture-of-low-rank-experts) cross layer (reference: models/context/DCNv2.py:96-144)
//
//   X0, Xl [N, D], N = batch * candidates;  U, V [E, D, r], C [E, r, r], bias [D];  the gate Wg [E, D], bg [E] (one gate for every layer)
//   per row and expert e:  t = tanh(V_e^T x_l),  s = tanh(C_e t),  y_e = U_e s + bias
//   g = softmax_e(Wg_e . x_l + bg_e),  x_{l+1} = x_l + x_0 * sum_e g_e y_e
//
// Launches: the forward is ONE launch per layer; the backward is TWO (the row-tile kernel and the fixed-order reduce of its partials).
//   tile    a workgroup of four waves owns TR = 16 RB rows (RB = 4 / 2 / 1: the largest for which the tile fits the 160 KB LDS and
//           every wave keeps its share of the [TR, D] accumulators in registers, halved while the batch gives fewer than 256 tiles)
//           and walks the batch with the grid as its stride.  Xl and X0 (backward: Xl and W = dXnext * X0) sit in LDS as
//           [TR][DP + 4], DP = D rounded up to 16, zero in the padding and in the rows past the batch; one expert's t, s (backward:
//           also dq, and dp over s) as [TR][RP + 4].  At D = 1024, r = 128 that is 2 * 64.25 KB + 3 * 8.25 KB + 1 KB = 154.25 KB.
//   MFMA    every product runs on v_mfma_f32_16x16x4_f32: the tile's rows are the A operand out of LDS, the weights the B operand
//           straight from global memory -- E (2 D r + r^2) floats, 0.5 MB at the demo shape, are L2-resident and every workgroup reads
//           all of them for every tile, so staging them through LDS would only copy them once more (and the LDS is full of rows at
//           D = 1024).  A wave takes 16-wide output column tiles and keeps RB accumulators per tile, so a weight operand is used RB
//           times.  Where the contraction index is the weights' contiguous one (C t, U s, V dp) both operands are read as float4 and
//           lane group g contracts k = 16 step + 4 g + u, u = 0..3; elsewhere (V^T x, U^T w, C^T dq) k = 4 step + g.
//   bwd     recomputes t, s and g.  Per expert: dg_e = <W, y_e> (16-lane butterfly, then the four waves in wave order), dq = g_e (U_e^T W)
//           (1 - s^2), dp = (C_e^T dq)(1 - t^2); dXl = dXnext + sum_e V_e dp_e + sum_e dz_e Wg_e with dz = g (dg - <g, dg>) and
//           dX0_part = dXnext * sum_e g_e y_e stay in registers over the experts and are stored once (dXnext is read a second time, from
//           L2, by that store: the LDS holds W = dXnext * X0 instead of dXnext).  The weight gradients dU_e = W^T
//           (g_e s), dC_e = dq^T t, dV_e = Xl^T dp are rank-TR updates on the same MFMA, added to THIS workgroup's partial in the caller
//           workspace (plain loads and stores: nobody else touches it; the first tile stores without loading, so the workspace needs no
//           zero fill); dbias, dWg, dbg are summed in registers over the workgroup's tiles.
//   reduce  one thread per element of dU | dV | dC | dbias | dWg | dbg adds the workgroups' partials in workgroup order, in double.
// The number of workgroups (= partials) is min(tiles, 256, 128 MB / bytes of one partial): independent of N once N passes 256 tiles.
// No float atomics anywhere: every sum has a fixed order, results are bitwise reproducible run to run.
#include <mutex>

#include "common.hpp"

namespace rc {

typedef float dc_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kDcMaxBlocks = 256;
constexpr int kDcMaxE = 4;
constexpr size_t kDcLdsBudget = 160 * 1024;
constexpr size_t kDcPartialBudget = (size_t)128 << 20;

struct DcGeom {      // everything derived from (N, D, r, E) and the pass; host side, copied into the kernel arguments
  int D, r, E;
  int DP, DS, RP, RS, CT, RT;   // padded widths, LDS row strides, 16-wide column tiles of D and r
  int RB, TR;
  int64_t P, PS;                // floats of one partial, and its stride (256-byte multiple)
  size_t lds;
};

struct DcArgs {
  const float *X0, *Xl, *U, *V, *C, *bias, *Wg, *bg;
  const float* dXn;               // backward
  float* Xnext;                   // forward
  float *dXl, *dX0, *part;        // backward
  int64_t N;
  DcGeom g;
};

static size_t dc_lds_bytes(int DS, int RS, int RB, bool bwd) {
  const size_t TR = 16 * (size_t)RB;
  return (2 * TR * DS + (bwd ? 3 : 2) * TR * RS + (bwd ? 16 : 4) * TR) * sizeof(float);
}

// n < 0: the smallest tile (what rc_dcnv2_check_shape asks for)
static bool dc_geometry(int64_t N, int D, int r, int E, bool bwd, DcGeom* out) {
  DcGeom g{};
  g.D = D, g.r = r, g.E = E;
  g.DP = (D + 15) / 16 * 16, g.DS = g.DP + 4, g.CT = g.DP / 16;
  g.RP = (r + 15) / 16 * 16, g.RS = g.RP + 4, g.RT = g.RP / 16;
  int RB = 0;
  // a wave keeps RB * ceil(CT / 4) accumulator tiles of Xnext (backward: of dXl and of dX0_part, so half as many columns per tile
  // height -- beyond that the compiler spills; the one shape class that still does is RB = 1 with D > 512 in the backward)
  for (int c : {4, 2, 1})
    if ((c == 1 || g.DP * c <= (bwd ? 512 : 1024)) && dc_lds_bytes(g.DS, g.RS, c, bwd) <= kDcLdsBudget) {
      RB = c;
      break;
    }
  if (RB == 0) return false;
  if (N < 0) RB = 1;
  while (RB > 1 && (N + 16 * RB - 1) / (16 * RB) < kDcMaxBlocks) RB /= 2;
  g.RB = RB, g.TR = 16 * RB;
  g.lds = dc_lds_bytes(g.DS, g.RS, RB, bwd);
  g.P = (int64_t)E * (2 * (int64_t)D * r + (int64_t)r * r) + D + (int64_t)E * D + E;
  g.PS = (g.P + 63) / 64 * 64;
  *out = g;
  return true;
}

static int dc_blocks(const DcGeom& g, int64_t N, bool bwd) {
  int64_t b = (N + g.TR - 1) / g.TR;
  if (b > kDcMaxBlocks) b = kDcMaxBlocks;
  if (bwd) {
    int64_t cap = (int64_t)(kDcPartialBudget / ((size_t)g.PS * sizeof(float)));
    if (cap < 1) cap = 1;
    if (b > cap) b = cap;
  }
  return (int)b;
}

// ---- device pieces -----------------------------------------------------------------------------------------------------------------
#define DC_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

template <int RB>
__device__ __forceinline__ void dc_zero(dc_f32x4 (&acc)[RB]) {
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) acc[rb] = dc_f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc[rb][v] += sum_k in[16 rb + 4 g + v][k] W[k ldw + n0 + i] over k in [0, K), K % 4 == 0; lane = 16 g + i.  Columns n >= nvalid are 0
template <int RB>
__device__ __forceinline__ void dc_mm_kn(const float* in, int ins, int K, const float* __restrict__ W, int ldw, int n0, int nvalid,
                                         dc_f32x4 (&acc)[RB], int lane) {
  const int i = lane & 15, g = lane >> 4;
  const bool ok = n0 + i < nvalid;
  const float* wp = W + (int64_t)g * ldw + (ok ? n0 + i : 0);
  const float* ip = in + i * ins + g;
#pragma unroll 4
  for (int k0 = 0; k0 < K; k0 += 4) {
    const float b = ok ? wp[(int64_t)k0 * ldw] : 0.f;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb] = DC_MFMA(ip[rb * 16 * ins + k0], b, acc[rb]);
  }
}

// acc[rb][v] += sum_k in[16 rb + 4 g + v][k] W[(n0 + i) ldw + k] over k in [0, K), K % 4 == 0; `in` is finite up to K rounded up to 16
template <int RB>
__device__ __forceinline__ void dc_mm_nk(const float* in, int ins, int K, const float* __restrict__ W, int ldw, int n0, int nvalid,
                                         dc_f32x4 (&acc)[RB], int lane) {
  const int i = lane & 15, g = lane >> 4;
  const bool ok = n0 + i < nvalid;
  const float* wp = W + (int64_t)(ok ? n0 + i : 0) * ldw + 4 * g;
  const float* ip = in + i * ins + 4 * g;
#pragma unroll 2
  for (int k0 = 0; k0 < K; k0 += 16) {
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok && k0 + 4 * g < K) b = *reinterpret_cast<const float4*>(wp + k0);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const float4 x = *reinterpret_cast<const float4*>(ip + rb * 16 * ins + k0);
      acc[rb] = DC_MFMA(x.x, b.x, acc[rb]);
      acc[rb] = DC_MFMA(x.y, b.y, acc[rb]);
      acc[rb] = DC_MFMA(x.z, b.z, acc[rb]);
      acc[rb] = DC_MFMA(x.w, b.w, acc[rb]);
    }
  }
}

// out[a0 + 4 g + v][b0 + i] (+)= sum over the tile's rows of L[row][a0 + i] R[row][b0 + i] scale[4 row]  (scale may be null)
template <int RB>
__device__ __forceinline__ void dc_wgrad(const float* L, int ls, const float* R, int rs, const float* scale, int a0, int b0, float* out,
                                         int ld, int A, int B, bool first, int lane) {
  const int i = lane & 15, g = lane >> 4;
  dc_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int row0 = 0; row0 < 16 * RB; row0 += 4) {
    const int row = row0 + g;
    float b = R[row * rs + b0 + i];
    if (scale != nullptr) b *= scale[4 * row];
    acc = DC_MFMA(L[row * ls + a0 + i], b, acc);
  }
  if (b0 + i < B) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int ar = a0 + 4 * g + v;
      if (ar < A) {
        float* p = out + (int64_t)ar * ld + b0 + i;
        *p = first ? acc[v] : *p + acc[v];
      }
    }
  }
}

// rows [row0, row0 + rows_valid) of X (times Y when given) -> dst [TR][DS], zeros in the padding and the rows past the batch
__device__ __forceinline__ void dc_load(const DcGeom& g, const float* X, const float* Y, float* dst, int64_t row0, int rows_valid, int tid) {
  const int Q4 = g.DP / 4;
  for (int idx = tid; idx < g.TR * Q4; idx += 256) {
    const int row = idx / Q4, c = 4 * (idx - row * Q4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < rows_valid && c < g.D) {
      v = load_stream4(reinterpret_cast<const float4*>(X + (row0 + row) * g.D + c));
      if (Y != nullptr) {
        const float4 y = load_stream4(reinterpret_cast<const float4*>(Y + (row0 + row) * g.D + c));
        v = make_float4(v.x * y.x, v.y * y.y, v.z * y.z, v.w * y.w);
      }
    }
    *reinterpret_cast<float4*>(&dst[row * g.DS + c]) = v;
  }
}

// G[4 row + e] = softmax_e(Wg_e . xl[row] + bg_e): a wave per row, the lanes over D
__device__ __forceinline__ void dc_gate(const DcArgs& a, const float* xl, float* G, int tid) {
  const DcGeom& g = a.g;
  const int wave = tid >> 6, lane = tid & 63;
  for (int row = wave; row < g.TR; row += 4) {
    float z[kDcMaxE];
#pragma unroll
    for (int e = 0; e < kDcMaxE; ++e) {
      z[e] = -INFINITY;
      if (e < g.E) {
        float acc = 0.f;
        for (int j = 4 * lane; j < g.D; j += 256)
          acc += dot4(*reinterpret_cast<const float4*>(&xl[row * g.DS + j]), *reinterpret_cast<const float4*>(a.Wg + (int64_t)e * g.D + j));
        z[e] = wave_allreduce_sum(acc) + a.bg[e];
      }
    }
    float m = z[0];
#pragma unroll
    for (int e = 1; e < kDcMaxE; ++e) m = fmaxf(m, z[e]);
    float l = 0.f;
#pragma unroll
    for (int e = 0; e < kDcMaxE; ++e) {
      z[e] = e < g.E ? expf(z[e] - m) : 0.f;
      l += z[e];
    }
    const float mine = lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3];
    if (lane < kDcMaxE) G[4 * row + lane] = mine / l;
  }
}

// t = tanh(V_e^T xl) -> T, then s = tanh(C_e t) -> S; ends synchronised
template <int RB>
__device__ __forceinline__ void dc_low_rank(const DcArgs& a, int e, const float* xl, float* T, float* S, int tid) {
  const DcGeom& g = a.g;
  const int wave = tid >> 6, lane = tid & 63, i = lane & 15, gq = lane >> 4;
  const float* Ve = a.V + (int64_t)e * g.D * g.r;
  const float* Ce = a.C + (int64_t)e * g.r * g.r;
  for (int ct = wave; ct < g.RT; ct += 4) {
    dc_f32x4 acc[RB];
    dc_zero<RB>(acc);
    dc_mm_kn<RB>(xl, g.DS, g.D, Ve, g.r, 16 * ct, g.r, acc, lane);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int v = 0; v < 4; ++v) T[(16 * rb + 4 * gq + v) * g.RS + 16 * ct + i] = tanhf(acc[rb][v]);
  }
  __syncthreads();
  for (int ct = wave; ct < g.RT; ct += 4) {
    dc_f32x4 acc[RB];
    dc_zero<RB>(acc);
    dc_mm_nk<RB>(T, g.RS, g.r, Ce, g.r, 16 * ct, g.r, acc, lane);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int v = 0; v < 4; ++v) S[(16 * rb + 4 * gq + v) * g.RS + 16 * ct + i] = tanhf(acc[rb][v]);
  }
  __syncthreads();
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <int RB, int MAXCT>
__global__ __launch_bounds__(256) void dcnv2_fwd_kernel(DcArgs a) {
  const DcGeom& g = a.g;
  constexpr int TR = 16 * RB;
  extern __shared__ __attribute__((aligned(16))) float dc_lds[];
  float* xl = dc_lds;                  // [TR][DS]
  float* x0 = xl + TR * g.DS;          // [TR][DS]
  float* T = x0 + TR * g.DS;           // [TR][RS]
  float* S = T + TR * g.RS;            // [TR][RS]
  float* G = S + TR * g.RS;            // [TR][4]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, gq = lane >> 4;
  const int64_t ntiles = (a.N + TR - 1) / TR;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * TR;
    const int rows_valid = (int)(a.N - row0 < TR ? a.N - row0 : TR);
    __syncthreads();   // every wave is done with the previous tile's LDS
    dc_load(g, a.Xl, nullptr, xl, row0, rows_valid, tid);
    dc_load(g, a.X0, nullptr, x0, row0, rows_valid, tid);
    __syncthreads();
    dc_gate(a, xl, G, tid);     // visible after the first barrier of dc_low_rank
    dc_f32x4 facc[MAXCT][RB];
#pragma unroll
    for (int c = 0; c < MAXCT; ++c) dc_zero<RB>(facc[c]);
    for (int e = 0; e < g.E; ++e) {
      dc_low_rank<RB>(a, e, xl, T, S, tid);
      const float* Ue = a.U + (int64_t)e * g.D * g.r;
#pragma unroll
      for (int c = 0; c < MAXCT; ++c) {
        const int ct = wave + 4 * c;
        if (ct < g.CT) {     // (wave-uniform)
          dc_f32x4 acc[RB];
          dc_zero<RB>(acc);
          dc_mm_nk<RB>(S, g.RS, g.r, Ue, g.r, 16 * ct, g.D, acc, lane);
          const int col = 16 * ct + i;
          const float b = col < g.D ? a.bias[col] : 0.f;
#pragma unroll
          for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int v = 0; v < 4; ++v) facc[c][rb][v] = fmaf(G[4 * (16 * rb + 4 * gq + v) + e], acc[rb][v] + b, facc[c][rb][v]);
        }
      }
      // the next expert's first product writes T only; its barrier keeps S until every wave is done here
    }
#pragma unroll
    for (int c = 0; c < MAXCT; ++c) {
      const int ct = wave + 4 * c, col = 16 * ct + i;
      if (ct < g.CT && col < g.D) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int row = 16 * rb + 4 * gq + v;
            if (row < rows_valid) a.Xnext[(row0 + row) * g.D + col] = fmaf(x0[row * g.DS + col], facc[c][rb][v], xl[row * g.DS + col]);
          }
      }
    }
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
template <int RB, int MAXCT>
__global__ __launch_bounds__(256) void dcnv2_bwd_kernel(DcArgs a) {
  const DcGeom& g = a.g;
  constexpr int TR = 16 * RB;
  extern __shared__ __attribute__((aligned(16))) float dc_lds[];
  float* xl = dc_lds;                  // [TR][DS]
  float* w = xl + TR * g.DS;           // [TR][DS]: dXnext * X0
  float* T = w + TR * g.DS;            // [TR][RS]
  float* S = T + TR * g.RS;            // [TR][RS]: s, then dp
  float* Q = S + TR * g.RS;            // [TR][RS]: dq
  float* G = Q + TR * g.RS;            // [TR][4]
  float* DG = G + 4 * TR;              // [TR][4]
  float* DZ = DG + 4 * TR;             // [TR][4]
  float* DGP = DZ + 4 * TR;            // [4 waves][TR]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, gq = lane >> 4;
  const int D = g.D, r = g.r, E = g.E, DS = g.DS, RS = g.RS;
  float* part = a.part + (int64_t)blockIdx.x * g.PS;
  float* pU = part;
  float* pV = pU + (int64_t)E * D * r;
  float* pC = pV + (int64_t)E * D * r;
  float* pb = pC + (int64_t)E * r * r;
  float* pWg = pb + D;
  float* pbg = pWg + (int64_t)E * D;
  float dbacc[4] = {0.f, 0.f, 0.f, 0.f}, dwgacc[4][kDcMaxE], dbgacc = 0.f;     // columns tid + 256 c
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int e = 0; e < kDcMaxE; ++e) dwgacc[c][e] = 0.f;
  bool first = true;
  const int64_t ntiles = (a.N + TR - 1) / TR;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * TR;
    const int rows_valid = (int)(a.N - row0 < TR ? a.N - row0 : TR);
    __syncthreads();
    dc_load(g, a.Xl, nullptr, xl, row0, rows_valid, tid);
    dc_load(g, a.dXn, a.X0, w, row0, rows_valid, tid);
    __syncthreads();
    dc_gate(a, xl, G, tid);
    dc_f32x4 dx0acc[MAXCT][RB], dxlacc[MAXCT][RB];
#pragma unroll
    for (int c = 0; c < MAXCT; ++c) dc_zero<RB>(dx0acc[c]), dc_zero<RB>(dxlacc[c]);
    for (int e = 0; e < E; ++e) {
      dc_low_rank<RB>(a, e, xl, T, S, tid);
      const float* Ue = a.U + (int64_t)e * D * r;
      const float* Ve = a.V + (int64_t)e * D * r;
      const float* Ce = a.C + (int64_t)e * r * r;
      // y_e = U_e s + bias: sum_e g_e y_e for dX0_part, dg_e = <w, y_e>
      {
        dc_f32x4 dgl[RB];
        dc_zero<RB>(dgl);
#pragma unroll
        for (int c = 0; c < MAXCT; ++c) {
          const int ct = wave + 4 * c;
          if (ct < g.CT) {     // (wave-uniform)
            dc_f32x4 acc[RB];
            dc_zero<RB>(acc);
            dc_mm_nk<RB>(S, RS, r, Ue, r, 16 * ct, D, acc, lane);
            const int col = 16 * ct + i;
            const float b = col < D ? a.bias[col] : 0.f;
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
              for (int v = 0; v < 4; ++v) {
                const int row = 16 * rb + 4 * gq + v;
                const float y = acc[rb][v] + b;
                dx0acc[c][rb][v] = fmaf(G[4 * row + e], y, dx0acc[c][rb][v]);
                float t = w[row * DS + col] * y;      // (the padding columns of w are zero)
                t += __shfl_xor(t, 1, 64);
                t += __shfl_xor(t, 2, 64);
                t += __shfl_xor(t, 4, 64);
                t += __shfl_xor(t, 8, 64);
                dgl[rb][v] += t;
              }
          }
        }
        if (i == 0) {
#pragma unroll
          for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int v = 0; v < 4; ++v) DGP[wave * TR + 16 * rb + 4 * gq + v] = dgl[rb][v];
        }
      }
      // dq = g_e (U_e^T w) (1 - s^2)
      for (int ct = wave; ct < g.RT; ct += 4) {
        dc_f32x4 acc[RB];
        dc_zero<RB>(acc);
        dc_mm_kn<RB>(w, DS, D, Ue, r, 16 * ct, r, acc, lane);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int row = 16 * rb + 4 * gq + v;
            const float s = S[row * RS + 16 * ct + i];
            Q[row * RS + 16 * ct + i] = G[4 * row + e] * acc[rb][v] * (1.f - s * s);
          }
      }
      __syncthreads();
      if (tid < TR) DG[4 * tid + e] = ((DGP[tid] + DGP[TR + tid]) + DGP[2 * TR + tid]) + DGP[3 * TR + tid];
      // dU_e += w^T (g_e s)
      for (int idx = wave; idx < g.CT * g.RT; idx += 4)
        dc_wgrad<RB>(w, DS, S, RS, G + e, 16 * (idx / g.RT), 16 * (idx % g.RT), pU + (int64_t)e * D * r, r, D, r, first, lane);
      __syncthreads();      // s is no longer needed: dp takes its place
      // dp = (C_e^T dq) (1 - t^2)
      for (int ct = wave; ct < g.RT; ct += 4) {
        dc_f32x4 acc[RB];
        dc_zero<RB>(acc);
        dc_mm_kn<RB>(Q, RS, r, Ce, r, 16 * ct, r, acc, lane);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int row = 16 * rb + 4 * gq + v;
            const float t = T[row * RS + 16 * ct + i];
            S[row * RS + 16 * ct + i] = acc[rb][v] * (1.f - t * t);
          }
      }
      __syncthreads();
      // dC_e += dq^T t, dV_e += xl^T dp, dXl += V_e dp
      for (int idx = wave; idx < g.RT * g.RT; idx += 4)
        dc_wgrad<RB>(Q, RS, T, RS, nullptr, 16 * (idx / g.RT), 16 * (idx % g.RT), pC + (int64_t)e * r * r, r, r, r, first, lane);
      for (int idx = wave; idx < g.CT * g.RT; idx += 4)
        dc_wgrad<RB>(xl, DS, S, RS, nullptr, 16 * (idx / g.RT), 16 * (idx % g.RT), pV + (int64_t)e * D * r, r, D, r, first, lane);
#pragma unroll
      for (int c = 0; c < MAXCT; ++c) {
        const int ct = wave + 4 * c;
        if (ct < g.CT) dc_mm_nk<RB>(S, RS, r, Ve, r, 16 * ct, D, dxlacc[c], lane);
      }
      __syncthreads();      // the next expert overwrites T and S
    }
    if (tid < TR) {
      float gd = 0.f;
#pragma unroll
      for (int e = 0; e < kDcMaxE; ++e)
        if (e < E) gd = fmaf(G[4 * tid + e], DG[4 * tid + e], gd);
#pragma unroll
      for (int e = 0; e < kDcMaxE; ++e) DZ[4 * tid + e] = e < E ? G[4 * tid + e] * (DG[4 * tid + e] - gd) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MAXCT; ++c) {
      const int ct = wave + 4 * c, col = 16 * ct + i;
      if (ct < g.CT && col < D) {
        float wg[kDcMaxE];
#pragma unroll
        for (int e = 0; e < kDcMaxE; ++e) wg[e] = e < E ? a.Wg[(int64_t)e * D + col] : 0.f;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int row = 16 * rb + 4 * gq + v;
            if (row < rows_valid) {
              const int64_t at = (row0 + row) * D + col;
              const float dv = a.dXn[at];
              float gate = 0.f;
#pragma unroll
              for (int e = 0; e < kDcMaxE; ++e) gate = fmaf(DZ[4 * row + e], wg[e], gate);
              a.dX0[at] = dv * dx0acc[c][rb][v];
              a.dXl[at] = (dv + dxlacc[c][rb][v]) + gate;
            }
          }
      }
    }
    // dbias, dWg, dbg: column sums over the tile's rows, kept in registers over the workgroup's tiles
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = tid + 256 * c;
      if (j < D)
        for (int row = 0; row < TR; ++row) {
          const float wv = w[row * DS + j], xv = xl[row * DS + j];
          float gs = 0.f;
#pragma unroll
          for (int e = 0; e < kDcMaxE; ++e) {
            if (e < E) gs += G[4 * row + e];
            dwgacc[c][e] = fmaf(DZ[4 * row + e], xv, dwgacc[c][e]);
          }
          dbacc[c] = fmaf(gs, wv, dbacc[c]);
        }
    }
    if (tid < E)
      for (int row = 0; row < TR; ++row) dbgacc += DZ[4 * row + tid];
    first = false;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = tid + 256 * c;
    if (j < D) {
      pb[j] = dbacc[c];
#pragma unroll
      for (int e = 0; e < kDcMaxE; ++e)
        if (e < E) pWg[(int64_t)e * D + j] = dwgacc[c][e];
    }
  }
  if (tid < E) pbg[tid] = dbgacc;
}

// one thread per element of dU | dV | dC | dbias | dWg | dbg: the workgroups' partials in workgroup order, in double
__global__ __launch_bounds__(kBlock) void dcnv2_grad_reduce_kernel(const float* __restrict__ part, int blocks, int64_t P, int64_t PS,
                                                                   int64_t nU, int64_t nC, int D, int E, float* __restrict__ dU,
                                                                   float* __restrict__ dV, float* __restrict__ dC, float* __restrict__ db,
                                                                   float* __restrict__ dWg, float* __restrict__ dbg) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= P) return;
  double acc = 0.0;
  for (int p = 0; p < blocks; ++p) acc += (double)part[p * PS + e];
  const float v = (float)acc;
  int64_t o = e;
  if (o < nU) { dU[o] = v; return; }
  o -= nU;
  if (o < nU) { dV[o] = v; return; }
  o -= nU;
  if (o < nC) { dC[o] = v; return; }
  o -= nC;
  if (o < D) { db[o] = v; return; }
  o -= D;
  if (o < (int64_t)E * D) { dWg[o] = v; return; }
  o -= (int64_t)E * D;
  dbg[o] = v;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
// the one statement of the envelope: every entry point checks it, rc_dcnv2_check_shape reports it to the host
static int dc_shape(const char* fn, int D, int r, int E) {
  if (D % 4 == 0 && D >= 8 && D <= 1024 && r % 4 == 0 && r >= 4 && r <= 128 && E >= 1 && E <= kDcMaxE) return RC_OK;
  return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (fields x emb_size a multiple of 4 in [8, 1024], low_rank a multiple of 4 in "
              "[4, 128], expert_num in [1, 4]): width=%d low_rank=%d expert_num=%d", fn, D, r, E);
}

static int dc_check(const char* fn, int64_t N, int D, int r, int E, bool bwd, DcGeom* g) {
  RC_TRY(dc_shape(fn, D, r, E));
  if (N < 1 || N > ((int64_t)1 << 24))
    return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (rows in [1, 2^24]): rows=%lld", fn, (long long)N);
  if (!dc_geometry(N, D, r, E, bwd, g)) return fail(RC_ERR_UNSUPPORTED, "%s: no tile fits the LDS for this shape", fn);
  return RC_OK;
}

template <int RB, int MAXCT>
static int dc_launch(const DcArgs& a, bool bwd, int blocks, hipStream_t st) {
  auto kern = bwd ? dcnv2_bwd_kernel<RB, MAXCT> : dcnv2_fwd_kernel<RB, MAXCT>;
  {
    static std::mutex mu;       // function attributes are per device: once per instantiation, pass and device of the process
    static bool done[2][64] = {};
    int dev = 0;
    RC_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || !done[bwd][dev]) {
      RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDcLdsBudget));
      if (dev >= 0 && dev < 64) done[bwd][dev] = true;
    }
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), a.g.lds, st, a);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

// MAXCT: the 16-wide column tiles of D one wave keeps accumulators for (a power of two >= CT / 4; RB MAXCT <= 16 by dc_geometry)
template <int RB>
static int dc_run_rb(const DcArgs& a, bool bwd, int blocks, hipStream_t st) {
  const int per_wave = (a.g.CT + 3) / 4;
  if constexpr (RB <= 1)
    if (per_wave > 8) return dc_launch<RB, 16>(a, bwd, blocks, st);
  if constexpr (RB <= 2)
    if (per_wave > 4) return dc_launch<RB, 8>(a, bwd, blocks, st);
  if (per_wave > 2) return dc_launch<RB, 4>(a, bwd, blocks, st);
  if (per_wave > 1) return dc_launch<RB, 2>(a, bwd, blocks, st);
  return dc_launch<RB, 1>(a, bwd, blocks, st);
}

static int dc_run(const DcArgs& a, bool bwd, int blocks, hipStream_t st) {
  return a.g.RB == 4 ? dc_run_rb<4>(a, bwd, blocks, st) : a.g.RB == 2 ? dc_run_rb<2>(a, bwd, blocks, st) : dc_run_rb<1>(a, bwd, blocks, st);
}

static int dc_fwd_impl(const float* X0, const float* Xl, const float* U, const float* V, const float* C, const float* bias, const float* Wg,
                       const float* bg, int64_t N, int D, int r, int E, float* Xnext, rc_stream_t stream) {
  const char* fn = "rc_dcnv2_mix_layer_fwd";
  DcGeom g;
  RC_TRY(dc_check(fn, N, D, r, E, false, &g));
  RC_REQUIRE(X0 != nullptr && Xl != nullptr && U != nullptr && V != nullptr && C != nullptr && bias != nullptr && Wg != nullptr &&
             bg != nullptr && Xnext != nullptr, "%s: null pointer", fn);
  RC_REQUIRE(aligned16(X0, Xl, U, V, C, bias, Wg, bg, Xnext), "%s: every tensor must be 16-byte aligned", fn);
  DcArgs a{X0, Xl, U, V, C, bias, Wg, bg, nullptr, Xnext, nullptr, nullptr, nullptr, N, g};
  return dc_run(a, false, dc_blocks(g, N, false), as_stream(stream));
}

static int dc_bwd_impl(const float* dXnext, const float* X0, const float* Xl, const float* U, const float* V, const float* C,
                       const float* bias, const float* Wg, const float* bg, int64_t N, int D, int r, int E, void* workspace, size_t ws_bytes,
                       float* dXl, float* dX0_part, float* dU, float* dV, float* dC, float* dbias, float* dWg, float* dbg,
                       rc_stream_t stream) {
  const char* fn = "rc_dcnv2_mix_layer_bwd";
  DcGeom g;
  RC_TRY(dc_check(fn, N, D, r, E, true, &g));
  RC_REQUIRE(dXnext != nullptr && X0 != nullptr && Xl != nullptr && U != nullptr && V != nullptr && C != nullptr && bias != nullptr &&
             Wg != nullptr && bg != nullptr && dXl != nullptr && dX0_part != nullptr && dU != nullptr && dV != nullptr && dC != nullptr &&
             dbias != nullptr && dWg != nullptr && dbg != nullptr, "%s: null pointer", fn);
  RC_REQUIRE(aligned16(dXnext, X0, Xl, U, V, C, bias, Wg, bg, dXl, dX0_part), "%s: every input, dXl and dX0_part must be 16-byte aligned", fn);
  RC_REQUIRE(workspace != nullptr && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "%s: workspace must be 256-byte aligned", fn);
  const int blocks = dc_blocks(g, N, true);
  Carver c(workspace);
  float* part = c.take<float>((size_t)blocks * g.PS);
  if (ws_bytes < c.off) return fail(RC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, c.off);
  const hipStream_t st = as_stream(stream);
  DcArgs a{X0, Xl, U, V, C, bias, Wg, bg, dXnext, nullptr, dXl, dX0_part, part, N, g};
  RC_TRY(dc_run(a, true, blocks, st));
  hipLaunchKernelGGL(dcnv2_grad_reduce_kernel, dim3((unsigned)((g.P + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, part, blocks, g.P, g.PS,
                     (int64_t)E * D * r, (int64_t)E * r * r, D, E, dU, dV, dC, dbias, dWg, dbg);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

}  // namespace rc

extern "C" enum rc_status rc_dcnv2_check_shape(int D, int low_rank, int expert_num) {
  using namespace rc;
  const char* fn = "rc_dcnv2_check_shape";
  const int rc_ = dc_shape(fn, D, low_rank, expert_num);
  if (rc_ != RC_OK) return (enum rc_status)rc_;
  DcGeom g;
  if (!dc_geometry(-1, D, low_rank, expert_num, true, &g) || !dc_geometry(-1, D, low_rank, expert_num, false, &g))
    return (enum rc_status)fail(RC_ERR_UNSUPPORTED, "%s: no tile fits the LDS for this shape", fn);
  return RC_OK;
}

extern "C" size_t rc_dcnv2_mix_layer_bwd_workspace_bytes(int64_t N, int D, int low_rank, int expert_num) {
  using namespace rc;
  DcGeom g;
  if (dc_check("rc_dcnv2_mix_layer_bwd_workspace_bytes", N, D, low_rank, expert_num, true, &g) != RC_OK) return 0;
  Carver c(nullptr);
  c.take<float>((size_t)dc_blocks(g, N, true) * g.PS);
  return c.off;
}

extern "C" enum rc_status rc_dcnv2_mix_layer_fwd(const float* X0, const float* Xl, const float* U, const float* V, const float* C,
                                                 const float* bias, const float* Wg, const float* bg, int64_t N, int D, int low_rank,
                                                 int expert_num, float* Xnext, rc_stream_t stream) {
  return (enum rc_status)rc::dc_fwd_impl(X0, Xl, U, V, C, bias, Wg, bg, N, D, low_rank, expert_num, Xnext, stream);
}

extern "C" enum rc_status rc_dcnv2_mix_layer_bwd(const float* dXnext, const float* X0, const float* Xl, const float* U, const float* V,
                                                 const float* C, const float* bias, const float* Wg, const float* bg, int64_t N, int D,
                                                 int low_rank, int expert_num, void* workspace, size_t ws_bytes, float* dXl,
                                                 float* dX0_part, float* dU, float* dV, float* dC, float* dbias, float* dWg, float* dbg,
                                                 rc_stream_t stream) {
  return (enum rc_status)rc::dc_bwd_impl(dXnext, X0, Xl, U, V, C, bias, Wg, bg, N, D, low_rank, expert_num, workspace, ws_bytes, dXl,
                                         dX0_part, dU, dV, dC, dbias, dWg, dbg, stream);
}
