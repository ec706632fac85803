// listenc_dev.hpp -- the device helpers, weight / gradient records and launch helper of the post-norm attention blocks over short lists:
// shared by listenc.hip (self-attention, PRM.py:64,90-92) and setmab.hip (query rows that are not the key rows, SetRank.py:29-56).
// Rows live in LDS padded to 16-row tiles; every product runs on v_mfma_f32_16x16x4_f32 (see listenc.hip's header for the layout).
#pragma once
#include <mutex>

#include "common.hpp"

namespace rc {

typedef float le_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kLeMaxBlocksBwd = 256;
constexpr int kLeMaxBlocksFwd = 1024;
constexpr size_t kLeLdsBudget = 160 * 1024;
constexpr size_t kLePartialBudget = (size_t)128 << 20;
constexpr float kLeEps = 1e-5f;

struct LeWeights {
  const float *Win, *bin, *Wo, *bo, *g1, *be1, *W1, *b1, *W2, *b2, *g2, *be2;
};

struct LeGrads {
  float *Win, *bin, *Wo, *bo, *g1, *be1, *W1, *b1, *W2, *b2, *g2, *be2;
};

// offsets of the twelve gradients inside one partial, in floats (all multiples of 16)
struct LeOffsets {
  int64_t Win, Wo, W1, W2, bin, bo, g1, be1, b1, b2, g2, be2, end;
};

__host__ __device__ inline LeOffsets le_offsets(int d, int dff) {
  LeOffsets o;
  o.Win = 0;
  o.Wo = 3 * (int64_t)d * d;
  o.W1 = o.Wo + (int64_t)d * d;
  o.W2 = o.W1 + (int64_t)dff * d;
  o.bin = o.W2 + (int64_t)dff * d;
  o.bo = o.bin + 3 * d;
  o.g1 = o.bo + d;
  o.be1 = o.g1 + d;
  o.b1 = o.be1 + d;
  o.b2 = o.b1 + dff;
  o.g2 = o.b2 + d;
  o.be2 = o.g2 + d;
  o.end = o.be2 + d;
  return o;
}

// ---- device pieces -----------------------------------------------------------------------------------------------------------------
#define LE_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

template <int RT>
__device__ __forceinline__ void le_zero(le_f32x4 (&acc)[RT]) {
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = le_f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc[rt][v] += sum_k in[16 rt + 4 g + v][k] W[(n0 + i) ldw + k] over k in [0, K), K % 16 == 0; lane = 16 g + i
template <int RT>
__device__ __forceinline__ void le_mm_nk(const float* in, int ins, int K, const float* __restrict__ W, int ldw, int n0,
                                         le_f32x4 (&acc)[RT], int lane) {
  const int i = lane & 15, g = lane >> 4;
  const float* wp = W + (int64_t)(n0 + i) * ldw + 4 * g;
  const float* ip = in + i * ins + 4 * g;
#pragma unroll 2
  for (int k0 = 0; k0 < K; k0 += 16) {
    const float4 b = *reinterpret_cast<const float4*>(wp + k0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const float4 x = *reinterpret_cast<const float4*>(ip + rt * 16 * ins + k0);
      acc[rt] = LE_MFMA(x.x, b.x, acc[rt]);
      acc[rt] = LE_MFMA(x.y, b.y, acc[rt]);
      acc[rt] = LE_MFMA(x.z, b.z, acc[rt]);
      acc[rt] = LE_MFMA(x.w, b.w, acc[rt]);
    }
  }
}

// acc[rt][v] += sum_k in[16 rt + 4 g + v][k] W[k ldw + n0 + i] over k in [0, K), K % 4 == 0
template <int RT>
__device__ __forceinline__ void le_mm_kn(const float* in, int ins, int K, const float* __restrict__ W, int ldw, int n0,
                                         le_f32x4 (&acc)[RT], int lane) {
  const int i = lane & 15, g = lane >> 4;
  const float* wp = W + (int64_t)g * ldw + n0 + i;
  const float* ip = in + i * ins + g;
#pragma unroll 4
  for (int k0 = 0; k0 < K; k0 += 4) {
    const float b = wp[(int64_t)k0 * ldw];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = LE_MFMA(ip[rt * 16 * ins + k0], b, acc[rt]);
  }
}

// MODE 0: out = in W^T + b;  1: relu of it;  2: resid + it.  W [N, K] row-major, every wave takes column tiles wave, wave + 4, ...
template <int RT, int MODE>
__device__ __forceinline__ void le_linear(const float* in, int ins, int K, const float* __restrict__ W, const float* __restrict__ bias,
                                          int N, float* out, int outs, const float* resid, int rs, int wave, int lane) {
  const int i = lane & 15, g = lane >> 4;
  for (int ct = wave; ct < N / 16; ct += 4) {
    le_f32x4 acc[RT];
    le_zero<RT>(acc);
    le_mm_nk<RT>(in, ins, K, W, K, 16 * ct, acc, lane);
    const int col = 16 * ct + i;
    const float b = bias[col];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 16 * rt + 4 * g + v;
        float y = acc[rt][v] + b;
        if (MODE == 1) y = fmaxf(y, 0.f);
        if (MODE == 2) y += resid[row * rs + col];
        out[row * outs + col] = y;
      }
  }
}

// this lane's two columns (lane, lane + 64) of one row, its mean and 1 / sqrt(var + eps): a wave per row
__device__ __forceinline__ void le_row_stats(const float* zr, int d, int lane, float (&x)[2], float& mu, float& rstd) {
  x[0] = lane < d ? zr[lane] : 0.f;
  x[1] = lane + 64 < d ? zr[lane + 64] : 0.f;
  mu = wave_allreduce_sum(x[0] + x[1]) / (float)d;
  const float c0 = lane < d ? x[0] - mu : 0.f, c1 = lane + 64 < d ? x[1] - mu : 0.f;
  const float var = wave_allreduce_sum(c0 * c0 + c1 * c1) / (float)d;
  rstd = 1.f / sqrtf(var + kLeEps);
}

// softmax over the NP entries of each of the 16 rows of S, four lanes a row (every list has a valid key: the maximum is finite)
__device__ __forceinline__ void le_softmax(float* S, int SS, int NP, int lane) {
  float* row = S + (lane >> 2) * SS;
  const int q = lane & 3;
  float m = -INFINITY;
  for (int j = q; j < NP; j += 4) m = fmaxf(m, row[j]);
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  m = fmaxf(m, __shfl_xor(m, 2, 64));
  float l = 0.f;
  for (int j = q; j < NP; j += 4) {
    const float e = expf(row[j] - m);
    row[j] = e;
    l += e;
  }
  l += __shfl_xor(l, 1, 64);
  l += __shfl_xor(l, 2, 64);
  for (int j = q; j < NP; j += 4) row[j] = row[j] / l;
}

// out[16 rt + r][h dk + c] = sum_j S[r][j] V[j][h dk + c], c in [0, dk)
__device__ __forceinline__ void le_pv(const float* S, int SS, int NP, const float* V, int vs, int dk, int h, int rt, float* out, int os,
                                      int lane) {
  const int i = lane & 15, g = lane >> 4;
  for (int c0 = 0; c0 < dk; c0 += 16) {
    const bool ok = c0 + i < dk;
    const float* vp = V + g * vs + h * dk + c0 + (ok ? i : 0);
    le_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < NP; j0 += 4) acc = LE_MFMA(S[i * SS + j0 + g], ok ? vp[j0 * vs] : 0.f, acc);
    if (ok) {
#pragma unroll
      for (int v = 0; v < 4; ++v) out[(16 * rt + 4 * g + v) * os + h * dk + c0 + i] = acc[v];
    }
  }
}

// one 16x16 tile of dW[a0.., b0..] += sum over rows of L[row][a0 + i] R[row][b0 + i]
__device__ __forceinline__ le_f32x4 le_wtile(const float* L, int ls, const float* R, int rs, int rows, int a0, int b0, le_f32x4 acc, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const float* lp = L + g * ls + a0 + i;
  const float* rp = R + g * rs + b0 + i;
#pragma unroll 4
  for (int row0 = 0; row0 < rows; row0 += 4) acc = LE_MFMA(lp[row0 * ls], rp[row0 * rs], acc);
  return acc;
}

__device__ __forceinline__ void le_wstore(float* out, int ld, int a0, int b0, const le_f32x4& acc, bool first, int lane) {
  const int i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    float* p = out + (int64_t)(a0 + 4 * g + v) * ld + b0 + i;
    *p = first ? acc[v] : *p + acc[v];
  }
}

// the weight gradient of one matrix [16 AT, 16 BT]: resident (AT, BT > 0, the tiles wave, wave + 4, ... in wacc) or into the partial
template <int AT, int BT>
__device__ __forceinline__ void le_wgrad(const float* L, int ls, const float* R, int rs, int rows, int at, int bt, float* out, bool first,
                                         le_f32x4* wacc, int wave, int lane) {
  if constexpr (AT > 0) {
#pragma unroll
    for (int t = 0; t < (AT * BT + 3) / 4; ++t) {
      const int idx = wave + 4 * t;
      if (idx < AT * BT) wacc[t] = le_wtile(L, ls, R, rs, rows, 16 * (idx / BT), 16 * (idx % BT), wacc[t], lane);
    }
  } else {
    for (int idx = wave; idx < at * bt; idx += 4) {
      const int a0 = 16 * (idx / bt), b0 = 16 * (idx % bt);
      le_wstore(out, 16 * bt, a0, b0, le_wtile(L, ls, R, rs, rows, a0, b0, le_f32x4{0.f, 0.f, 0.f, 0.f}, lane), first, lane);
    }
  }
}

template <int AT, int BT>
__device__ __forceinline__ void le_wflush(float* out, le_f32x4* wacc, int wave, int lane) {
#pragma unroll
  for (int t = 0; t < (AT * BT + 3) / 4; ++t) {
    const int idx = wave + 4 * t;
    if (idx < AT * BT) le_wstore(out, 16 * BT, 16 * (idx / BT), 16 * (idx % BT), wacc[t], true, lane);
  }
}

__device__ __forceinline__ float le_colsum(const float* M, int ms, int rows, int col) {
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += M[r * ms + col];
  return s;
}

// one thread per element of the twelve gradients: the workgroups' partials in workgroup order, in double
static __global__ __launch_bounds__(kBlock) void listenc_grad_reduce_kernel(const float* __restrict__ part, int blocks, int64_t PS, LeOffsets o,
                                                                     LeGrads out) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= o.end) return;
  double acc = 0.0;
  for (int p = 0; p < blocks; ++p) acc += (double)part[p * PS + e];
  const float v = (float)acc;
  if (e < o.Wo) out.Win[e] = v;
  else if (e < o.W1) out.Wo[e - o.Wo] = v;
  else if (e < o.W2) out.W1[e - o.W1] = v;
  else if (e < o.bin) out.W2[e - o.W2] = v;
  else if (e < o.bo) out.bin[e - o.bin] = v;
  else if (e < o.g1) out.bo[e - o.bo] = v;
  else if (e < o.be1) out.g1[e - o.g1] = v;
  else if (e < o.b1) out.be1[e - o.be1] = v;
  else if (e < o.b2) out.b1[e - o.b1] = v;
  else if (e < o.g2) out.b2[e - o.b2] = v;
  else if (e < o.be2) out.g2[e - o.g2] = v;
  else out.be2[e - o.be2] = v;
}

template <class K, class A>
inline int le_launch(K kern, int slot, const A& a, size_t lds, int blocks, hipStream_t st) {
  {
    static std::mutex mu;       // function attributes are per device: once per instantiation and device of the process
    static bool done[16][64] = {};
    int dev = 0;
    RC_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || !done[slot][dev]) {
      RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLeLdsBudget));
      if (dev >= 0 && dev < 64) done[slot][dev] = true;
    }
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, st, a);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

inline bool le_weights_ok(const LeWeights& w) {
  return w.Win != nullptr && w.bin != nullptr && w.Wo != nullptr && w.bo != nullptr && w.g1 != nullptr && w.be1 != nullptr &&
         w.W1 != nullptr && w.b1 != nullptr && w.W2 != nullptr && w.b2 != nullptr && w.g2 != nullptr && w.be2 != nullptr &&
         aligned16(w.Win, w.bin, w.Wo, w.bo, w.g1, w.be1, w.W1, w.b1, w.W2, w.b2, w.g2, w.be2);
}

}  // namespace rc
