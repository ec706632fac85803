// din.hip -- DIN's target attention (Zhou et al., KDD 2018; reference models/context_seq/DIN.py:63-95): for instance n = (b, c) and
// history position l, s[n, l] = att_mlp(cat[q, k, q - k, q * k]) with Linear -> Sigmoid -> Dropout hidden layers and Linear(., 1),
//     w[n, l] = (l < len_b ? s[n, l] : 0) / sqrt(H),      out[n] = sum_l w[n, l] keys[b, l].
// No tensor of N L 4H or N L A elements exists: a workgroup owns a TILE of 64 rows r = (c, l) = c * L + l of ONE batch row b
// (CT = max(1, 64 / L) candidates) and keeps every layer's activation of the tile in LDS.
//
// First layer, folded: with W_1 = [Wq | Wk | Wd | Wp],  z_1 = (Wq + Wd) q + (Wk - Wd) k + Wp (q o k) + b_1.  The q term is one
// product over the tile's CT candidates, the k term one over the row's L positions (shared by the tile's candidates), only the Wp
// term runs over all 64 rows.  All three are v_mfma_f32_16x16x4_f32 products over H in chunks of 16: the operand rows are staged in
// LDS chunk by chunk, the weights are read from global memory as float4 along the reduction (MFMA e of a chunk contracts
// h = h0 + 4 g + e, so both operands are one 16-byte read per lane), the folds are formed in the load.  A wave takes the column tiles
// nt = wave, wave + 4, ... of all row tiles, so a weight element is read once per workgroup.
// The later layers, the output layer, mask, scale and the weighted key sum follow in the same launch.
//
//   din_fwd_kernel      one tile per workgroup
//   din_bwd_kernel      persistent: workgroup g owns batch rows g, g + G, ... and ALL their tiles, recomputes the forward, and walks
//                       back: the tile's dz_j live in LDS beside the h_j; dq is complete per tile; dkeys[b] is accumulated by the one
//                       owner in tile order; every parameter gradient is accumulated in the workgroup's own slice of the workspace
//                       (same lane, same element, every time).  The first layer folds back: dz_1 summed over l (per candidate)
//                       against q, summed over the tile's candidates (per position) against k.
//   din_reduce_kernel   sums the G slices in workgroup order and unfolds dWq = dWqd, dWk = dWkd, dWd = dWqd - dWkd
// No atomics; every sum has a fixed order, so two runs are bit-equal.
#include <mutex>

#include "common.hpp"
#include "philox.hpp"

namespace rc {

typedef float din_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kDinRows = 64;        // rows (c, l) of a tile
constexpr int kDinKC = 16;          // reduction chunk of the first layer
constexpr int kDinLdC = 20;         // row stride of a staged chunk
constexpr int kDinBufRows = 65;     // L + CT <= 65: the k-term rows and the q-term rows share one activation-sized buffer
constexpr int kDinMaxLayers = 3;
constexpr int kDinMaxSum = 256;     // sum of the hidden widths: the tile's h_j (and dz_j) of every layer sit side by side in LDS
constexpr size_t kDinLdsBudget = 160 * 1024;

enum { kStageK = 0, kStageQ = 1, kStageU = 2, kStageG = 3 };

struct DinArgs {
  const float* q;
  const float* keys;
  const int64_t* lengths;
  const float* W[kDinMaxLayers];
  const float* bias[kDinMaxLayers];
  const float* w_out;
  const float* b_out;
  int A[kDinMaxLayers], off[kDinMaxLayers];
  int n_layers, SA, ld;
  int B, C, L, H, CT, tiles_per_row;
  float inv_sqrt_h;
  const uint64_t* seed;
  uint32_t drop_thresh, site0;
  float keep_scale;
  float* out;
  int64_t ld_out;
  float* att;
  // backward
  const float* d_out;
  float* dq;
  float* dkeys;
  float* partial;     // [G][P]
  int64_t P;
  int64_t poff_w[kDinMaxLayers], poff_b[kDinMaxLayers], poff_wout, poff_bout;   // offsets inside a slice
};

struct DinCtx {
  int b;          // batch row
  int64_t n0;     // first instance of the tile
  int ct;         // candidates in the tile
  int rows;       // ct * L
  int len;        // min(max(len_b, 0), L)
};

// The thread index, opaque at every use: what depends on it is computed where it is used.  Read as threadIdx.x, the address arithmetic
// of every phase of the backward was hoisted out of its row and tile loops as loop invariants and stayed live across all of them
// (330 spilled registers).
__device__ __forceinline__ int din_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

__device__ __forceinline__ float4 din_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ DinCtx din_ctx(const DinArgs& a, int b, int tile) {
  DinCtx cx;
  cx.b = b;
  const int c0 = tile * a.CT;
  cx.ct = min(a.CT, a.C - c0);
  cx.n0 = (int64_t)b * a.C + c0;
  cx.rows = cx.ct * a.L;
  const int64_t len = a.lengths[b];
  cx.len = (int)(len < 0 ? 0 : (len > a.L ? a.L : len));
  return cx;
}

// one chunk [64][16] of operand rows into LDS; everything outside the valid rows / positions / width is 0 and never read
__device__ __forceinline__ void din_stage(const DinArgs& a, const DinCtx& cx, int mode, int h0, float* dst) {
  const int t = din_tid(), row = t >> 2, h = h0 + 4 * (t & 3);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (h < a.H) {
    if (mode == kStageK) {
      if (row < cx.len) v = din_ld4(a.keys + ((int64_t)cx.b * a.L + row) * a.H + h);
    } else if (mode == kStageQ) {
      if (row < cx.ct) v = din_ld4(a.q + (cx.n0 + row) * a.H + h);
    } else if (mode == kStageG) {
      if (row < cx.ct) v = din_ld4(a.d_out + (cx.n0 + row) * a.H + h);
    } else {
      if (row < cx.rows) {
        const int c = row / a.L, l = row - c * a.L;
        if (l < cx.len) {
          const float4 k = din_ld4(a.keys + ((int64_t)cx.b * a.L + l) * a.H + h);
          const float4 qv = din_ld4(a.q + (cx.n0 + c) * a.H + h);
          v = make_float4(qv.x * k.x, qv.y * k.y, qv.z * k.z, qv.w * k.w);
        }
      }
    }
  }
  *reinterpret_cast<float4*>(dst + row * kDinLdC + 4 * (t & 3)) = v;
}

// acc[mt][j] += X[16 mt + i][4 g + e] * Wf[16 nt + i][kb + 4 g + e], nt = wave + 4 j, Wf = Wa + sgn Wb (Wb may be null)
__device__ __forceinline__ void din_mm_chunk(din_f32x4 (&acc)[4][4], const float* Xs, int ldx, int MT, const float* Wa, const float* Wb,
                                             float sgn, int ldw, int kb, int K, int NT) {
  const int t = din_tid(), lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), i = lane & 15, g = lane >> 4;
  const bool kin = kb + 4 * g < K;
  float4 av[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    av[mt] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mt < MT) av[mt] = din_ld4(Xs + (16 * mt + i) * ldx + 4 * g);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nt = wave + 4 * j;
    if (nt < NT) {
      float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kin) {
        const int64_t o = (int64_t)(16 * nt + i) * ldw + kb + 4 * g;
        bv = din_ld4(Wa + o);
        if (Wb != nullptr) {
          const float4 c = din_ld4(Wb + o);
          bv = make_float4(bv.x + sgn * c.x, bv.y + sgn * c.y, bv.z + sgn * c.z, bv.w + sgn * c.w);
        }
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        if (mt < MT) {
          acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].x, bv.x, acc[mt][j], 0, 0, 0);
          acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].y, bv.y, acc[mt][j], 0, 0, 0);
          acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].z, bv.z, acc[mt][j], 0, 0, 0);
          acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].w, bv.w, acc[mt][j], 0, 0, 0);
        }
      }
    }
  }
}

// keep-and-scale factor of hidden unit `col` of layer `layer` at row m = n L + l: rc_linear_fwd's rule
__device__ __forceinline__ float din_keep(const DinArgs& a, uint64_t seed, int64_t m, int layer, int col) {
  if (a.seed == nullptr) return 1.f;
  uint32_t w[4];
  philox4x32_10(seed, (uint64_t)(m >> 2), (a.site0 + (uint32_t)layer) * 65536u + (uint32_t)col, w);
  const int e = (int)(m & 3);
  const uint32_t word = e == 0 ? w[0] : (e == 1 ? w[1] : (e == 2 ? w[2] : w[3]));
  return word < a.drop_thresh ? 0.f : a.keep_scale;
}

// a finished product into LDS: acc[mt][j][r] is element (row 16 mt + 4 g + r, column 16 (wave + 4 j) + i); rows < limit are stored
__device__ __forceinline__ void din_store_acc(din_f32x4 (&acc)[4][4], int NT, float* dst, int ld, int limit) {
  const int t = din_tid(), lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nt = wave + 4 * j;
    if (nt >= NT) continue;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * mt + 4 * g + r;
        if (row < limit) dst[row * ld + 16 * nt + i] = acc[mt][j][r];
      }
    }
  }
}

// z_j -> h_j = dropout(sigmoid(z_j + ...)) in place, one element per thread and trip (the products above leave the bare sums: with
// the 64 elements of a lane activated in the product's epilogue, their Philox states and k / q term reads spilled).  Layer 0 adds the
// k term of its position, the q term of its candidate and b_1; rows past the tile become 0 (their dz must be 0, not 0 * garbage).
__device__ __forceinline__ void din_activate(const DinArgs& a, const DinCtx& cx, int layer, float* Hs, const float* Ds, uint64_t seed) {
  const int A = a.A[layer];
#pragma unroll 1
  for (int idx = din_tid(); idx < kDinRows * A; idx += kBlock) {
    const int row = idx / A, col = idx - row * A;
    float* p = Hs + row * a.ld + a.off[layer] + col;
    float h = 0.f;
    if (row < cx.rows) {
      float v = *p;
      if (layer == 0) {
        const int c = row / a.L, l = row - c * a.L;
        v = (v + Ds[l * a.ld + col]) + Ds[(a.L + c) * a.ld + col];
      }
      v += a.bias[layer][col];
      h = sigmoidf_(v) * din_keep(a, seed, cx.n0 * a.L + row, layer, col);
    }
    *p = h;
  }
}

#define DIN_ZERO_ACC(acc)                                     \
  _Pragma("unroll") for (int mt_ = 0; mt_ < 4; ++mt_)         \
  _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) acc[mt_][j_] = din_f32x4{0.f, 0.f, 0.f, 0.f};

// The forward of one tile: h_j of every layer into Hs, the masked, scaled weights into wts[64] (0 on rows past the tile, past len).
// Xs: a [64][kDinLdC] staging buffer; Ds: scratch for the k and q terms.
__device__ __forceinline__ void din_tile_forward(const DinArgs& a, const DinCtx& cx, float* Hs, float* Ds, float* Xs, float* wts,
                                                 uint64_t seed) {
  const int H = a.H, ldw = 4 * H, NT0 = a.A[0] / 16;
  din_f32x4 acc[4][4];
  // k term: (Wk - Wd) k_l for the row's positions
  DIN_ZERO_ACC(acc)
#pragma unroll 1
  for (int h0 = 0; h0 < H; h0 += kDinKC) {
    din_stage(a, cx, kStageK, h0, Xs);
    __syncthreads();
    din_mm_chunk(acc, Xs, kDinLdC, (a.L + 15) / 16, a.W[0] + H, a.W[0] + 2 * H, -1.f, ldw, h0, H, NT0);
    __syncthreads();
  }
  din_store_acc(acc, NT0, Ds, a.ld, a.L);
  // q term: (Wq + Wd) q_c + b_1 for the tile's candidates
  DIN_ZERO_ACC(acc)
#pragma unroll 1
  for (int h0 = 0; h0 < H; h0 += kDinKC) {
    din_stage(a, cx, kStageQ, h0, Xs);
    __syncthreads();
    din_mm_chunk(acc, Xs, kDinLdC, (cx.ct + 15) / 16, a.W[0], a.W[0] + 2 * H, 1.f, ldw, h0, H, NT0);
    __syncthreads();
  }
  din_store_acc(acc, NT0, Ds + a.L * a.ld, a.ld, cx.ct);
  // Wp (q o k) for every row, then z_1 -> h_1
  DIN_ZERO_ACC(acc)
#pragma unroll 1
  for (int h0 = 0; h0 < H; h0 += kDinKC) {
    din_stage(a, cx, kStageU, h0, Xs);
    __syncthreads();
    din_mm_chunk(acc, Xs, kDinLdC, 4, a.W[0] + 3 * H, nullptr, 0.f, ldw, h0, H, NT0);
    __syncthreads();
  }
  din_store_acc(acc, NT0, Hs, a.ld, kDinRows);
  __syncthreads();
  din_activate(a, cx, 0, Hs, Ds, seed);
  __syncthreads();
#pragma unroll 1
  for (int j = 1; j < a.n_layers; ++j) {
    const int K = a.A[j - 1];
    DIN_ZERO_ACC(acc)
#pragma unroll 1
    for (int k0 = 0; k0 < K; k0 += kDinKC)
      din_mm_chunk(acc, Hs + a.off[j - 1] + k0, a.ld, 4, a.W[j], nullptr, 0.f, K, k0, K, a.A[j] / 16);
    din_store_acc(acc, a.A[j] / 16, Hs + a.off[j], a.ld, kDinRows);
    __syncthreads();
    din_activate(a, cx, j, Hs, Ds, seed);
    __syncthreads();
  }
  // output layer, mask, scale: four threads per row
  {
    const int t = din_tid(), row = t >> 2, part = t & 3, last = a.n_layers - 1, AL = a.A[last];
    const float* h = Hs + row * a.ld + a.off[last];
    float s = 0.f;
    for (int k = 4 * part; k < AL; k += 16) s += dot4(din_ld4(h + k), din_ld4(a.w_out + k));
    s = row_allreduce_sum<4>(s);
    if (part == 0) {
      bool valid = row < cx.rows;
      if (valid) valid = (row % a.L) < cx.len;
      wts[row] = valid ? (s + a.b_out[0]) * a.inv_sqrt_h : 0.f;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void din_fwd_kernel(DinArgs a) {
  extern __shared__ __attribute__((aligned(16))) float din_lds[];
  float* Hs = din_lds;
  float* Ds = Hs + kDinBufRows * a.ld;
  float* Xs = Ds + kDinBufRows * a.ld;
  float* wts = Xs + kDinRows * kDinLdC;
  const int b = blockIdx.x / a.tiles_per_row, tile = blockIdx.x % a.tiles_per_row;
  const DinCtx cx = din_ctx(a, b, tile);
  const uint64_t seed = a.seed ? *a.seed : 0;
  din_tile_forward(a, cx, Hs, Ds, Xs, wts, seed);
  if (a.att != nullptr)
    for (int r = din_tid(); r < cx.rows; r += kBlock) a.att[cx.n0 * a.L + r] = wts[r];
  // out[n] = sum_{l < len} w[n, l] keys[b, l]: a float4 of one candidate per thread
  const int H4 = a.H / 4;
  for (int idx = din_tid(); idx < cx.ct * H4; idx += kBlock) {
    const int c = idx / H4, h4 = idx - c * H4;
    const float* kp = a.keys + (int64_t)cx.b * a.L * a.H + 4 * h4;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l = 0; l < cx.len; ++l) {
      const float w = wts[c * a.L + l];
      const float4 k = din_ld4(kp + (int64_t)l * a.H);
      o.x = fmaf(w, k.x, o.x); o.y = fmaf(w, k.y, o.y); o.z = fmaf(w, k.z, o.z); o.w = fmaf(w, k.w, o.w);
    }
    *reinterpret_cast<float4*>(a.out + (cx.n0 + c) * a.ld_out + 4 * h4) = o;
  }
}

// ---- backward pieces ---------------------------------------------------------------------------------------------------------------
// d sigmoid-and-dropout: h = keep * s, so d h / d z = keep * s (1 - s); a dropped (or padded) unit has h = 0
__device__ __forceinline__ float din_dact(const DinArgs& a, float h) {
  if (!(h > 0.f)) return 0.f;
  const float ks = a.seed ? a.keep_scale : 1.f;
  const float s = a.seed ? h / ks : h;
  return ks * (s * (1.f - s));
}

// part[aa * ldp + col0 + 16 nt + i] (+)= sum_{r < nrows} Dz[r][aa] * X[r][16 nt + i]   (aa < A, NTo column tiles, columns < colmax)
__device__ __forceinline__ void din_dw(const float* Dz, int ldz, int A, const float* X, int ldx, int NTo, int nrows, float* part, int ldp,
                                       int col0, int colmax, bool first) {
  const int t = din_tid(), lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), i = lane & 15, g = lane >> 4;
  const int tiles = (A / 16) * NTo, nsteps = (nrows + 3) / 4;
#pragma unroll 1
  for (int tt = wave; tt < tiles; tt += 4) {
    const int mt = tt / NTo, nt = tt - mt * NTo;
    din_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int s = 0; s < nsteps; ++s) {
      const int r = 4 * s + g;
      float av = 0.f, bv = 0.f;
      if (r < nrows) {
        av = Dz[r * ldz + 16 * mt + i];
        bv = X[r * ldx + 16 * nt + i];
      }
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
    const int cc = col0 + 16 * nt + i;
    if (cc < colmax) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* p = part + (int64_t)(16 * mt + 4 * g + r) * ldp + cc;
        *p = (first ? 0.f : *p) + acc[r];
      }
    }
  }
}

// one 16 x 16 tile of Dz Wf: element (mrow0 + 4 g + r, col) for this lane's col, Wf[a][col] = Wa + sgn Wb
__device__ __forceinline__ din_f32x4 din_dx_tile(const float* Dz, int ldz, int A, int mrow0, const float* Wa, const float* Wb, float sgn,
                                                 int ldw, int col, bool col_ok) {
  const int lane = din_tid() & 63, i = lane & 15, g = lane >> 4;
  din_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int a0 = 0; a0 < A; a0 += 16) {
    const float4 av = din_ld4(Dz + (mrow0 + i) * ldz + a0 + 4 * g);
    float bv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bv[e] = 0.f;
      if (col_ok) {
        const int64_t o = (int64_t)(a0 + 4 * g + e) * ldw + col;
        bv[e] = Wa[o];
        if (Wb != nullptr) bv[e] += sgn * Wb[o];
      }
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv[3], acc, 0, 0, 0);
  }
  return acc;
}

// part[k] (+)= sum_{r < 64} Dz[r][k], k < A: one thread per column, rows in order
__device__ __forceinline__ void din_colsum(const float* Dz, int ldz, int A, float* part, bool first) {
  for (int k = din_tid(); k < A; k += kBlock) {
    float s = 0.f;
#pragma unroll 4
    for (int r = 0; r < kDinRows; ++r) s += Dz[r * ldz + k];
    part[k] = (first ? 0.f : part[k]) + s;
  }
}

__global__ __launch_bounds__(kBlock) void din_bwd_kernel(DinArgs a, int G) {
  extern __shared__ __attribute__((aligned(16))) float din_lds[];
  float* Hs = din_lds;                                  // h_j of the tile; later rows [0, L): dz_1 summed over c, rows [L, L + ct): over l
  float* Ds = Hs + kDinBufRows * a.ld;                  // forward scratch; then dz_j of the tile
  float* Ks = Ds + kDinBufRows * a.ld;                  // staged chunks
  float* Qs = Ks + kDinRows * kDinLdC;
  float* Us = Qs + kDinRows * kDinLdC;                  // q o k, then dU
  float* Gs = Us + kDinRows * kDinLdC;                  // d_out
  float* Fs = Gs + kDinRows * kDinLdC;                  // [66][kDinLdC]: folded dk rows [0, L), folded dq rows [L, L + ct)
  float* wts = Fs + (kDinBufRows + 1) * kDinLdC;
  float* dss = wts + kDinRows;
  const int H = a.H, L = a.L, ld = a.ld, A0 = a.A[0], last = a.n_layers - 1, AL = a.A[last];
  const uint64_t seed = a.seed ? *a.seed : 0;
  float* part = a.partial + (int64_t)blockIdx.x * a.P;
  bool first = true;

#pragma unroll 1
  for (int b = blockIdx.x; b < a.B; b += G) {
#pragma unroll 1
    for (int tile = 0; tile < a.tiles_per_row; ++tile) {
      const DinCtx cx = din_ctx(a, b, tile);
      const bool first_of_row = tile == 0;
      const int t = din_tid(), lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), i = lane & 15, g = lane >> 4;
      din_tile_forward(a, cx, Hs, Ds, Us, wts, seed);

      // d w[n, l] = d_out[n] . keys[b, l] on valid positions; d s = d w / sqrt(H)
      {
        const int row = t >> 2, part4 = t & 3;
        bool valid = row < cx.rows;
        const int c = valid ? row / L : 0, l = row - c * L;
        valid = valid && l < cx.len;
        float s = 0.f;
        if (valid) {
          const float* kp = a.keys + ((int64_t)cx.b * L + l) * H;
          const float* gp = a.d_out + (cx.n0 + c) * H;
          for (int h = 4 * part4; h < H; h += 16) s += dot4(din_ld4(kp + h), din_ld4(gp + h));
        }
        s = row_allreduce_sum<4>(s);
        if (part4 == 0) dss[row] = valid ? s * a.inv_sqrt_h : 0.f;
      }
      __syncthreads();
      // output layer: db_out, dw_out, dz of the last hidden layer
      if (t == 0) {
        float s = 0.f;
#pragma unroll 4
        for (int r = 0; r < kDinRows; ++r) s += dss[r];
        part[a.poff_bout] = (first ? 0.f : part[a.poff_bout]) + s;
      }
      for (int k = t; k < AL; k += kBlock) {
        float s = 0.f;
#pragma unroll 4
        for (int r = 0; r < kDinRows; ++r) s += dss[r] * Hs[r * ld + a.off[last] + k];
        part[a.poff_wout + k] = (first ? 0.f : part[a.poff_wout + k]) + s;
      }
      for (int idx = t; idx < kDinRows * AL; idx += kBlock) {
        const int r = idx / AL, k = idx - r * AL;
        Ds[r * ld + a.off[last] + k] = (dss[r] * a.w_out[k]) * din_dact(a, Hs[r * ld + a.off[last] + k]);
      }
      __syncthreads();
      // hidden layers j = last .. 1: db_j, dW_j, dz_{j-1}
#pragma unroll 1
      for (int j = last; j >= 1; --j) {
        const int Aj = a.A[j], K = a.A[j - 1];
        din_colsum(Ds + a.off[j], ld, Aj, part + a.poff_b[j], first);
        din_dw(Ds + a.off[j], ld, Aj, Hs + a.off[j - 1], ld, K / 16, kDinRows, part + a.poff_w[j], K, 0, K, first);
#pragma unroll 1
        for (int nt = 0; nt < K / 16; ++nt) {
          const int col = 16 * nt + i;
          const din_f32x4 acc = din_dx_tile(Ds + a.off[j], ld, Aj, 16 * wave, a.W[j], nullptr, 0.f, K, col, true);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * wave + 4 * g + r;
            Ds[row * ld + a.off[j - 1] + col] = acc[r] * din_dact(a, Hs[row * ld + a.off[j - 1] + col]);
          }
        }
        __syncthreads();
      }
      din_colsum(Ds, ld, A0, part + a.poff_b[0], first);
      __syncthreads();      // every read of Hs is done
      // fold dz_1: rows [0, L) summed over the tile's candidates, rows [L, L + ct) summed over the positions
      for (int idx = t; idx < (L + cx.ct) * A0; idx += kBlock) {
        const int r = idx / A0, k = idx - r * A0;
        float s = 0.f;
        if (r < L) {
          for (int c = 0; c < cx.ct; ++c) s += Ds[(c * L + r) * ld + k];
        } else {
          for (int l = 0; l < L; ++l) s += Ds[((r - L) * L + l) * ld + k];
        }
        Hs[r * ld + k] = s;
      }
      __syncthreads();

      const float* W0 = a.W[0];
      const int ldw = 4 * H;
      float* pWqd = part + a.poff_w[0];
      float* pWkd = pWqd + (int64_t)A0 * H;
      float* pWp = pWkd + (int64_t)A0 * H;
#pragma unroll 1
      for (int h0 = 0; h0 < H; h0 += kDinKC) {
        din_stage(a, cx, kStageK, h0, Ks);
        din_stage(a, cx, kStageQ, h0, Qs);
        din_stage(a, cx, kStageG, h0, Gs);
        din_stage(a, cx, kStageU, h0, Us);
        __syncthreads();
        din_dw(Ds, ld, A0, Us, kDinLdC, 1, cx.rows, pWp, H, h0, H, first);
        din_dw(Hs + L * ld, ld, A0, Qs, kDinLdC, 1, cx.ct, pWqd, H, h0, H, first);
        din_dw(Hs, ld, A0, Ks, kDinLdC, 1, L, pWkd, H, h0, H, first);
        __syncthreads();      // Us is free
        {
          const int col = h0 + i;
          const bool ok = col < H;
          const din_f32x4 du = din_dx_tile(Ds, ld, A0, 16 * wave, W0 + 3 * H, nullptr, 0.f, ldw, col, ok);
#pragma unroll
          for (int r = 0; r < 4; ++r) Us[(16 * wave + 4 * g + r) * kDinLdC + i] = du[r];
          if (16 * wave < L) {
            const din_f32x4 dk = din_dx_tile(Hs, ld, A0, 16 * wave, W0 + H, W0 + 2 * H, -1.f, ldw, col, ok);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = 16 * wave + 4 * g + r;
              if (row < L) Fs[row * kDinLdC + i] = dk[r];
            }
          }
          if (16 * wave < cx.ct) {
            const din_f32x4 dqf = din_dx_tile(Hs + L * ld, ld, A0, 16 * wave, W0, W0 + 2 * H, 1.f, ldw, col, ok);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = 16 * wave + 4 * g + r;
              if (row < cx.ct) Fs[(L + row) * kDinLdC + i] = dqf[r];
            }
          }
        }
        __syncthreads();
        // dq: complete within the tile
        for (int idx = t; idx < cx.ct * kDinKC; idx += kBlock) {
          const int c = idx >> 4, kc = idx & 15;
          if (h0 + kc < H) {
            float s = Fs[(L + c) * kDinLdC + kc];
            for (int l = 0; l < L; ++l) s += Us[(c * L + l) * kDinLdC + kc] * Ks[l * kDinLdC + kc];
            a.dq[(cx.n0 + c) * H + h0 + kc] = s;
          }
        }
        // dkeys[b]: this workgroup owns the row; tiles add in order
        for (int idx = t; idx < L * kDinKC; idx += kBlock) {
          const int l = idx >> 4, kc = idx & 15;
          if (h0 + kc < H) {
            float s = Fs[l * kDinLdC + kc];
            for (int c = 0; c < cx.ct; ++c)
              s += Us[(c * L + l) * kDinLdC + kc] * Qs[c * kDinLdC + kc] + wts[c * L + l] * Gs[c * kDinLdC + kc];
            float* p = a.dkeys + ((int64_t)cx.b * L + l) * H + h0 + kc;
            *p = (first_of_row ? 0.f : *p) + s;
          }
        }
        __syncthreads();
      }
      first = false;
    }
  }
}

// the G slices summed in workgroup order; the first layer unfolded into [Wq | Wk | Wd | Wp]
__global__ __launch_bounds__(kBlock) void din_reduce_kernel(DinArgs a, int G, float* dparams) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n1 = (int64_t)a.A[0] * a.H;
  if (e >= a.P - 2 * n1) return;
  if (e < n1) {
    float sq = 0.f, sk = 0.f, sp = 0.f;
    for (int gi = 0; gi < G; ++gi) {
      const float* p = a.partial + (int64_t)gi * a.P + a.poff_w[0] + e;
      sq += p[0];
      sk += p[n1];
      sp += p[2 * n1];
    }
    const int64_t row = e / a.H, h = e - row * a.H;
    float* o = dparams + row * 4 * a.H + h;
    o[0] = sq;
    o[a.H] = sk;
    o[2 * a.H] = sq - sk;
    o[3 * a.H] = sp;
  } else {
    // everything behind the first layer's weights has the same offset in a slice (+ 3 n1) as in dparams (+ 4 n1)
    const int64_t r = e - n1;
    float s = 0.f;
    for (int gi = 0; gi < G; ++gi) s += a.partial[(int64_t)gi * a.P + 3 * n1 + r];
    dparams[4 * n1 + r] = s;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static int din_shape_check(const char* who, int H, int L, int n_layers, const int* widths, float drop_p) {
  RC_REQUIRE(H >= 4 && H <= 512 && H % 4 == 0, "%s: H=%d must be a multiple of 4 in [4, 512] (fields x emb_size)", who, H);
  RC_REQUIRE(L >= 1 && L <= 64, "%s: history_max L=%d outside [1, 64]", who, L);
  RC_REQUIRE(n_layers >= 1 && n_layers <= kDinMaxLayers, "%s: att_layers has %d hidden layers, need 1 to 3", who, n_layers);
  RC_REQUIRE(widths != nullptr, "%s: null pointer (widths)", who);
  int sum = 0;
  for (int j = 0; j < n_layers; ++j) {
    RC_REQUIRE(widths[j] >= 16 && widths[j] <= 256 && widths[j] % 16 == 0,
               "%s: att_layers width %d must be a multiple of 16 in [16, 256]", who, widths[j]);
    sum += widths[j];
  }
  RC_REQUIRE(sum <= kDinMaxSum, "%s: att_layers widths sum to %d, at most %d fit in LDS", who, sum, kDinMaxSum);
  RC_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: dropout %g outside [0, 1)", who, (double)drop_p);
  return RC_OK;
}

static int64_t din_param_count(int H, int n_layers, const int* widths) {
  int64_t n = 0;
  int K = 4 * H;
  for (int j = 0; j < n_layers; ++j) {
    n += (int64_t)widths[j] * K + widths[j];
    K = widths[j];
  }
  return n + K + 1;
}

static size_t din_lds_bytes(int SA, bool bwd) {
  const size_t ld = SA + 4;
  size_t f = 2 * kDinBufRows * ld + kDinRows * kDinLdC + kDinRows;
  if (bwd) f += 3 * kDinRows * kDinLdC + (kDinBufRows + 1) * kDinLdC + kDinRows;
  return f * sizeof(float);
}

// workgroups of the backward: one slice of P floats each, at most 128 MiB of slices, at least 16 workgroups
static int din_bwd_groups(int64_t B, int64_t P) {
  int64_t cap = ((int64_t)128 << 20) / (P * 4);
  cap = cap < 16 ? 16 : (cap > 512 ? 512 : cap);
  return (int)(B < cap ? (B < 1 ? 1 : B) : cap);
}

static size_t din_bwd_ws_bytes(int64_t B, int H, int n_layers, const int* widths) {
  const int64_t P = din_param_count(H, n_layers, widths) - (int64_t)widths[0] * H;
  return align_up((size_t)din_bwd_groups(B, P) * P * sizeof(float), 256);
}

static int din_lds_attr(const char* who, const void* kern, int which, size_t lds) {
  static std::mutex mu;
  static size_t have[64][2];
  int dev = 0;
  RC_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if (dev < 0 || dev >= 64) {      // outside the cache: set it every time
    RC_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return RC_OK;
  }
  if (have[dev][which] < lds) {
    RC_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    have[dev][which] = lds;
  }
  return RC_OK;
}

static int din_fill_args(const char* who, DinArgs* a, const float* q, const float* keys, const int64_t* lengths, const float* params,
                         int64_t B, int C, int L, int H, int n_layers, const int* widths, float drop_p, const uint64_t* seed_dev,
                         uint32_t site0) {
  RC_TRY(din_shape_check(who, H, L, n_layers, widths, drop_p));
  RC_REQUIRE(q && keys && lengths && params, "%s: null pointer", who);
  RC_REQUIRE(B >= 1 && C >= 1 && B * (int64_t)C * L < ((int64_t)1 << 40) && B <= kMaxGridX, "%s: bad shape B=%lld C=%d", who, (long long)B, C);
  RC_REQUIRE(aligned16(q, keys, params), "%s: q, keys and params must be 16-byte aligned", who);
  RC_REQUIRE(drop_p == 0.f || seed_dev != nullptr, "%s: dropout p=%g needs a device seed", who, (double)drop_p);
  RC_REQUIRE(site0 + (uint32_t)n_layers <= 65536u, "%s: dropout site %u outside [0, 65536)", who, site0);
  memset(a, 0, sizeof(*a));
  a->q = q; a->keys = keys; a->lengths = lengths;
  a->B = (int)B; a->C = C; a->L = L; a->H = H; a->n_layers = n_layers;
  a->CT = kDinRows / L;
  a->tiles_per_row = (C + a->CT - 1) / a->CT;
  a->inv_sqrt_h = (float)(1.0 / sqrt((double)H));
  const float* p = params;
  int64_t po = 3 * (int64_t)widths[0] * H;      // a slice holds [dWqd | dWkd | dWp] where params hold [Wq | Wk | Wd | Wp], then the same order
  int K = 4 * H, off = 0;
  for (int j = 0; j < n_layers; ++j) {
    a->A[j] = widths[j];
    a->off[j] = off;
    off += widths[j];
    a->W[j] = p;
    p += (int64_t)widths[j] * K;
    a->bias[j] = p;
    p += widths[j];
    if (j == 0) {
      a->poff_w[0] = 0;
    } else {
      a->poff_w[j] = po;
      po += (int64_t)widths[j] * K;
    }
    a->poff_b[j] = po;
    po += widths[j];
    K = widths[j];
  }
  a->w_out = p;
  a->b_out = p + K;
  a->poff_wout = po;
  a->poff_bout = po + K;
  a->P = po + K + 1;
  a->SA = off;
  a->ld = off + 4;
  if (drop_p > 0.f) {      // (as rc_linear_fwd)
    a->seed = seed_dev;
    a->drop_thresh = (uint32_t)((double)drop_p * 4294967296.0);
    a->keep_scale = 1.0f / (1.0f - drop_p);
  }
  a->site0 = site0;
  return RC_OK;
}

static int din_fwd_impl(const float* q, const float* keys, const int64_t* lengths, const float* params, int64_t B, int C, int L, int H,
                        int n_layers, const int* widths, float drop_p, const uint64_t* seed_dev, uint32_t site0, float* out,
                        int64_t ld_out, float* att, rc_stream_t stream) {
  static const char* who = "rc_din_attention_fwd";
  if (B == 0) return RC_OK;
  DinArgs a;
  RC_TRY(din_fill_args(who, &a, q, keys, lengths, params, B, C, L, H, n_layers, widths, drop_p, seed_dev, site0));
  RC_REQUIRE(out != nullptr, "%s: null pointer", who);
  RC_REQUIRE(ld_out >= H && ld_out % 4 == 0 && aligned16(out), "%s: out must be 16-byte aligned with a row stride ld_out=%lld >= H, a multiple of 4",
             who, (long long)ld_out);
  a.out = out; a.ld_out = ld_out; a.att = att;
  const int64_t blocks = B * a.tiles_per_row;
  if (blocks > kMaxGridX) return fail(RC_ERR_UNSUPPORTED, "%s: grid too large (B=%lld C=%d)", who, (long long)B, C);
  const size_t lds = din_lds_bytes(a.SA, false);
  RC_REQUIRE(lds <= kDinLdsBudget, "%s: %zu bytes of LDS needed", who, lds);
  RC_TRY(din_lds_attr(who, reinterpret_cast<const void*>(din_fwd_kernel), 0, lds));
  hipLaunchKernelGGL(din_fwd_kernel, dim3((unsigned)blocks), dim3(kBlock), lds, as_stream(stream), a);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

static int din_bwd_impl(const float* q, const float* keys, const int64_t* lengths, const float* params, const float* d_out, int64_t B,
                        int C, int L, int H, int n_layers, const int* widths, float drop_p, const uint64_t* seed_dev, uint32_t site0,
                        float* dq, float* dkeys, float* dparams, void* ws, size_t ws_bytes, rc_stream_t stream) {
  static const char* who = "rc_din_attention_bwd";
  if (B == 0) return RC_OK;
  DinArgs a;
  RC_TRY(din_fill_args(who, &a, q, keys, lengths, params, B, C, L, H, n_layers, widths, drop_p, seed_dev, site0));
  RC_REQUIRE(d_out && dq && dkeys && dparams && ws, "%s: null pointer", who);
  RC_REQUIRE(aligned16(d_out, dq, dkeys, dparams, ws), "%s: d_out, dq, dkeys, dparams and the workspace must be 16-byte aligned", who);
  const size_t need = din_bwd_ws_bytes(B, H, n_layers, widths);
  if (ws_bytes < need) return fail(RC_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, need);
  a.d_out = d_out; a.dq = dq; a.dkeys = dkeys; a.partial = reinterpret_cast<float*>(ws);
  const int G = din_bwd_groups(B, a.P);
  const size_t lds = din_lds_bytes(a.SA, true);
  RC_REQUIRE(lds <= kDinLdsBudget, "%s: %zu bytes of LDS needed", who, lds);
  RC_TRY(din_lds_attr(who, reinterpret_cast<const void*>(din_bwd_kernel), 1, lds));
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(din_bwd_kernel, dim3(G), dim3(kBlock), lds, s, a, G);
  RC_LAUNCH_CHECK();
  const int64_t outs = a.P - 2 * (int64_t)a.A[0] * H;
  hipLaunchKernelGGL(din_reduce_kernel, dim3((unsigned)((outs + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a, G, dparams);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

}  // namespace rc

using namespace rc;

extern "C" enum rc_status rc_din_check_shape(int H, int L, int n_layers, const int* widths, float drop_p) {
  return (enum rc_status)din_shape_check("rc_din_check_shape", H, L, n_layers, widths, drop_p);
}

extern "C" size_t rc_din_param_count(int H, int n_layers, const int* widths) {
  if (din_shape_check("rc_din_param_count", H, 1, n_layers, widths, 0.f) != RC_OK) return 0;
  return (size_t)din_param_count(H, n_layers, widths);
}

extern "C" size_t rc_din_attention_bwd_workspace_bytes(int64_t B, int H, int n_layers, const int* widths) {
  if (din_shape_check("rc_din_attention_bwd_workspace_bytes", H, 1, n_layers, widths, 0.f) != RC_OK) return 0;
  return din_bwd_ws_bytes(B, H, n_layers, widths);
}

extern "C" enum rc_status rc_din_attention_fwd(const float* q, const float* keys, const int64_t* lengths, const float* params, int64_t B,
                                               int C, int L, int H, int n_layers, const int* widths, float drop_p,
                                               const uint64_t* seed_dev, uint32_t site0, float* out, int64_t ld_out, float* att,
                                               rc_stream_t stream) {
  return (enum rc_status)din_fwd_impl(q, keys, lengths, params, B, C, L, H, n_layers, widths, drop_p, seed_dev, site0, out, ld_out, att,
                                      stream);
}

extern "C" enum rc_status rc_din_attention_bwd(const float* q, const float* keys, const int64_t* lengths, const float* params,
                                               const float* d_out, int64_t B, int C, int L, int H, int n_layers, const int* widths,
                                               float drop_p, const uint64_t* seed_dev, uint32_t site0, float* dq, float* dkeys,
                                               float* dparams, void* ws, size_t ws_bytes, rc_stream_t stream) {
  return (enum rc_status)din_bwd_impl(q, keys, lengths, params, d_out, B, C, L, H, n_layers, widths, drop_p, seed_dev, site0, dq, dkeys,
                                      dparams, ws, ws_bytes, stream);
}
