// finalmlp.hip -- FinalMLP's two pieces of arithmetic beside the MLP streams (reference: models/context/FinalMLP.py)
//
// (a) feature selection + the first layer of both streams (FeatureSelection.forward :188-221, MLP_Block's first Linear + ReLU + Dropout)
//       X [N, D], D = F d, N = batch * candidates;  per stream s: Zin_s [Ng_s, G_s] (the input of the gate's last Linear),
//       Wg_s [D, G_s], bg_s [D], W_s [H_s, D], b_s [H_s];  instance n uses gate row 0 (Ng = 1), n / C (Ng = B) or n (Ng = N)
//       g_s = 2 sigmoid(Zin_s Wg_s^T + bg_s),  A_s = drop(relu((X * g_s) W_s^T + b_s)) [N, H_s]
// (b) its backward from X, the saved A_s (its own ReLU / dropout mask) and dA_s; the gate is recomputed:
//       dA' = dA * (A > 0) / (1 - p),  P_s = dA'_s W_s,  dX = sum_s P_s * g_s,  dz_s = P_s * X * g_s (1 - g_s / 2),
//       dZin_s = dz_s Wg_s (summed over the instances of one gate row),  dWg_s = dz_s^T Zin_s,  dbg_s = colsum dz_s,
//       dW_s = dA'_s^T (X * g_s),  db_s = colsum dA'_s
// (c) the bilinear fusion (InteractionAggregation.forward :238-249) and its backward:
//       out = w_x x + b_x + w_y y + b_y + sum_h x_h^T W_h y_h,  x [N, H1], y [N, H2], w_xy viewed [h, H1 / h, H2 / h]
//
// Two MFMA shapes serve every product, both on v_mfma_f32_32x32x2_f32 with the lane maps of autoint.hip / buir.hip (A operand: index
// i on the lane, B operand: index j on the lane, accumulator register r: i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), j = lane & 31):
//   fm_ksplit   one [TR][32] result tile whose reduction axis is cut over the four waves; the four partial tiles go to LDS and are
//               added in wave order by the step that consumes them (gate logits, P, the bilinear products)
//   output cut  32 x 32 output tiles dealt to the waves, accumulators in registers over the loop that feeds them (A_s over the column
//               chunks of D; the weight gradients over the workgroup's row tiles)
// Launches:
//   gate fwd    ONE launch for both streams.  A workgroup owns TR = 64 / 32 rows: both Zin tiles stay in LDS, D is walked in chunks
//               of 32 columns; per chunk the X chunk is read once, per stream the Wg / W chunks are staged, the gate chunk is formed
//               (fm_ksplit over G), multiplied into the X chunk in LDS and accumulated into the [TR][H_s] registers.  Neither the
//               gate nor the gated features leave the chip.
//   gate bwd    grid (row blocks, column slabs of 32): a workgroup keeps dW_s[:, slab], dWg_s[slab, :] in registers over its row
//               tiles.  Per tile and stream: gate chunk and P chunk (fm_ksplit over G and over H), dX chunk (both streams summed in
//               LDS, written once), dz and X * g chunks in LDS, then the three output-cut products.  With Ng > 1 the slab's share of
//               dZin, dz[:, slab] Wg[slab, :], goes to a plane [slab][N][G] of the workspace (a sum over D cannot stay on chip when
//               the columns are cut over workgroups).  Then: one reduce launch (partials in row-block order, in double) and one
//               launch that finishes dZin (Ng = 1: dbg Wg, as colsum(dz) = dbg; else the planes over slabs and gate-row members in
//               ascending order).
//   fusion fwd  ONE launch: x, y tiles in LDS; per 32-column tile of y the block-diagonal slice of w_xy (zeros off the heads) is
//               staged, T = x W (fm_ksplit over the rows of the heads that meet the tile), sum_j (T + w_y) y and w_x x per lane,
//               rows finished with a 32-lane shuffle sum.
//   fusion bwd  ONE launch + the reduce: dy = dout (w_y + x W), dx = dout (w_x + W y) by the same tile product, dw_xy += (dout x)^T y
//               for the 32 x 32 tiles that meet a head's block, in registers over the row tiles; x and y are read once.
// No float atomics: every sum has a fixed order, reruns are bitwise identical.
#include "common.hpp"
#include "philox.hpp"

namespace rc {

typedef float fm_f32x16 __attribute__((ext_vector_type(16)));

constexpr size_t kFmLdsBudget = 160 * 1024;
constexpr int kFmFwdBlocks = 1024;     // workgroups of the forward tile kernels
constexpr int kFmBwdWgs = 256;         // gate bwd: slabs x row blocks stays within one workgroup per CU, so that the slabs of a row
                                       // block run at the same time and its re-read tiles come from the caches
constexpr int kFuBlocks = 256;         // fusion: workgroups = partials per element
constexpr int kFmCS = 36;              // LDS stride of a 32-column chunk

struct FmStream {
  const float *Zin, *Wg, *bg, *W, *b;
  const float *A, *dA;                 // backward
  float* Aout;                         // forward
  const uint64_t* seed;
  uint32_t thresh, site;
  float keep;
  int G, H, GP, HP, GS, HS, mode;      // mode 0: gate row 0, 1: n / C, 2: n
  float *dW_part, *dWg_part, *dbg_part, *db_part, *plane;
};

struct FmArgs {
  const float* X;
  float* dX;
  int64_t N;
  int D, C, TR, maxGS, maxHP;      // (forward: the staging buffers both streams share)
  FmStream s[2];
};

__device__ __forceinline__ int fm_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// part[wave][row][32] = sum over this wave's quarter of k in [0, KP) of A[row][k] * (BK ? B[col][k] : B[k][col]);  KP % 32 == 0,
// A [TR][SA] and a k-major B float4-aligned.  Ends with the stores issued, not yet synced.
template <bool BK>
__device__ __forceinline__ void fm_ksplit(const float* A, int SA, const float* B, int SB, int KP, int nrb, int TR, float* part, int tid) {
  const int wave = tid >> 6, lane = tid & 63, h = lane >> 5, li = lane & 31;
  const int KH = KP / 8, k0 = wave * (KP / 4) + h * KH;
  fm_f32x16 acc[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[rb][r] = 0.f;
  for (int t = 0; t < KH; t += 4) {
    float4 b;
    if constexpr (BK) {
      b = *reinterpret_cast<const float4*>(B + li * SB + k0 + t);
    } else {
      const float* bp = B + (k0 + t) * SB + li;
      b = make_float4(bp[0], bp[SB], bp[2 * SB], bp[3 * SB]);
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
      if (rb < nrb) {   // (workgroup-uniform)
        const float4 a = *reinterpret_cast<const float4*>(A + (32 * rb + li) * SA + k0 + t);
        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[rb], 0, 0, 0);
        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[rb], 0, 0, 0);
        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[rb], 0, 0, 0);
        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[rb], 0, 0, 0);
      }
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
    if (rb < nrb)
#pragma unroll
      for (int r = 0; r < 16; ++r) part[(wave * TR + 32 * rb + fm_row(r, h)) * 32 + li] = acc[rb][r];
}

__device__ __forceinline__ float fm_part_sum(const float* part, int TR, int e) {
  return ((part[e] + part[TR * 32 + e]) + part[2 * TR * 32 + e]) + part[3 * TR * 32 + e];
}

__device__ __forceinline__ int64_t fm_zrow(int mode, int C, int64_t n) { return mode == 0 ? 0 : (mode == 1 ? n / C : n); }

__device__ __forceinline__ void fm_load_z(const FmStream& st, int C, float* zs, int64_t n0, int valid, int TR, int tid) {
  const int Q = st.GP / 4;
  for (int idx = tid; idx < TR * Q; idx += 256) {
    const int row = idx / Q, g = 4 * (idx - row * Q);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < valid && g < st.G) v = *reinterpret_cast<const float4*>(st.Zin + fm_zrow(st.mode, C, n0 + row) * st.G + g);
    *reinterpret_cast<float4*>(zs + row * st.GS + g) = v;
  }
}

// wgs[c][g] = Wg[c0 + c][g] (32 rows, GP columns, zeros outside), ws[o][k] = W[o][c0 + k] (HP rows, 32 columns, zeros outside)
__device__ __forceinline__ void fm_stage_w(const FmStream& st, int D, int c0, float* wgs, float* ws, int tid) {
  const int Q = st.GP / 4;
  for (int idx = tid; idx < 32 * Q; idx += 256) {
    const int c = idx / Q, g = 4 * (idx - c * Q);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 + c < D && g < st.G) v = *reinterpret_cast<const float4*>(st.Wg + (int64_t)(c0 + c) * st.G + g);
    *reinterpret_cast<float4*>(wgs + c * st.GS + g) = v;
  }
  for (int idx = tid; idx < st.HP * 8; idx += 256) {
    const int o = idx >> 3, k = 4 * (idx & 7);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o < st.H && c0 + k < D) v = *reinterpret_cast<const float4*>(st.W + (int64_t)o * D + c0 + k);
    *reinterpret_cast<float4*>(ws + o * kFmCS + k) = v;
  }
}

__device__ __forceinline__ void fm_load_x(const float* X, int D, int c0, float* xs, int64_t n0, int valid, int TR, int tid) {
  for (int idx = tid; idx < TR * 8; idx += 256) {
    const int row = idx >> 3, k = 4 * (idx & 7);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < valid && c0 + k < D) v = load_stream4(reinterpret_cast<const float4*>(X + (n0 + row) * D + c0 + k));
    *reinterpret_cast<float4*>(xs + row * kFmCS + k) = v;
  }
}

__device__ __forceinline__ float fm_gate(float logit) { return 2.0f / (1.0f + expf(-logit)); }

// ---- (a) forward ---------------------------------------------------------------------------------------------------------------------
template <bool DROP>      // (the Philox chains of the dropout epilogue cost registers: the p = 0 instance has none)
__global__ __launch_bounds__(256) void finalmlp_gate_fwd_kernel(FmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fm_lds[];
  const int TR = a.TR, nrb = TR / 32, D = a.D;
  float* zs[2];
  zs[0] = fm_lds;                                   // [TR][GS0]
  zs[1] = zs[0] + TR * a.s[0].GS;                   // [TR][GS1]
  float* wgs = zs[1] + TR * a.s[1].GS;              // [32][maxGS]
  float* ws = wgs + 32 * a.maxGS;                   // [maxHP][36]
  float* xs = ws + a.maxHP * kFmCS;                 // [TR][36]
  float* gxs = xs + TR * kFmCS;                     // [TR][36]
  float* part = gxs + TR * kFmCS;                   // [4][TR][32]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, li = lane & 31;
  const int64_t ntiles = (a.N + TR - 1) / TR;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t n0 = tile * TR;
    const int valid = (int)(a.N - n0 < TR ? a.N - n0 : TR);
    __syncthreads();   // every wave is done with the previous tile's LDS
#pragma unroll
    for (int s = 0; s < 2; ++s) fm_load_z(a.s[s], a.C, zs[s], n0, valid, TR, tid);
    fm_f32x16 acc[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][q][r] = 0.f;
    for (int c0 = 0; c0 < D; c0 += 32) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const FmStream& st = a.s[s];
        __syncthreads();   // the products of the stream before are done with wgs / ws / gxs (and, s == 0, with xs)
        if (s == 0) fm_load_x(a.X, D, c0, xs, n0, valid, TR, tid);
        fm_stage_w(st, D, c0, wgs, ws, tid);
        __syncthreads();
        fm_ksplit<true>(zs[s], st.GS, wgs, st.GS, st.GP, nrb, TR, part, tid);
        __syncthreads();
        for (int e = tid; e < TR * 32; e += 256) {
          const int row = e >> 5, col = e & 31, c = c0 + col;
          const float g = c < D ? fm_gate(fm_part_sum(part, TR, e) + st.bg[c]) : 0.f;
          gxs[row * kFmCS + col] = xs[row * kFmCS + col] * g;
        }
        __syncthreads();
        const int not_ = st.HP / 32;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int p = wave + 4 * q;
          if (p < nrb * not_) {   // (wave-uniform)
            const int rb = p % nrb, ot = p / nrb;
            const float* ap = gxs + (32 * rb + li) * kFmCS + 16 * h;
            const float* bp = ws + (32 * ot + li) * kFmCS + 16 * h;
#pragma unroll
            for (int t = 0; t < 16; t += 4) {
              const float4 x = *reinterpret_cast<const float4*>(ap + t);
              const float4 w = *reinterpret_cast<const float4*>(bp + t);
              acc[s][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, w.x, acc[s][q], 0, 0, 0);
              acc[s][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, w.y, acc[s][q], 0, 0, 0);
              acc[s][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, w.z, acc[s][q], 0, 0, 0);
              acc[s][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, w.w, acc[s][q], 0, 0, 0);
            }
          }
        }
      }
    }
    // bias, ReLU, dropout (the mask stream of rc_linear_fwd: word (n & 3) of Philox(seed, n >> 2, site * 65536 + o)), one store
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const FmStream& st = a.s[s];
      const int not_ = st.HP / 32;
      const uint64_t seed = st.seed ? *st.seed : 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = wave + 4 * q;
        if (p < nrb * not_) {
          const int rb = p % nrb, o = 32 * (p / nrb) + li;
          const float bias = o < st.H ? st.b[o] : 0.f;
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int64_t nb = n0 + 32 * rb + 8 * r4 + 4 * h;
            uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            if (DROP && st.seed && nb < a.N && o < st.H) philox4x32_10(seed, (uint64_t)(nb >> 2), st.site * 65536u + (uint32_t)o, w);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float v = fmaxf(acc[s][q][4 * r4 + e] + bias, 0.f);
              if (DROP && st.seed) v *= (w[e] < st.thresh ? 0.f : st.keep);
              if (nb + e < a.N && o < st.H) st.Aout[(nb + e) * st.H + o] = v;
            }
          }
        }
      }
    }
  }
}

// ---- (b) backward --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void finalmlp_gate_bwd_kernel(FmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fm_lds[];
  const int TR = a.TR, nrb = TR / 32, D = a.D;
  float* xs = fm_lds;                               // [TR][36]
  float* gts = xs + TR * kFmCS;                     // gate chunk
  float* gxs = gts + TR * kFmCS;                    // X * g
  float* dzs = gxs + TR * kFmCS;                    // dz
  float* dxs = dzs + TR * kFmCS;                    // dX, both streams
  float* part = dxs + TR * kFmCS;                   // [4][TR][32]
  float* sbase = part + 4 * TR * 32;                // the stream in hand: zs [TR][GS], das [TR][HS] (dA'), wgs [32][GS], ws [HP][36]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, li = lane & 31;
  // the slab is the fast grid index: the workgroups that share a row block (and re-read its Zin, A, dA) are dispatched together
  const int slab = blockIdx.x, rblk = blockIdx.y, nrblk = gridDim.y;
  const int c0 = 32 * slab;

  fm_f32x16 dwacc[2][2], dgacc[2][2];    // dW_s[32 (wave + 4 q) ..][slab], dWg_s[slab][32 (wave + 4 q) ..]
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) dwacc[s][q][r] = 0.f, dgacc[s][q][r] = 0.f;
  float dbg_acc[2] = {0.f, 0.f}, db_acc[2] = {0.f, 0.f};

  const int64_t ntiles = (a.N + TR - 1) / TR;
  for (int64_t tile = rblk; tile < ntiles; tile += nrblk) {
    const int64_t n0 = tile * TR;
    const int valid = (int)(a.N - n0 < TR ? a.N - n0 : TR);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const FmStream& st = a.s[s];
      float* zs = sbase;
      float* das = zs + TR * st.GS;
      float* wgs = das + TR * st.HS;
      float* ws = wgs + 32 * st.GS;
      __syncthreads();   // every wave is done with the stream before (and the tile before)
      if (s == 0) fm_load_x(a.X, D, c0, xs, n0, valid, TR, tid);
      fm_load_z(st, a.C, zs, n0, valid, TR, tid);
      fm_stage_w(st, D, c0, wgs, ws, tid);
      {   // dA' = dA * (A > 0) / (1 - p); zeros in the padding and past the batch
        const int Q = st.HP / 4;
        for (int idx = tid; idx < TR * Q; idx += 256) {
          const int row = idx / Q, o = 4 * (idx - row * Q);
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (row < valid && o < st.H) {
            const float4 y = *reinterpret_cast<const float4*>(st.A + (n0 + row) * st.H + o);
            const float4 dy = load_stream4(reinterpret_cast<const float4*>(st.dA + (n0 + row) * st.H + o));
            v = make_float4(y.x > 0.f ? dy.x * st.keep : 0.f, y.y > 0.f ? dy.y * st.keep : 0.f, y.z > 0.f ? dy.z * st.keep : 0.f,
                            y.w > 0.f ? dy.w * st.keep : 0.f);
          }
          *reinterpret_cast<float4*>(das + row * st.HS + o) = v;
        }
      }
      __syncthreads();
      fm_ksplit<true>(zs, st.GS, wgs, st.GS, st.GP, nrb, TR, part, tid);
      __syncthreads();
      for (int e = tid; e < TR * 32; e += 256) {
        const int row = e >> 5, col = e & 31, c = c0 + col;
        gts[row * kFmCS + col] = c < D ? fm_gate(fm_part_sum(part, TR, e) + st.bg[c]) : 0.f;
      }
      __syncthreads();
      fm_ksplit<false>(das, st.HS, ws, kFmCS, st.HP, nrb, TR, part, tid);      // P = dA' W[:, slab]
      __syncthreads();
      for (int e = tid; e < TR * 32; e += 256) {
        const int row = e >> 5, col = e & 31, at = row * kFmCS + col;
        const float P = fm_part_sum(part, TR, e), g = gts[at], x = xs[at];
        const float pg = P * g;
        dxs[at] = s == 0 ? pg : dxs[at] + pg;
        gxs[at] = x * g;
        dzs[at] = (P * x) * (g * (1.0f - 0.5f * g));
      }
      __syncthreads();
      // dW_s[o][c] += sum_row dA'[row][o] (X g)[row][c]: step t contracts row 2 t + h; A = dA'[row][32 ot + li], B = (X g)[row][li]
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int ot = wave + 4 * q;
        if (ot < st.HP / 32) {
#pragma unroll 4
          for (int t = 0; t < TR / 2; ++t) {
            const int row = 2 * t + h;
            dwacc[s][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(das[row * st.HS + 32 * ot + li], gxs[row * kFmCS + li], dwacc[s][q], 0, 0, 0);
          }
        }
      }
      // dWg_s[c][g] += sum_row dz[row][c] Zin[row][g]
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int gt = wave + 4 * q;
        if (gt < st.GP / 32) {
#pragma unroll 4
          for (int t = 0; t < TR / 2; ++t) {
            const int row = 2 * t + h;
            dgacc[s][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(dzs[row * kFmCS + li], zs[row * st.GS + 32 * gt + li], dgacc[s][q], 0, 0, 0);
          }
        }
      }
      // the slab's share of dZin: plane[slab][n][g] = sum_c dz[n][c] Wg[c0 + c][g]
      if (st.mode != 0) {
        const int ngt = st.GP / 32;
        for (int p = wave; p < nrb * ngt; p += 4) {
          const int rb = p % nrb, gt = p / nrb;
          fm_f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
          const float* ap = dzs + (32 * rb + li) * kFmCS + 16 * h;
          const float* bp = wgs + (16 * h) * st.GS + 32 * gt + li;
#pragma unroll
          for (int t = 0; t < 16; t += 4) {
            const float4 x = *reinterpret_cast<const float4*>(ap + t);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, bp[(t + 0) * st.GS], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, bp[(t + 1) * st.GS], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, bp[(t + 2) * st.GS], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, bp[(t + 3) * st.GS], acc, 0, 0, 0);
          }
          const int g = 32 * gt + li;
          float* pl = st.plane + ((int64_t)slab * a.N + n0 + 32 * rb) * st.G + g;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = fm_row(r, h);
            if (32 * rb + row < valid && g < st.G) pl[(int64_t)row * st.G] = acc[r];
          }
        }
      }
      if (tid < 32)
        for (int row = 0; row < valid; ++row) dbg_acc[s] += dzs[row * kFmCS + tid];
      if (slab == 0 && tid < st.H)
        for (int row = 0; row < valid; ++row) db_acc[s] += das[row * st.HS + tid];
    }
    // dX chunk, both streams: written once
    for (int idx = tid; idx < TR * 8; idx += 256) {
      const int row = idx >> 3, k = 4 * (idx & 7);
      if (row < valid && c0 + k < D)
        *reinterpret_cast<float4*>(a.dX + (n0 + row) * D + c0 + k) = *reinterpret_cast<const float4*>(dxs + row * kFmCS + k);
    }
  }

#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const FmStream& st = a.s[s];
    float* dWp = st.dW_part + (int64_t)rblk * st.H * D;
    float* dGp = st.dWg_part + (int64_t)rblk * D * st.G;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int t32 = wave + 4 * q;
      if (t32 < st.HP / 32) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int o = 32 * t32 + fm_row(r, h), c = c0 + li;
          if (o < st.H && c < D) dWp[(int64_t)o * D + c] = dwacc[s][q][r];
        }
      }
      if (t32 < st.GP / 32) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = c0 + fm_row(r, h), g = 32 * t32 + li;
          if (c < D && g < st.G) dGp[(int64_t)c * st.G + g] = dgacc[s][q][r];
        }
      }
    }
    if (tid < 32 && c0 + tid < D) st.dbg_part[(int64_t)rblk * D + c0 + tid] = dbg_acc[s];
    if (slab == 0 && tid < st.H) st.db_part[(int64_t)rblk * st.H + tid] = db_acc[s];
  }
}

// the partials of up to 8 gradient arrays, [parts][n] each, added in part order in double: one thread per element
struct FmSeg {
  const float* src;
  float* dst;
  int64_t n;
};
struct FmReduceArgs {
  FmSeg seg[8];
  int nseg, parts;
};
__global__ __launch_bounds__(kBlock) void finalmlp_reduce_kernel(FmReduceArgs a) {
  int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  for (int i = 0; i < a.nseg; ++i) {
    const FmSeg& sg = a.seg[i];
    if (e < sg.n) {
      double acc = 0.0;
      for (int p = 0; p < a.parts; ++p) acc += (double)sg.src[(int64_t)p * sg.n + e];
      sg.dst[e] = (float)acc;
      return;
    }
    e -= sg.n;
  }
}

// dZin per stream.  Ng = 1: dZin[g] = sum_c dbg[c] Wg[c][g];  else dZin[r][g] = the planes over the members of gate row r and the slabs
struct FmDzinArgs {
  const float *dbg[2], *Wg[2], *plane[2];
  float* dZin[2];
  int G[2], mode[2];
  int64_t N;
  int D, C, nslab;
};
__global__ __launch_bounds__(kBlock) void finalmlp_dzin_kernel(FmDzinArgs a) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  for (int s = 0; s < 2; ++s) {
    const int G = a.G[s];
    if (a.mode[s] == 0) {
      if (e < G) {
        double acc = 0.0;
        for (int c = 0; c < a.D; ++c) acc += (double)a.dbg[s][c] * (double)a.Wg[s][(int64_t)c * G + e];
        a.dZin[s][e] = (float)acc;
      }
    } else {
      const int members = a.mode[s] == 1 ? a.C : 1;
      const int64_t rows = a.N / members;
      if (e < rows * G) {
        const int64_t r = e / G;
        const int g = (int)(e - r * G);
        float acc = 0.f;
        for (int m = 0; m < members; ++m)
          for (int sl = 0; sl < a.nslab; ++sl) acc += a.plane[s][((int64_t)sl * a.N + r * members + m) * G + g];
        a.dZin[s][e] = acc;
      }
    }
  }
}

// ---- (c) fusion ----------------------------------------------------------------------------------------------------------------------
struct FuArgs {
  const float *x, *y, *wxy, *wx, *wy, *bx, *by, *dout;
  float *out, *dx, *dy;
  float *dwxy_part, *dwx_part, *dwy_part, *db_part;
  int64_t N;
  int H1, H2, heads, hx, hy, H1P, H2P, SX, SY, SW, TR;
  int ntile;
  unsigned char tiles[64];    // the 32 x 32 tiles (it * 8 + jt) of [H1][H2] that meet a head's block
};

// Wbd[i][j]: w_xy as the block-diagonal [H1][H2] matrix
__device__ __forceinline__ float fu_w(const FuArgs& a, int i, int j) {
  if (i >= a.H1 || j >= a.H2) return 0.f;
  const int hd = i / a.hx;
  if (j / a.hy != hd) return 0.f;
  return a.wxy[(int64_t)hd * a.hx * a.hy + (i - hd * a.hx) * a.hy + (j - hd * a.hy)];
}

// the 32-aligned range of the other axis whose heads meet [t0, t0 + 32) of this axis (w: head width here, wo: head width there)
__device__ __forceinline__ void fu_range(int t0, int n, int w, int wo, int nP, int* kbeg, int* kend) {
  const int hi = (t0 + 31 < n ? t0 + 31 : n - 1) / w, lo = t0 / w;
  *kbeg = (lo * wo) / 32 * 32;
  const int e = ((hi + 1) * wo + 31) / 32 * 32;
  *kend = e < nP ? e : nP;
}

__device__ __forceinline__ void fu_load_xy(const FuArgs& a, float* xs, float* ys, int64_t n0, int valid, int tid) {
  const int Q1 = a.H1P / 4, Q2 = a.H2P / 4;
  for (int idx = tid; idx < a.TR * Q1; idx += 256) {
    const int row = idx / Q1, k = 4 * (idx - row * Q1);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < valid && k < a.H1) v = load_stream4(reinterpret_cast<const float4*>(a.x + (n0 + row) * a.H1 + k));
    *reinterpret_cast<float4*>(xs + row * a.SX + k) = v;
  }
  for (int idx = tid; idx < a.TR * Q2; idx += 256) {
    const int row = idx / Q2, k = 4 * (idx - row * Q2);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < valid && k < a.H2) v = load_stream4(reinterpret_cast<const float4*>(a.y + (n0 + row) * a.H2 + k));
    *reinterpret_cast<float4*>(ys + row * a.SY + k) = v;
  }
}

// wch[c][k] for the 32 columns j0 + c of y and k = i in [kbeg, kend) (TRANSPOSED: the 32 rows i0 + c of x and k = j)
template <bool TRANSPOSED>
__device__ __forceinline__ void fu_stage(const FuArgs& a, float* wch, int t0, int kbeg, int kend, int tid) {
  const int len = kend - kbeg;
  if constexpr (!TRANSPOSED) {
    for (int idx = tid; idx < 32 * len; idx += 256) {     // consecutive threads: consecutive j (contiguous in w_xy)
      const int c = idx & 31, k = kbeg + (idx >> 5);
      wch[c * a.SW + k] = fu_w(a, k, t0 + c);
    }
  } else {
    for (int idx = tid; idx < 32 * len; idx += 256) {
      const int c = idx / len, k = kbeg + (idx - c * len);
      wch[c * a.SW + k] = fu_w(a, t0 + c, k);
    }
  }
}

__global__ __launch_bounds__(256) void finalmlp_fusion_fwd_kernel(FuArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fm_lds[];
  const int TR = a.TR, nrb = TR / 32;
  float* xs = fm_lds;                     // [TR][SX]
  float* ys = xs + TR * a.SX;             // [TR][SY]
  float* wch = ys + TR * a.SY;            // [32][SW]
  float* part = wch + 32 * a.SW;          // [4][TR][32]
  const int tid = threadIdx.x;
  const float bias = a.bx[0] + a.by[0];
  const int64_t ntiles = (a.N + TR - 1) / TR;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t n0 = tile * TR;
    const int valid = (int)(a.N - n0 < TR ? a.N - n0 : TR);
    __syncthreads();
    fu_load_xy(a, xs, ys, n0, valid, tid);
    float racc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) racc[i] = 0.f;
    for (int j0 = 0; j0 < a.H2; j0 += 32) {
      int kbeg, kend;
      fu_range(j0, a.H2, a.hy, a.hx, a.H1P, &kbeg, &kend);
      __syncthreads();   // the product before is done with wch, its consumer with part; xs / ys are written (first time)
      fu_stage<false>(a, wch, j0, kbeg, kend, tid);
      __syncthreads();
      fm_ksplit<true>(xs + kbeg, a.SX, wch + kbeg, a.SW, kend - kbeg, nrb, TR, part, tid);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int e = tid + 256 * i;
        if (e < TR * 32) {
          const int row = e >> 5, j = j0 + (e & 31);
          if (j < a.H2) racc[i] = fmaf(fm_part_sum(part, TR, e) + a.wy[j], ys[row * a.SY + j], racc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i;
      if (e < TR * 32) {      // (uniform over a 32-lane half)
        const int row = e >> 5;
        float v = racc[i];
        for (int k = e & 31; k < a.H1; k += 32) v = fmaf(a.wx[k], xs[row * a.SX + k], v);
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((e & 31) == 0 && row < valid) a.out[n0 + row] = v + bias;
      }
    }
  }
}

template <int NSLOT>
__global__ __launch_bounds__(256) void finalmlp_fusion_bwd_kernel(FuArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fm_lds[];
  const int TR = a.TR, nrb = TR / 32;
  float* xs = fm_lds;
  float* ys = xs + TR * a.SX;
  float* wch = ys + TR * a.SY;
  float* part = wch + 32 * a.SW;
  float* ds = part + 4 * TR * 32;         // [TR] dout, zeros past the batch
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, li = lane & 31;
  fm_f32x16 dwacc[NSLOT];
#pragma unroll
  for (int q = 0; q < NSLOT; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) dwacc[q][r] = 0.f;
  float dwx_acc = 0.f, dwy_acc = 0.f, db_acc = 0.f;
  const int64_t ntiles = (a.N + TR - 1) / TR;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t n0 = tile * TR;
    const int valid = (int)(a.N - n0 < TR ? a.N - n0 : TR);
    __syncthreads();
    fu_load_xy(a, xs, ys, n0, valid, tid);
    if (tid < TR) ds[tid] = tid < valid ? a.dout[n0 + tid] : 0.f;
    // dy = dout (w_y + x W)
    for (int j0 = 0; j0 < a.H2; j0 += 32) {
      int kbeg, kend;
      fu_range(j0, a.H2, a.hy, a.hx, a.H1P, &kbeg, &kend);
      __syncthreads();
      fu_stage<false>(a, wch, j0, kbeg, kend, tid);
      __syncthreads();
      fm_ksplit<true>(xs + kbeg, a.SX, wch + kbeg, a.SW, kend - kbeg, nrb, TR, part, tid);
      __syncthreads();
      for (int e = tid; e < TR * 32; e += 256) {
        const int row = e >> 5, j = j0 + (e & 31);
        if (row < valid && j < a.H2) a.dy[(n0 + row) * a.H2 + j] = ds[row] * (fm_part_sum(part, TR, e) + a.wy[j]);
      }
    }
    // dx = dout (w_x + W y)
    for (int i0 = 0; i0 < a.H1; i0 += 32) {
      int kbeg, kend;
      fu_range(i0, a.H1, a.hx, a.hy, a.H2P, &kbeg, &kend);
      __syncthreads();
      fu_stage<true>(a, wch, i0, kbeg, kend, tid);
      __syncthreads();
      fm_ksplit<true>(ys + kbeg, a.SY, wch + kbeg, a.SW, kend - kbeg, nrb, TR, part, tid);
      __syncthreads();
      for (int e = tid; e < TR * 32; e += 256) {
        const int row = e >> 5, i = i0 + (e & 31);
        if (row < valid && i < a.H1) a.dx[(n0 + row) * a.H1 + i] = ds[row] * (fm_part_sum(part, TR, e) + a.wx[i]);
      }
    }
    // dWbd[i][j] += sum_row (dout x)[row][i] y[row][j] on the tiles that meet a head's block
#pragma unroll
    for (int q = 0; q < NSLOT; ++q) {
      const int idx = wave + 4 * q;
      if (idx < a.ntile) {    // (wave-uniform)
        const int it = a.tiles[idx] >> 3, jt = a.tiles[idx] & 7;
#pragma unroll 4
        for (int t = 0; t < TR / 2; ++t) {
          const int row = 2 * t + h;
          dwacc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[row * a.SX + 32 * it + li] * ds[row], ys[row * a.SY + 32 * jt + li], dwacc[q], 0, 0, 0);
        }
      }
    }
    if (tid < a.H1)
      for (int row = 0; row < valid; ++row) dwx_acc = fmaf(ds[row], xs[row * a.SX + tid], dwx_acc);
    if (tid < a.H2)
      for (int row = 0; row < valid; ++row) dwy_acc = fmaf(ds[row], ys[row * a.SY + tid], dwy_acc);
    if (tid == 0)
      for (int row = 0; row < valid; ++row) db_acc += ds[row];
  }
  const int nxy = a.heads * a.hx * a.hy;
  float* wp = a.dwxy_part + (int64_t)blockIdx.x * nxy;
#pragma unroll
  for (int q = 0; q < NSLOT; ++q) {
    const int idx = wave + 4 * q;
    if (idx < a.ntile) {
      const int it = a.tiles[idx] >> 3, jt = a.tiles[idx] & 7;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = 32 * it + fm_row(r, h), j = 32 * jt + li;
        if (i < a.H1 && j < a.H2) {
          const int hd = i / a.hx;
          if (j / a.hy == hd) wp[hd * a.hx * a.hy + (i - hd * a.hx) * a.hy + (j - hd * a.hy)] = dwacc[q][r];
        }
      }
    }
  }
  if (tid < a.H1) a.dwx_part[(int64_t)blockIdx.x * a.H1 + tid] = dwx_acc;
  if (tid < a.H2) a.dwy_part[(int64_t)blockIdx.x * a.H2 + tid] = dwy_acc;
  if (tid == 0) a.db_part[blockIdx.x] = db_acc;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static int fm_up32(int v) { return (v + 31) / 32 * 32; }

static bool fm_width_ok(int v) { return v >= 4 && v <= 256 && v % 4 == 0; }

// the one statement of the gate kernels' envelope
static int fm_gate_shape(const char* fn, int D, int G1, int H1, int G2, int H2, float p1, float p2) {
  if (D >= 12 && D <= 4096 && D % 4 == 0 && fm_width_ok(G1) && fm_width_ok(H1) && fm_width_ok(G2) && fm_width_ok(H2) && p1 >= 0.f &&
      p1 < 1.f && p2 >= 0.f && p2 < 1.f)
    return RC_OK;
  return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (flattened field width a multiple of 4 in [12, 4096], gate input and first-layer "
              "widths multiples of 4 in [4, 256], dropout in [0, 1)): width=%d gate=%d/%d first_layer=%d/%d dropout=%g/%g", fn, D, G1, G2,
              H1, H2, (double)p1, (double)p2);
}

static size_t fm_fwd_lds(int TR, int GP1, int GP2, int maxHP) {
  const int maxGS = (GP1 > GP2 ? GP1 : GP2) + 4;
  return sizeof(float) * ((size_t)TR * (GP1 + 4 + GP2 + 4) + 32 * (size_t)maxGS + (size_t)maxHP * kFmCS + 2 * (size_t)TR * kFmCS + 4 * (size_t)TR * 32);
}
static size_t fm_bwd_lds(int TR, int GP1, int HP1, int GP2, int HP2) {
  auto stream = [&](int GP, int HP) { return (size_t)TR * (GP + 4) + (size_t)TR * (HP + 4) + 32 * (size_t)(GP + 4) + (size_t)HP * kFmCS; };
  const size_t s1 = stream(GP1, HP1), s2 = stream(GP2, HP2);
  return sizeof(float) * (5 * (size_t)TR * kFmCS + 4 * (size_t)TR * 32 + (s1 > s2 ? s1 : s2));
}
// tile rows: 64 where the LDS holds them, else 32; 0: no tile fits
static int fm_tile(int G1, int H1, int G2, int H2, bool bwd) {
  const int GP1 = fm_up32(G1), GP2 = fm_up32(G2), HP1 = fm_up32(H1), HP2 = fm_up32(H2);
  const int maxHP = HP1 > HP2 ? HP1 : HP2;
  for (int TR : {64, 32})
    if ((bwd ? fm_bwd_lds(TR, GP1, HP1, GP2, HP2) : fm_fwd_lds(TR, GP1, GP2, maxHP)) <= kFmLdsBudget) return TR;
  return 0;
}

static int fm_gate_check(const char* fn, int64_t N, int C, int D, int G1, int H1, int G2, int H2, float p1, float p2, bool bwd, int* TR) {
  RC_TRY(fm_gate_shape(fn, D, G1, H1, G2, H2, p1, p2));
  if (N < 1 || N > ((int64_t)1 << 26) || C < 1 || N % C != 0)
    return fail(RC_ERR_UNSUPPORTED, "%s: instances in [1, 2^26], a whole number of candidate lists: instances=%lld candidates=%d", fn,
                (long long)N, C);
  *TR = fm_tile(G1, H1, G2, H2, bwd);
  if (*TR == 0)
    return fail(RC_ERR_UNSUPPORTED, "%s: no tile fits the LDS (the backward holds 32 rows of one stream's gate input and first-layer gradient beside "
                "the weight chunks: 256 gate + 272 first_layer <= 122880 per stream, both rounded up to 32): gate=%d/%d first_layer=%d/%d", fn, G1, G2, H1, H2);
  return RC_OK;
}

static int fu_shape(const char* fn, int H1, int H2, int heads) {
  if (fm_width_ok(H1) && fm_width_ok(H2) && heads >= 1 && H1 % heads == 0 && H2 % heads == 0) return RC_OK;
  return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (stream output widths multiples of 4 in [4, 256], num_heads a divisor of both): "
              "widths=%d/%d num_heads=%d", fn, H1, H2, heads);
}

static void fu_geometry(FuArgs* a, int H1, int H2, int heads) {
  a->H1 = H1, a->H2 = H2, a->heads = heads, a->hx = H1 / heads, a->hy = H2 / heads;
  a->H1P = fm_up32(H1), a->H2P = fm_up32(H2);
  a->SX = a->H1P + 4, a->SY = a->H2P + 4, a->SW = (a->H1P > a->H2P ? a->H1P : a->H2P) + 4;
  const size_t fixed = sizeof(float) * 32 * (size_t)a->SW;
  a->TR = 32;
  if (fixed + sizeof(float) * 64 * ((size_t)a->SX + a->SY + 128 + 1) <= kFmLdsBudget) a->TR = 64;
  a->ntile = 0;
  for (int it = 0; it < a->H1P / 32; ++it)
    for (int jt = 0; jt < a->H2P / 32; ++jt) {
      const int ilo = 32 * it / a->hx, ihi = (32 * it + 31 < H1 ? 32 * it + 31 : H1 - 1) / a->hx;
      const int jlo = 32 * jt / a->hy, jhi = (32 * jt + 31 < H2 ? 32 * jt + 31 : H2 - 1) / a->hy;
      if (ilo <= jhi && jlo <= ihi) a->tiles[a->ntile++] = (unsigned char)(it * 8 + jt);
    }
}
static size_t fu_lds(const FuArgs& a) { return sizeof(float) * ((size_t)a.TR * (a.SX + a.SY + 128 + 1) + 32 * (size_t)a.SW); }

static int fu_blocks(const FuArgs& a, int64_t N) {
  const int64_t tiles = (N + a.TR - 1) / a.TR;
  return (int)(tiles < kFuBlocks ? tiles : kFuBlocks);
}

static int fm_fill_stream(const char* fn, const rc_finalmlp_stream* in, int64_t N, int C, bool draws, FmStream* st) {
  RC_REQUIRE(in->Zin && in->Wg && in->bg && in->W && in->b, "%s: null pointer in a stream", fn);
  RC_REQUIRE(aligned16(in->Zin, in->Wg, in->W), "%s: Zin, Wg and W must be 16-byte aligned", fn);
  RC_REQUIRE(!draws || in->drop_p == 0.f || in->seed != nullptr, "%s: dropout p=%g needs a device seed", fn, (double)in->drop_p);
  RC_REQUIRE(in->site < 65536u, "%s: dropout site %u outside [0, 65536)", fn, in->site);
  memset(st, 0, sizeof(*st));
  st->Zin = in->Zin, st->Wg = in->Wg, st->bg = in->bg, st->W = in->W, st->b = in->b;
  st->G = in->G, st->H = in->H, st->GP = fm_up32(in->G), st->HP = fm_up32(in->H), st->GS = st->GP + 4, st->HS = st->HP + 4;
  if (in->n_gate_rows == N && (C > 1 || N > 1)) st->mode = 2;
  else if (in->n_gate_rows == N / C && N / C > 1) st->mode = 1;
  else if (in->n_gate_rows == 1) st->mode = 0;
  else
    return fail(RC_ERR_INVALID_ARG, "%s: a gate has 1, instances / candidates or instances rows: rows=%lld instances=%lld candidates=%d", fn,
                (long long)in->n_gate_rows, (long long)N, C);
  st->keep = 1.0f / (1.0f - in->drop_p);
  if (draws && in->drop_p > 0.f) {
    st->seed = in->seed;
    st->thresh = (uint32_t)((double)in->drop_p * 4294967296.0);
    st->site = in->site;
  }
  return RC_OK;
}

static void fm_bwd_grid(int64_t N, int D, int TR, int* bx, int* nslab) {
  *nslab = (D + 31) / 32;
  const int64_t tiles = (N + TR - 1) / TR;
  int cap = kFmBwdWgs / *nslab;
  if (cap < 1) cap = 1;
  *bx = (int)(tiles < cap ? tiles : cap);
}

struct FmBwdWs {
  float *dW[2], *dWg[2], *dbg[2], *db[2], *plane[2], *dbg_sum[2];
  size_t bytes;
};
static FmBwdWs fm_bwd_carve(void* ws, int64_t N, int D, const int G[2], const int H[2], const int mode[2], int bx, int nslab) {
  Carver c(ws);
  FmBwdWs w{};
  for (int s = 0; s < 2; ++s) {
    w.dW[s] = c.take<float>((size_t)bx * H[s] * D);
    w.dWg[s] = c.take<float>((size_t)bx * D * G[s]);
    w.dbg[s] = c.take<float>((size_t)bx * D);
    w.db[s] = c.take<float>((size_t)bx * H[s]);
    w.plane[s] = c.take<float>(mode[s] != 0 ? (size_t)nslab * N * G[s] : 0);
  }
  w.bytes = c.off;
  return w;
}

static int fm_mode_of(int64_t rows, int64_t N, int C) {
  if (rows == N && (C > 1 || N > 1)) return 2;
  if (rows == N / C && N / C > 1) return 1;
  return 0;
}

}  // namespace rc

extern "C" int rc_finalmlp_check_shape(int n_fields, int emb_size, int gate_in_1, int first_1, int gate_in_2, int first_2, int x_dim, int y_dim,
                                       int num_heads, float drop_p_1, float drop_p_2) {
  using namespace rc;
  const char* fn = "rc_finalmlp_check_shape";
  if (n_fields < 3 || n_fields > 32 || emb_size < 4 || emb_size > 128 || emb_size % 4 != 0)
    return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (fields in [3, 32], emb_size a multiple of 4 in [4, 128]): fields=%d emb_size=%d", fn,
                n_fields, emb_size);
  RC_TRY(fm_gate_shape(fn, n_fields * emb_size, gate_in_1, first_1, gate_in_2, first_2, drop_p_1, drop_p_2));
  RC_TRY(fu_shape(fn, x_dim, y_dim, num_heads));
  int TR;
  RC_TRY(fm_gate_check(fn, 1, 1, n_fields * emb_size, gate_in_1, first_1, gate_in_2, first_2, drop_p_1, drop_p_2, false, &TR));
  RC_TRY(fm_gate_check(fn, 1, 1, n_fields * emb_size, gate_in_1, first_1, gate_in_2, first_2, drop_p_1, drop_p_2, true, &TR));
  return RC_OK;
}

extern "C" size_t rc_finalmlp_gate_workspace_bytes(int64_t n_instances, int n_cand, int D, int gate_in_1, int first_1, int64_t gate_rows_1,
                                                   int gate_in_2, int first_2, int64_t gate_rows_2) {
  using namespace rc;
  int TR;
  if (fm_gate_check("rc_finalmlp_gate_workspace_bytes", n_instances, n_cand, D, gate_in_1, first_1, gate_in_2, first_2, 0.f, 0.f, true, &TR) != RC_OK)
    return 0;
  int bx, nslab;
  fm_bwd_grid(n_instances, D, TR, &bx, &nslab);
  const int G[2] = {gate_in_1, gate_in_2}, H[2] = {first_1, first_2};
  const int mode[2] = {fm_mode_of(gate_rows_1, n_instances, n_cand), fm_mode_of(gate_rows_2, n_instances, n_cand)};
  return fm_bwd_carve(nullptr, n_instances, D, G, H, mode, bx, nslab).bytes;
}

extern "C" int rc_finalmlp_gate_fwd(const float* X, int64_t n_instances, int n_cand, int D, const rc_finalmlp_stream* s1,
                                    const rc_finalmlp_stream* s2, float* A1, float* A2, rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_finalmlp_gate_fwd";
  RC_REQUIRE(X != nullptr && s1 != nullptr && s2 != nullptr && A1 != nullptr && A2 != nullptr, "%s: null pointer", fn);
  int TR;
  RC_TRY(fm_gate_check(fn, n_instances, n_cand, D, s1->G, s1->H, s2->G, s2->H, s1->drop_p, s2->drop_p, false, &TR));
  RC_REQUIRE(aligned16(X), "%s: X must be 16-byte aligned", fn);
  FmArgs a{};
  a.X = X, a.N = n_instances, a.D = D, a.C = n_cand, a.TR = TR;
  RC_TRY(fm_fill_stream(fn, s1, n_instances, n_cand, true, &a.s[0]));
  RC_TRY(fm_fill_stream(fn, s2, n_instances, n_cand, true, &a.s[1]));
  a.s[0].Aout = A1, a.s[1].Aout = A2;
  a.maxGS = (a.s[0].GS > a.s[1].GS ? a.s[0].GS : a.s[1].GS);
  a.maxHP = (a.s[0].HP > a.s[1].HP ? a.s[0].HP : a.s[1].HP);
  const size_t lds = fm_fwd_lds(TR, a.s[0].GP, a.s[1].GP, a.maxHP);
  const int64_t tiles = (n_instances + TR - 1) / TR;
  const int blocks = (int)(tiles < kFmFwdBlocks ? tiles : kFmFwdBlocks);
  auto kern = (a.s[0].seed || a.s[1].seed) ? finalmlp_gate_fwd_kernel<true> : finalmlp_gate_fwd_kernel<false>;
  RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, as_stream(stream), a);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

extern "C" int rc_finalmlp_gate_bwd(const float* X, int64_t n_instances, int n_cand, int D, const rc_finalmlp_stream* s1,
                                    const rc_finalmlp_stream* s2, const float* A1, const float* dA1, const float* A2, const float* dA2,
                                    void* workspace, size_t ws_bytes, float* dX, const rc_finalmlp_grads* g1, const rc_finalmlp_grads* g2,
                                    rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_finalmlp_gate_bwd";
  RC_REQUIRE(X && s1 && s2 && A1 && dA1 && A2 && dA2 && dX && g1 && g2, "%s: null pointer", fn);
  int TR;
  RC_TRY(fm_gate_check(fn, n_instances, n_cand, D, s1->G, s1->H, s2->G, s2->H, s1->drop_p, s2->drop_p, true, &TR));
  RC_REQUIRE(aligned16(X, A1, dA1, A2, dA2, dX), "%s: X, A, dA and dX must be 16-byte aligned", fn);
  RC_REQUIRE(workspace != nullptr && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "%s: workspace must be 256-byte aligned", fn);
  const rc_finalmlp_grads* gr[2] = {g1, g2};
  for (int s = 0; s < 2; ++s)
    RC_REQUIRE(gr[s]->dZin && gr[s]->dWg && gr[s]->dbg && gr[s]->dW && gr[s]->db, "%s: null gradient pointer", fn);
  FmArgs a{};
  a.X = X, a.dX = dX, a.N = n_instances, a.D = D, a.C = n_cand, a.TR = TR;
  RC_TRY(fm_fill_stream(fn, s1, n_instances, n_cand, false, &a.s[0]));
  RC_TRY(fm_fill_stream(fn, s2, n_instances, n_cand, false, &a.s[1]));
  a.s[0].A = A1, a.s[0].dA = dA1, a.s[1].A = A2, a.s[1].dA = dA2;
  int bx, nslab;
  fm_bwd_grid(n_instances, D, TR, &bx, &nslab);
  const int G[2] = {s1->G, s2->G}, H[2] = {s1->H, s2->H}, mode[2] = {a.s[0].mode, a.s[1].mode};
  const FmBwdWs w = fm_bwd_carve(workspace, n_instances, D, G, H, mode, bx, nslab);
  if (ws_bytes < w.bytes) return fail(RC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, w.bytes);
  for (int s = 0; s < 2; ++s)
    a.s[s].dW_part = w.dW[s], a.s[s].dWg_part = w.dWg[s], a.s[s].dbg_part = w.dbg[s], a.s[s].db_part = w.db[s], a.s[s].plane = w.plane[s];
  const hipStream_t st = as_stream(stream);
  const size_t lds = fm_bwd_lds(TR, a.s[0].GP, a.s[0].HP, a.s[1].GP, a.s[1].HP);
  RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(finalmlp_gate_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(finalmlp_gate_bwd_kernel, dim3((unsigned)nslab, (unsigned)bx), dim3(256), lds, st, a);
  RC_LAUNCH_CHECK();
  FmReduceArgs r{};
  r.parts = bx;
  int64_t total = 0;
  for (int s = 0; s < 2; ++s) {
    r.seg[r.nseg++] = FmSeg{w.dW[s], gr[s]->dW, (int64_t)H[s] * D};
    r.seg[r.nseg++] = FmSeg{w.dWg[s], gr[s]->dWg, (int64_t)D * G[s]};
    r.seg[r.nseg++] = FmSeg{w.dbg[s], gr[s]->dbg, (int64_t)D};
    r.seg[r.nseg++] = FmSeg{w.db[s], gr[s]->db, (int64_t)H[s]};
  }
  for (int i = 0; i < r.nseg; ++i) total += r.seg[i].n;
  hipLaunchKernelGGL(finalmlp_reduce_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, r);
  RC_LAUNCH_CHECK();
  FmDzinArgs z{};
  int64_t zmax = 0;
  for (int s = 0; s < 2; ++s) {
    z.dbg[s] = gr[s]->dbg, z.Wg[s] = a.s[s].Wg, z.plane[s] = w.plane[s], z.dZin[s] = gr[s]->dZin, z.G[s] = G[s], z.mode[s] = mode[s];
    const int64_t n = mode[s] == 0 ? G[s] : (mode[s] == 1 ? n_instances / n_cand : n_instances) * G[s];
    if (n > zmax) zmax = n;
  }
  z.N = n_instances, z.D = D, z.C = n_cand, z.nslab = nslab;
  hipLaunchKernelGGL(finalmlp_dzin_kernel, dim3((unsigned)((zmax + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, z);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

extern "C" size_t rc_finalmlp_fusion_workspace_bytes(int64_t n_instances, int x_dim, int y_dim, int num_heads) {
  using namespace rc;
  if (fu_shape("rc_finalmlp_fusion_workspace_bytes", x_dim, y_dim, num_heads) != RC_OK || n_instances < 1) return 0;
  FuArgs a{};
  fu_geometry(&a, x_dim, y_dim, num_heads);
  const int blocks = fu_blocks(a, n_instances);
  Carver c(nullptr);
  c.take<float>((size_t)blocks * (x_dim / num_heads) * y_dim);
  c.take<float>((size_t)blocks * x_dim);
  c.take<float>((size_t)blocks * y_dim);
  c.take<float>((size_t)blocks);
  return c.off;
}

extern "C" int rc_finalmlp_fusion_fwd(const float* x, const float* y, const float* w_xy, const float* w_x, const float* b_x, const float* w_y,
                                      const float* b_y, int64_t n_instances, int x_dim, int y_dim, int num_heads, float* out,
                                      rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_finalmlp_fusion_fwd";
  RC_TRY(fu_shape(fn, x_dim, y_dim, num_heads));
  RC_REQUIRE(n_instances >= 1 && n_instances <= ((int64_t)1 << 26), "%s: instances in [1, 2^26]: instances=%lld", fn, (long long)n_instances);
  RC_REQUIRE(x && y && w_xy && w_x && b_x && w_y && b_y && out, "%s: null pointer", fn);
  RC_REQUIRE(aligned16(x, y), "%s: x and y must be 16-byte aligned", fn);
  FuArgs a{};
  fu_geometry(&a, x_dim, y_dim, num_heads);
  a.x = x, a.y = y, a.wxy = w_xy, a.wx = w_x, a.wy = w_y, a.bx = b_x, a.by = b_y, a.out = out, a.N = n_instances;
  const size_t lds = fu_lds(a);
  const int64_t tiles = (n_instances + a.TR - 1) / a.TR;
  const int blocks = (int)(tiles < kFmFwdBlocks ? tiles : kFmFwdBlocks);
  RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(finalmlp_fusion_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(finalmlp_fusion_fwd_kernel, dim3((unsigned)blocks), dim3(256), lds, as_stream(stream), a);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

extern "C" int rc_finalmlp_fusion_bwd(const float* x, const float* y, const float* w_xy, const float* w_x, const float* w_y, const float* dout,
                                      int64_t n_instances, int x_dim, int y_dim, int num_heads, void* workspace, size_t ws_bytes, float* dx,
                                      float* dy, float* dw_xy, float* dw_x, float* db_x, float* dw_y, float* db_y, rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_finalmlp_fusion_bwd";
  RC_TRY(fu_shape(fn, x_dim, y_dim, num_heads));
  RC_REQUIRE(n_instances >= 1 && n_instances <= ((int64_t)1 << 26), "%s: instances in [1, 2^26]: instances=%lld", fn, (long long)n_instances);
  RC_REQUIRE(x && y && w_xy && w_x && w_y && dout && dx && dy && dw_xy && dw_x && db_x && dw_y && db_y, "%s: null pointer", fn);
  RC_REQUIRE(aligned16(x, y), "%s: x and y must be 16-byte aligned", fn);
  RC_REQUIRE(workspace != nullptr && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "%s: workspace must be 256-byte aligned", fn);
  FuArgs a{};
  fu_geometry(&a, x_dim, y_dim, num_heads);
  const int blocks = fu_blocks(a, n_instances);
  const int nxy = (x_dim / num_heads) * y_dim;
  Carver c(workspace);
  a.dwxy_part = c.take<float>((size_t)blocks * nxy);
  a.dwx_part = c.take<float>((size_t)blocks * x_dim);
  a.dwy_part = c.take<float>((size_t)blocks * y_dim);
  a.db_part = c.take<float>((size_t)blocks);
  if (ws_bytes < c.off) return fail(RC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, c.off);
  a.x = x, a.y = y, a.wxy = w_xy, a.wx = w_x, a.wy = w_y, a.dout = dout, a.dx = dx, a.dy = dy, a.N = n_instances;
  const size_t lds = fu_lds(a);
  const hipStream_t st = as_stream(stream);
  auto kern = a.ntile <= 16 ? finalmlp_fusion_bwd_kernel<4> : finalmlp_fusion_bwd_kernel<16>;
  RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, st, a);
  RC_LAUNCH_CHECK();
  FmReduceArgs r{};
  r.parts = blocks;
  r.seg[r.nseg++] = FmSeg{a.dwxy_part, dw_xy, (int64_t)nxy};
  r.seg[r.nseg++] = FmSeg{a.dwx_part, dw_x, (int64_t)x_dim};
  r.seg[r.nseg++] = FmSeg{a.dwy_part, dw_y, (int64_t)y_dim};
  r.seg[r.nseg++] = FmSeg{a.db_part, db_x, 1};
  r.seg[r.nseg++] = FmSeg{a.db_part, db_y, 1};
  const int64_t total = (int64_t)nxy + x_dim + y_dim + 2;
  hipLaunchKernelGGL(finalmlp_reduce_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, r);
  RC_LAUNCH_CHECK();
  return RC_OK;
}
