// buir.hip -- BUIR's bootstrap loss, evaluation head and target update  (reference: models/general/BUIR.py:66-110)
//
//   P = nn.Linear(d, d): W [d, d] (out x in), b;   n(x) = x / max(|x|, 1e-12)   (F.normalize, per row)
//   pu = W uo + b,  pi = W io + b                       uo / io rows of the online tables, ut / it rows of the target tables
//   loss = mean_b [ 4 - 2 <n(pu), n(it)> - 2 <n(pi), n(ut)> ]                      (the target rows carry no gradient)
//   prediction[b, c] = <P(io_c), uo> + <P(uo), io_c>
//
// Launches:
//   tile      one workgroup owns 64 batch rows at a time (and walks over the batch with the grid as its stride).  It gathers the
//             tile's uo | io rows into LDS as ONE stacked [128, d] block beside W and b, and forms pu | pi = X W^T on
//             v_mfma_f32_32x32x2_f32: a wave owns 32 stacked rows, the output features are the accumulator's rows and the batch
//             rows sit on the lanes, so |pu|, <pu, it> and the training prediction are sums inside a lane plus one exchange
//             between the lane halves.  The target rows are read straight from HBM in the accumulator's layout (float4).
//             Backward (the same kernel, BWD = true, the forward values recomputed): g_pu | g_pi replace pu | pi in the
//             accumulators and are, as they stand, the B operand of dX = G W (per-occurrence row gradients [B, d] x 2); they
//             then take W's place in LDS as the A operand of dW += G^T X, which stays in registers over the workgroup's tiles;
//             db is the column sum of the same LDS block.  W is staged again for the next tile (an L2 hit).
//   reduce    loss: one workgroup adds the per-wave partials in double, fixed order.  Gradients: one thread per element of
//             dW | db adds the workgroups' partials in workgroup order.
//   query     q_b = (W + W^T) uo_b + b, c_b = <b, uo_b>: prediction[b, c] = <q_b, io_c> + c_b
//   scores    <q_b, I[iid[b, c]]> + c_b over [B, C] candidates
//   ema       target = target * m + online * (1 - m) on both tables in one launch, the two products and the sum rounded
//             separately as torch does (no contraction into a fused multiply-add): bit-equal to the reference
// No float atomics anywhere: every sum has a fixed order, results are bitwise reproducible run to run.
#include "common.hpp"

namespace rc {

typedef float buir_f32x16 __attribute__((ext_vector_type(16)));

constexpr float kBuirEps = 1e-12f;    // F.normalize's default eps
constexpr int kBuirTile = 64;         // batch rows per tile: 128 stacked rows, 32 per wave
constexpr int kBuirMaxBlocks = 512;   // workgroups of the tile kernel = partials the reduce adds per element

struct BuirArgs {
  const float *uo, *ut, *io, *it, *W, *b;
  const int64_t *uid, *iid;
  int64_t B;
  int d;
  const float* gout;    // [1] upstream gradient (backward)
  float* pred;          // [B] or null (forward)
  float *gu, *gi;       // [B, d] per-occurrence row gradients (backward)
  float* loss_part;     // [blocks][4]
  float* dW_part;       // [blocks][d][d]
  float* db_part;       // [blocks][d]
};

struct BuirLayout {   // the workspace, carved in this order
  int blocks;
  float *loss_part, *dW_part, *db_part;
  size_t bytes;
};

static BuirLayout buir_layout(int d, int64_t B, void* base) {
  BuirLayout L{};
  const int64_t tiles = (B + kBuirTile - 1) / kBuirTile;
  L.blocks = (int)(tiles < kBuirMaxBlocks ? tiles : kBuirMaxBlocks);
  Carver c(base);
  L.loss_part = c.take<float>((size_t)L.blocks * 4);
  L.dW_part = c.take<float>((size_t)L.blocks * d * d);
  L.db_part = c.take<float>((size_t)L.blocks * d);
  L.bytes = c.off;
  return L;
}

template <int DP>
constexpr size_t buir_lds_bytes() {
  return sizeof(float) * ((size_t)2 * 128 * (DP + 4) + DP + 128);
}

// ---- tile kernel ---------------------------------------------------------------------------------------------------------------
// DP = d rounded up to a multiple of 32 (zero padded in LDS).  Lane l of wave w: h = l >> 5, li = l & 31, stacked row s = 32 w + li
// (s < 64: uo of batch row b0 + s against it; s >= 64: io of batch row b0 + s - 64 against ut).
//   forward step t: k = h DP / 2 + t on both operands; A = W[32 ot + li][k], B = X[s][k]
//   accumulator register r of tile ot: Y[s][o], o = 32 ot + jr(r, h), jr(r, h) = (r & 3) + 8 (r >> 2) + 4 h
//   dX tile kt, step (ot, r): A = W[32 ot + jr(r, h)][32 kt + li], B = G[s][32 ot + jr(r, h)] = the accumulator register itself;
//   its register r holds dX[s][32 kt + jr(r, h)]
//   dW tile (ot, kt), step t: stacked row 2 t + h on both operands; A = G[row][32 ot + li], B = X[row][32 kt + li];
//   its register r holds dW[32 ot + jr(r, h)][32 kt + li]
template <int DP, bool BWD>
__global__ __launch_bounds__(256) void buir_tile_kernel(BuirArgs a) {
  constexpr int SR = DP + 4;                 // LDS row stride (floats)
  constexpr int KH = DP / 2;                 // k per lane half
  constexpr int NCT = DP / 32;               // 32-wide feature tiles
  constexpr int NT2 = NCT * NCT;             // dW tiles
  constexpr int TPW = (NT2 + 3) / 4;         // dW tiles per wave
  constexpr int Q4 = DP / 4;                 // float4 per padded row
  extern __shared__ __attribute__((aligned(16))) float buir_lds[];
  float* xs = buir_lds;                      // [128][SR]  uo | io rows of the tile
  float* ws = xs + 128 * SR;                 // [128][SR]  W in the first DP rows; G during the dW phase
  float* bs = ws + 128 * SR;                 // [DP]
  float* dots = bs + DP;                     // [128] the two halves of the training prediction
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, li = lane & 31;
  const int d = a.d;
  const int64_t B = a.B;
  const int64_t ntiles = (B + kBuirTile - 1) / kBuirTile;
  const int s = wave * 32 + li;

  float lacc = 0.f, dbacc = 0.f;
  buir_f32x16 dwacc[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) dwacc[j][r] = 0.f;
  float cg = 0.f;
  if constexpr (BWD) cg = -2.f * a.gout[0] / (float)B;
  for (int o = tid; o < DP; o += 256) bs[o] = o < d ? a.b[o] : 0.f;

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * kBuirTile;
    __syncthreads();   // every wave is done with the previous tile's LDS
    for (int idx = tid; idx < DP * Q4; idx += 256) {
      const int o = idx / Q4, c4 = idx % Q4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (o < d && 4 * c4 < d) v = *reinterpret_cast<const float4*>(a.W + (int64_t)o * d + 4 * c4);
      *reinterpret_cast<float4*>(&ws[o * SR + 4 * c4]) = v;
    }
    for (int idx = tid; idx < 128 * Q4; idx += 256) {
      const int row = idx / Q4, c4 = idx % Q4;
      const int64_t bb = b0 + (row & 63);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (bb < B && 4 * c4 < d) {
        const float* src = row < 64 ? a.uo + a.uid[bb] * d : a.io + a.iid[bb] * d;
        v = *reinterpret_cast<const float4*>(src + 4 * c4);
      }
      *reinterpret_cast<float4*>(&xs[row * SR + 4 * c4]) = v;
    }
    __syncthreads();

    // ---- pu | pi = X W^T
    buir_f32x16 acc[NCT];
#pragma unroll
    for (int ot = 0; ot < NCT; ++ot)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ot][r] = 0.f;
#pragma unroll 2
    for (int t = 0; t < KH; t += 4) {
      const float4 x = *reinterpret_cast<const float4*>(&xs[s * SR + h * KH + t]);
#pragma unroll
      for (int ot = 0; ot < NCT; ++ot) {
        const float4 w = *reinterpret_cast<const float4*>(&ws[(32 * ot + li) * SR + h * KH + t]);
        acc[ot] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, x.x, acc[ot], 0, 0, 0);
        acc[ot] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, x.y, acc[ot], 0, 0, 0);
        acc[ot] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, x.z, acc[ot], 0, 0, 0);
        acc[ot] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, x.w, acc[ot], 0, 0, 0);
      }
    }

    // ---- norms, dots: feature o = 32 ot + 8 q + 4 h + (0..3) in registers 4 q .. 4 q + 3
    const int64_t bb = b0 + (s & 63);
    const bool valid = bb < B;
    const float* trow = a.it;
    if (valid) trow = wave < 2 ? a.it + a.iid[bb] * d : a.ut + a.uid[bb] * d;
    const float* orow = xs + (s ^ 64) * SR;   // the other side's online row: io for pu, uo for pi
    float4 tv[NCT][4];
    float sx = 0.f, st = 0.f, sxt = 0.f, sp = 0.f;
#pragma unroll
    for (int ot = 0; ot < NCT; ++ot)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int o = 32 * ot + 8 * q + 4 * h;
        float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid && o < d) t4 = *reinterpret_cast<const float4*>(trow + o);
        tv[ot][q] = t4;
        const float4 b4 = *reinterpret_cast<const float4*>(&bs[o]);
        const float4 o4 = *reinterpret_cast<const float4*>(&orow[o]);
        const float y0 = acc[ot][4 * q + 0] + b4.x, y1 = acc[ot][4 * q + 1] + b4.y;
        const float y2 = acc[ot][4 * q + 2] + b4.z, y3 = acc[ot][4 * q + 3] + b4.w;
        acc[ot][4 * q + 0] = y0;
        acc[ot][4 * q + 1] = y1;
        acc[ot][4 * q + 2] = y2;
        acc[ot][4 * q + 3] = y3;
        sx += y0 * y0 + y1 * y1 + y2 * y2 + y3 * y3;
        st += t4.x * t4.x + t4.y * t4.y + t4.z * t4.z + t4.w * t4.w;
        sxt += y0 * t4.x + y1 * t4.y + y2 * t4.z + y3 * t4.w;
        sp += y0 * o4.x + y1 * o4.y + y2 * o4.z + y3 * o4.w;
      }
    sx += __shfl_xor(sx, 32, 64);   // the two lane halves hold the two halves of a row's features
    st += __shfl_xor(st, 32, 64);
    sxt += __shfl_xor(sxt, 32, 64);
    sp += __shfl_xor(sp, 32, 64);
    const float nx = sqrtf(sx);
    const float dx = fmaxf(nx, kBuirEps), dt = fmaxf(sqrtf(st), kBuirEps);
    const float cosv = sxt / (dx * dt);
    float lv = valid ? 2.f - 2.f * cosv : 0.f;
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) lv += __shfl_xor(lv, off, 64);   // this wave's 32 rows, fixed butterfly order
    lacc += lv;
    if (a.pred != nullptr) {   // (workgroup-uniform)
      if (h == 0) dots[s] = sp;
      __syncthreads();
      if (tid < kBuirTile && b0 + tid < B) a.pred[b0 + tid] = dots[64 + tid] + dots[tid];   // <P(io), uo> + <P(uo), io>
    }

    if constexpr (BWD) {
      // ---- g = -2 g0 / B * d <n(y), n(t)> / d y: F.normalize's backward, (g' - y^ (y^ . g')) / |y| past eps, g' / eps below
      const float c = valid ? cg : 0.f;
      const bool past = nx > kBuirEps;
#pragma unroll
      for (int ot = 0; ot < NCT; ++ot)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float tq[4] = {tv[ot][q].x, tv[ot][q].y, tv[ot][q].z, tv[ot][q].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float th = tq[j] / dt;
            const float y = acc[ot][4 * q + j];
            acc[ot][4 * q + j] = past ? c * (th - (y / dx) * cosv) / dx : c * th / kBuirEps;
          }
        }
      // ---- dX = G W: per-occurrence row gradients
      float* grow = (wave < 2 ? a.gu : a.gi) + (valid ? bb : 0) * d;
#pragma unroll
      for (int kt = 0; kt < NCT; ++kt) {
        buir_f32x16 dxa;
#pragma unroll
        for (int r = 0; r < 16; ++r) dxa[r] = 0.f;
#pragma unroll
        for (int ot = 0; ot < NCT; ++ot)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int jr = (r & 3) + 8 * (r >> 2) + 4 * h;
            dxa = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[(32 * ot + jr) * SR + 32 * kt + li], acc[ot][r], dxa, 0, 0, 0);
          }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = 32 * kt + 8 * q + 4 * h;
          if (valid && k < d)
            *reinterpret_cast<float4*>(grow + k) = make_float4(dxa[4 * q], dxa[4 * q + 1], dxa[4 * q + 2], dxa[4 * q + 3]);
        }
      }
      __syncthreads();   // every wave is done with W
#pragma unroll
      for (int ot = 0; ot < NCT; ++ot)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<float4*>(&ws[s * SR + 32 * ot + 8 * q + 4 * h]) =
              make_float4(acc[ot][4 * q], acc[ot][4 * q + 1], acc[ot][4 * q + 2], acc[ot][4 * q + 3]);
      __syncthreads();
      // ---- dW += G^T X over the tile's 128 stacked rows; db += column sums of G
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        const int idx = wave + 4 * j;
        if (idx < NT2) {   // (wave-uniform)
          const int ot = idx / NCT, kt = idx % NCT;
#pragma unroll 8
          for (int t = 0; t < 64; ++t) {
            const int row = 2 * t + h;
            dwacc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[row * SR + 32 * ot + li], xs[row * SR + 32 * kt + li], dwacc[j], 0, 0, 0);
          }
        }
      }
      if (tid < DP)
        for (int row = 0; row < 128; ++row) dbacc += ws[row * SR + tid];
    }
  }

  if constexpr (BWD) {
    float* dWp = a.dW_part + (int64_t)blockIdx.x * d * d;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int idx = wave + 4 * j;
      if (idx < NT2) {
        const int ot = idx / NCT, kt = idx % NCT;
        const int k = 32 * kt + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int o = 32 * ot + (r & 3) + 8 * (r >> 2) + 4 * h;
          if (o < d && k < d) dWp[o * d + k] = dwacc[j][r];
        }
      }
    }
    if (tid < d) a.db_part[(int64_t)blockIdx.x * d + tid] = dbacc;
  } else {
    if (lane == 0) a.loss_part[blockIdx.x * 4 + wave] = lacc;
  }
}

// ---- reduces: fixed order, double -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void buir_loss_reduce_kernel(const float* __restrict__ part, int n, int64_t B,
                                                                  float* __restrict__ loss) {
  __shared__ double red[kBlock];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int p = t; p < n; p += kBlock) acc += (double)part[p];
  red[t] = acc;
  __syncthreads();
  for (int w = kBlock / 2; w >= 1; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) loss[0] = (float)(red[0] / (double)B);
}

__global__ __launch_bounds__(kBlock) void buir_grad_reduce_kernel(const float* __restrict__ dW_part, const float* __restrict__ db_part,
                                                                  int blocks, int d, float* __restrict__ dW, float* __restrict__ db) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  const int nW = d * d;
  if (e >= nW + d) return;
  const float* src = e < nW ? dW_part + e : db_part + (e - nW);
  const int64_t stride = e < nW ? nW : d;
  double acc = 0.0;
  for (int p = 0; p < blocks; ++p) acc += (double)src[p * stride];   // workgroup order
  if (e < nW) dW[e] = (float)acc;
  else db[e - nW] = (float)acc;
}

// ---- evaluation head ---------------------------------------------------------------------------------------------------------------
constexpr int kBuirQueryRows = 8;

__global__ __launch_bounds__(kBlock) void buir_query_kernel(const float* __restrict__ uo, const float* __restrict__ W,
                                                            const float* __restrict__ bvec, const int64_t* __restrict__ uid,
                                                            int64_t B, int d, float* __restrict__ q, float* __restrict__ c) {
  __shared__ float us[kBuirQueryRows][128];
  const int tid = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * kBuirQueryRows;
  for (int idx = tid; idx < kBuirQueryRows * d; idx += kBlock) {
    const int r = idx / d, k = idx % d;
    us[r][k] = b0 + r < B ? uo[uid[b0 + r] * d + k] : 0.f;
  }
  __syncthreads();
  for (int idx = tid; idx < kBuirQueryRows * d; idx += kBlock) {
    const int r = idx / d, o = idx % d;
    if (b0 + r >= B) continue;
    float acc = bvec[o];
    for (int k = 0; k < d; ++k) acc = fmaf(W[o * d + k] + W[k * d + o], us[r][k], acc);
    q[(b0 + r) * d + o] = acc;
  }
  if (tid < kBuirQueryRows && b0 + tid < B) {
    float acc = 0.f;
    for (int k = 0; k < d; ++k) acc = fmaf(bvec[k], us[tid][k], acc);
    c[b0 + tid] = acc;
  }
}

// 16 lanes per (row, candidate) pair, float4 each
__global__ __launch_bounds__(kBlock) void buir_scores_kernel(const float* __restrict__ q, const float* __restrict__ c,
                                                             const float* __restrict__ itab, const int64_t* __restrict__ iid,
                                                             int64_t B, int64_t C, int d, float* __restrict__ out) {
  const int l = threadIdx.x & 15;
  const int64_t n = B * C;
  const int64_t stride = (int64_t)gridDim.x * (kBlock / 16);
  for (int64_t p = (int64_t)blockIdx.x * (kBlock / 16) + (threadIdx.x >> 4); p < n; p += stride) {
    const int64_t b = p / C;
    const float4* q4 = reinterpret_cast<const float4*>(q + b * d);
    const float4* i4 = reinterpret_cast<const float4*>(itab + iid[p] * d);
    float acc = 0.f;
    for (int j = l; j < d / 4; j += 16) acc += dot4(q4[j], i4[j]);
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (l == 0) out[p] = acc + c[b];
  }
}

// ---- target update -----------------------------------------------------------------------------------------------------------------
// target = fl(fl(target * m) + fl(online * om)), m and om the fp32 roundings of the momentum and of (1 - momentum) formed in double
// (torch's scalar handling of `t * m + o * (1. - m)`, BUIR.py:66-71).  Contraction is off: a fused multiply-add rounds once where
// torch rounds twice, and differs on about a quarter of the elements.
__global__ __launch_bounds__(kBlock) void buir_ema_kernel(float* __restrict__ t1, const float* __restrict__ o1, int64_t n1,
                                                          float* __restrict__ t2, const float* __restrict__ o2, int64_t n2, float m,
                                                          float om) {
#pragma clang fp contract(off)
  const int64_t v1 = n1 / 4, v2 = n2 / 4;
  const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = gid; i < v1 + v2; i += stride) {
    float4* tp = i < v1 ? reinterpret_cast<float4*>(t1) + i : reinterpret_cast<float4*>(t2) + (i - v1);
    const float4* op = i < v1 ? reinterpret_cast<const float4*>(o1) + i : reinterpret_cast<const float4*>(o2) + (i - v1);
    const float4 t = *tp, o = *op;
    float4 r;
    r.x = (t.x * m) + (o.x * om);
    r.y = (t.y * m) + (o.y * om);
    r.z = (t.z * m) + (o.z * om);
    r.w = (t.w * m) + (o.w * om);
    *tp = r;
  }
  const int64_t r1 = n1 - 4 * v1, r2 = n2 - 4 * v2;   // tails of tables whose size is no multiple of 4
  if (gid < r1) t1[4 * v1 + gid] = (t1[4 * v1 + gid] * m) + (o1[4 * v1 + gid] * om);
  else if (gid - r1 < r2) t2[4 * v2 + gid - r1] = (t2[4 * v2 + gid - r1] * m) + (o2[4 * v2 + gid - r1] * om);
}

// the one statement of the envelope: every entry point checks it, rc_buir_check_shape reports it to the host
static int buir_shape(const char* fn, int d, int64_t B) {
  if (d % 16 == 0 && d >= 16 && d <= 128 && B >= 1 && B <= ((int64_t)1 << 20)) return RC_OK;
  return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (emb_size a multiple of 16 in [16, 128], batch in [1, 1048576]): "
              "emb_size=%d batch=%lld", fn, d, (long long)B);
}

static int buir_workspace_check(const char* fn, int d, int64_t B, const void* ws, size_t ws_bytes, BuirLayout* L) {
  RC_TRY(buir_shape(fn, d, B));
  RC_REQUIRE(ws != nullptr && reinterpret_cast<uintptr_t>(ws) % 256 == 0, "%s: workspace must be 256-byte aligned", fn);
  *L = buir_layout(d, B, const_cast<void*>(ws));
  RC_REQUIRE(ws_bytes >= L->bytes, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, L->bytes);
  return RC_OK;
}

template <int DP, bool BWD>
static int buir_launch_tile(const BuirArgs& a, int blocks, hipStream_t st) {
  auto kern = buir_tile_kernel<DP, BWD>;
  constexpr size_t lds = buir_lds_bytes<DP>();
  RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, st, a);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

template <bool BWD>
static int buir_tile(const char* fn, const BuirArgs& a, int blocks, hipStream_t st) {
  return dispatch_or_fail<32, 64, 96, 128>(fn, "padded emb_size", (a.d + 31) / 32 * 32,
                                           [&](auto dp) { return buir_launch_tile<decltype(dp)::value, BWD>(a, blocks, st); });
}

}  // namespace rc

extern "C" int rc_buir_check_shape(int d, int64_t batch) { return rc::buir_shape("rc_buir_check_shape", d, batch); }

extern "C" size_t rc_buir_workspace_bytes(int d, int64_t batch) {
  if (rc::buir_shape("rc_buir_workspace_bytes", d, batch) != RC_OK) return 0;
  return rc::buir_layout(d, batch, nullptr).bytes;
}

extern "C" int rc_buir_fwd(const float* user_online, const float* user_target, const float* item_online, const float* item_target,
                           const float* W, const float* b, const int64_t* uid, const int64_t* iid, int64_t batch, int d,
                           void* workspace, size_t ws_bytes, float* prediction, float* loss, rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_buir_fwd";
  BuirLayout L;
  RC_TRY(buir_workspace_check(fn, d, batch, workspace, ws_bytes, &L));
  RC_REQUIRE(user_online != nullptr && user_target != nullptr && item_online != nullptr && item_target != nullptr && W != nullptr &&
             b != nullptr && uid != nullptr && iid != nullptr && loss != nullptr, "%s: null pointer", fn);
  RC_REQUIRE(aligned16(user_online, user_target, item_online, item_target, W), "%s: tables and W must be 16-byte aligned", fn);
  const hipStream_t st = as_stream(stream);
  BuirArgs a{user_online, user_target, item_online, item_target, W, b, uid, iid, batch, d, nullptr, prediction, nullptr, nullptr,
             L.loss_part, L.dW_part, L.db_part};
  RC_TRY(buir_tile<false>(fn, a, L.blocks, st));
  hipLaunchKernelGGL(buir_loss_reduce_kernel, dim3(1), dim3(kBlock), 0, st, L.loss_part, L.blocks * 4, batch, loss);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

extern "C" int rc_buir_bwd(const float* user_online, const float* user_target, const float* item_online, const float* item_target,
                           const float* W, const float* b, const int64_t* uid, const int64_t* iid, const float* grad_out,
                           int64_t batch, int d, void* workspace, size_t ws_bytes, float* grad_user, float* grad_item, float* dW,
                           float* db, rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_buir_bwd";
  BuirLayout L;
  RC_TRY(buir_workspace_check(fn, d, batch, workspace, ws_bytes, &L));
  RC_REQUIRE(user_online != nullptr && user_target != nullptr && item_online != nullptr && item_target != nullptr && W != nullptr &&
             b != nullptr && uid != nullptr && iid != nullptr && grad_out != nullptr && grad_user != nullptr &&
             grad_item != nullptr && dW != nullptr && db != nullptr, "%s: null pointer", fn);
  RC_REQUIRE(aligned16(user_online, user_target, item_online, item_target, W, grad_user, grad_item),
             "%s: tables, W and row gradients must be 16-byte aligned", fn);
  const hipStream_t st = as_stream(stream);
  BuirArgs a{user_online, user_target, item_online, item_target, W, b, uid, iid, batch, d, grad_out, nullptr, grad_user, grad_item,
             L.loss_part, L.dW_part, L.db_part};
  RC_TRY(buir_tile<true>(fn, a, L.blocks, st));
  hipLaunchKernelGGL(buir_grad_reduce_kernel, dim3((unsigned)((d * d + d + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, L.dW_part,
                     L.db_part, L.blocks, d, dW, db);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

extern "C" int rc_buir_query(const float* user_online, const float* W, const float* b, const int64_t* uid, int64_t batch, int d,
                             float* q, float* c, rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_buir_query";
  RC_TRY(buir_shape(fn, d, batch));
  RC_REQUIRE(user_online != nullptr && W != nullptr && b != nullptr && uid != nullptr && q != nullptr && c != nullptr,
             "%s: null pointer", fn);
  hipLaunchKernelGGL(buir_query_kernel, dim3((unsigned)((batch + kBuirQueryRows - 1) / kBuirQueryRows)), dim3(kBlock), 0,
                     as_stream(stream), user_online, W, b, uid, batch, d, q, c);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

extern "C" int rc_buir_scores(const float* q, const float* c, const float* item_online, const int64_t* iid, int64_t batch,
                              int64_t n_candidates, int d, float* scores, rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_buir_scores";
  RC_TRY(buir_shape(fn, d, batch));
  RC_REQUIRE(n_candidates >= 1 && n_candidates <= ((int64_t)1 << 31) / batch, "%s: 1 <= candidates, batch * candidates <= 2^31", fn);
  RC_REQUIRE(q != nullptr && c != nullptr && item_online != nullptr && iid != nullptr && scores != nullptr, "%s: null pointer", fn);
  RC_REQUIRE(aligned16(q, item_online), "%s: q and the item table must be 16-byte aligned", fn);
  int64_t blocks = (batch * n_candidates + kBlock / 16 - 1) / (kBlock / 16);
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(buir_scores_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), q, c, item_online, iid, batch,
                     n_candidates, d, scores);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

extern "C" int rc_buir_ema(float* target_a, const float* online_a, int64_t n_a, float* target_b, const float* online_b, int64_t n_b,
                           double momentum, rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_buir_ema";
  RC_REQUIRE(n_a >= 0 && n_b >= 0 && n_a + n_b >= 1, "%s: element counts must not be negative, and not both 0", fn);
  RC_REQUIRE((n_a == 0 || (target_a != nullptr && online_a != nullptr)) && (n_b == 0 || (target_b != nullptr && online_b != nullptr)),
             "%s: null pointer", fn);
  RC_REQUIRE(aligned16(target_a, online_a, target_b, online_b), "%s: tables must be 16-byte aligned", fn);
  const float m = (float)momentum, om = (float)(1.0 - momentum);
  int64_t blocks = (n_a / 4 + n_b / 4 + kBlock - 1) / kBlock;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(buir_ema_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), target_a, online_a, n_a, target_b,
                     online_b, n_b, m, om);
  RC_LAUNCH_CHECK();
  return RC_OK;
}
