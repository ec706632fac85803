// comirec.hip -- ComiRec's multi-interest extraction  (reference: models/sequential/ComiRec.py:57-93)
//
//   h_l = I[hist_l], valid_l = hist_l > 0, x_l = h_l + P[(len - l) valid_l]            (x = h without a position table)
//   s[l, k] = W2[k] . tanh(W1 x_l + b1) + b2[k], -inf on invalid positions              (:75-76)
//   a[k, .] = softmax_l s[., k], 0 where a sequence has no valid position                (:78-79; the reference subtracts the batch-wide
//             maximum first, softmax is shift invariant per row: the running row maximum is subtracted here)
//   interest[k] = sum_l a[k, l] h_l                                                      (:80, the un-positioned rows)
//   training:   sel = argmax_k <interest[k], I[target]> (lowest index on a tie), user = interest[sel]   (:84-87)
//   evaluation: pred[c] = max_k <interest[k], I[iid[c]]>                                 (:90-91)
//
// Lane mapping (all three kernels): LPR = d / 4 rounded up to a power of two lanes share one table row (a float4 each), a wave
// works on G = 64 / LPR positions (candidates) at a time; the A projections are LPR-lane DPP all-reduces against W1 rows that
// every lane group reads from LDS at the same address (a broadcast).  Launches:
//   forward   one wave per sequence, ONE pass over the history: online softmax per interest (running maximum, sum and weighted
//             row sum per lane group, merged across the groups in a fixed butterfly order), so every row is read once and nothing
//             of size [B, L, d] is written.  Scores wait in LDS until the row's maximum and sum are known, then become a [K, L].
//   backward  only row sel of a / W2 / b2 carries gradient.  With e_l = <d_user, h_l> and c = <d_user, user>:
//             ds_l = a[sel, l] (e_l - c), dpre_l = ds_l W2[sel] (1 - t_l^2), dx_l = W1^T dpre_l, g_hist_l = a[sel, l] d_user + dx_l.
//             The workgroup's 4 G positions of a step are staged in LDS (x rows, dpre, ds t) and every thread adds its own
//             elements of dW1 / db1 / dW2 / db2 (held in LDS, one owner per element) in ascending position order; each workgroup
//             leaves one partial, a second launch adds the partials in workgroup order (double).
//   score_max one workgroup per (sequence, 1,024 candidates): the K interests in LDS, each candidate row read once.
// No float atomics anywhere: every sum has a fixed order, results are bitwise reproducible run to run.
#include "common.hpp"

namespace rc {

constexpr int kCrMaxA = 64, kCrMaxK = 16, kCrMaxL = 256, kCrMaxD = 256;
constexpr int kCrWaves = kBlock / 64;      // sequences a workgroup works on at a time
constexpr int kCrFwdBlocks = 2048;         // grid caps: the weights are staged once per workgroup
constexpr int kCrBwdBlocks = 1024;         // (= the number of weight-gradient partials)
constexpr int kCrScoreChunk = 1024;        // candidates per workgroup of the evaluation head
constexpr int kCrRedE = 16, kCrRedJ = kBlock / kCrRedE;   // partial reduction: 16 elements x 16 partial phases per workgroup

struct CrFwdArgs {
  const float *item, *pos, *W1, *b1, *W2, *b2;
  const int64_t *hist, *len, *tgt;
  int64_t B, n_items;
  int L, d, A, K, n_pos;
  float *interests, *attn, *user;
  int* sel;
};

struct CrBwdArgs {
  const float *item, *pos, *W1, *b1, *W2;
  const int64_t *hist, *len;
  const float *attn, *user, *d_user;
  const int* sel;
  int64_t B, n_items;
  int L, d, A, K, n_pos;
  float *g_hist, *g_x, *part;
  int part_stride;
};

__host__ __device__ inline int cr_align4(int x) { return (x + 3) / 4 * 4; }
static int cr_part_floats(int d, int A, int K) { return cr_align4(A * d + A + K * A + K); }
static int64_t cr_bwd_blocks(int64_t B) {
  const int64_t n = (B + kCrWaves - 1) / kCrWaves;
  return n < 1 ? 1 : (n > kCrBwdBlocks ? kCrBwdBlocks : n);
}

__device__ __forceinline__ float4 cr_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 cr_fma4(float s, float4 v, float4 acc) {
  return make_float4(fmaf(s, v.x, acc.x), fmaf(s, v.y, acc.y), fmaf(s, v.z, acc.z), fmaf(s, v.w, acc.w));
}

// the rows of position l of sequence b: h (item row), x (h + position row); zeros on an invalid position.  An id outside the
// table is a caller error that reads no memory: the position counts as padding.
__device__ __forceinline__ bool cr_load_rows(const float* __restrict__ item, const float* __restrict__ pos, int64_t id, int64_t n_items,
                                             int64_t len, int l, int n_pos, int d, int li, bool on, float4& h, float4& x) {
  const bool valid = id > 0 && id < n_items;
  h = cr_zero4();
  x = cr_zero4();
  if (valid && on) {
    h = *reinterpret_cast<const float4*>(item + id * d + 4 * li);
    x = h;
    if (pos != nullptr) {
      int64_t pid = len - l;
      pid = pid < 0 ? 0 : (pid >= n_pos ? n_pos - 1 : pid);
      const float4 p = *reinterpret_cast<const float4*>(pos + pid * d + 4 * li);
      x = make_float4(h.x + p.x, h.y + p.y, h.z + p.z, h.w + p.w);
    }
  }
  return valid;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
// LDS: W1 [A, d] | b1 [A] | W2 [K, A] | b2 [K] | per wave: scores [K, L], row maximum [KP], row sum [KP]
template <int LPR, int KP>
__global__ __launch_bounds__(kBlock) void cr_fwd_kernel(CrFwdArgs a) {
  constexpr int G = 64 / LPR;
  extern __shared__ __attribute__((aligned(16))) float cr_lds[];
  const int d = a.d, A = a.A, K = a.K, L = a.L, dq = d / 4;
  float* W1s = cr_lds;
  float* b1s = W1s + A * d;
  float* W2s = b1s + A;
  float* b2s = W2s + K * A;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane / LPR, li = lane % LPR;
  float* sc = cr_lds + cr_align4(A * d + A + K * A + K) + wave * cr_align4(K * L + 2 * KP);
  float* mz = sc + K * L;
  for (int i = threadIdx.x; i < A * d; i += kBlock) W1s[i] = a.W1[i];
  for (int i = threadIdx.x; i < A; i += kBlock) b1s[i] = a.b1[i];
  for (int i = threadIdx.x; i < K * A; i += kBlock) W2s[i] = a.W2[i];
  for (int i = threadIdx.x; i < K; i += kBlock) b2s[i] = a.b2[i];
  __syncthreads();
  const bool on = li < dq;
  const float4* W1q = reinterpret_cast<const float4*>(W1s);
  const float ninf = -INFINITY;

  for (int64_t base = (int64_t)blockIdx.x * kCrWaves; base < a.B; base += (int64_t)gridDim.x * kCrWaves) {   // (workgroup-uniform)
    const int64_t b = base + wave;
    const bool ok = b < a.B;
    const int64_t len = ok ? a.len[b] : 0;
    float m[KP], z[KP];
    float4 acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      m[k] = ninf;
      z[k] = 0.f;
      acc[k] = cr_zero4();
    }
    for (int l0 = 0; l0 < L; l0 += G) {
      const int l = l0 + grp;
      const bool inl = ok && l < L;
      const int64_t id = inl ? a.hist[b * L + l] : 0;
      float4 h, x;
      const bool valid = cr_load_rows(a.item, a.pos, id, a.n_items, len, l, a.n_pos, d, li, on, h, x);
      float s[KP];
#pragma unroll
      for (int k = 0; k < KP; ++k) s[k] = k < K ? b2s[k] : 0.f;
      for (int j = 0; j < A; ++j) {
        const float pa = row_allreduce_sum<LPR>(on ? dot4(x, W1q[j * dq + li]) : 0.f);
        const float t = tanhf(pa + b1s[j]);
#pragma unroll
        for (int k = 0; k < KP; ++k)
          if (k < K) s[k] = fmaf(W2s[k * A + j], t, s[k]);
      }
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        if (k < K && valid) {   // online softmax: the sums so far are rescaled to the new maximum
          const float mn = fmaxf(m[k], s[k]);
          const float c = expf(m[k] - mn), e = expf(s[k] - mn);
          z[k] = fmaf(z[k], c, e);
          acc[k] = make_float4(fmaf(acc[k].x, c, e * h.x), fmaf(acc[k].y, c, e * h.y), fmaf(acc[k].z, c, e * h.z),
                               fmaf(acc[k].w, c, e * h.w));
          m[k] = mn;
        }
      }
      if (li == 0 && inl)
#pragma unroll
        for (int k = 0; k < KP; ++k)
          if (k < K) sc[k * L + l] = valid ? s[k] : ninf;
    }
    // merge the G lane groups (fixed butterfly order), normalise
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (k < K) {
        const float M = groups_allreduce_max<LPR, 64>(m[k]);
        const float c = m[k] == ninf ? 0.f : expf(m[k] - M);
        const float Z = groups_allreduce_sum<LPR, 64>(z[k] * c);
        float4 v;
        v.x = groups_allreduce_sum<LPR, 64>(acc[k].x * c);
        v.y = groups_allreduce_sum<LPR, 64>(acc[k].y * c);
        v.z = groups_allreduce_sum<LPR, 64>(acc[k].z * c);
        v.w = groups_allreduce_sum<LPR, 64>(acc[k].w * c);
        acc[k] = Z > 0.f ? make_float4(v.x / Z, v.y / Z, v.z / Z, v.w / Z) : cr_zero4();   // no valid position: zero interests
        if (lane == 0) {
          mz[k] = M;
          mz[KP + k] = Z;
        }
        if (ok && grp == 0 && on) *reinterpret_cast<float4*>(a.interests + (b * K + k) * d + 4 * li) = acc[k];
      }
    }
    __syncthreads();   // scores, maxima and sums of every wave are in LDS
    if (a.attn != nullptr && ok) {
      for (int i = lane; i < K * L; i += 64) {
        const int k = i / L;
        const float sv = sc[i], Z = mz[KP + k];
        a.attn[b * K * L + i] = (sv == ninf || !(Z > 0.f)) ? 0.f : expf(sv - mz[k]) / Z;
      }
    }
    if (a.tgt != nullptr) {
      const int64_t tid = ok ? a.tgt[b] : -1;
      const float4 t4 = (on && tid >= 0 && tid < a.n_items) ? *reinterpret_cast<const float4*>(a.item + tid * d + 4 * li) : cr_zero4();
      float best = 0.f;
      int bi = 0;
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        if (k < K) {
          const float v = row_allreduce_sum<LPR>(dot4(acc[k], t4));
          if (k == 0 || v > best) {   // strictly greater: the lowest index wins a tie
            best = v;
            bi = k;
          }
        }
      }
      float4 u = acc[0];
#pragma unroll
      for (int k = 1; k < KP; ++k)
        if (k == bi) u = acc[k];
      if (ok && grp == 0 && on) *reinterpret_cast<float4*>(a.user + b * d + 4 * li) = u;
      if (ok && lane == 0) a.sel[b] = bi;
    }
    __syncthreads();   // the next sequence overwrites the scores
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// LDS: W1 [A, d] | b1 [A] | W2 [K, A] | accumulators dW1 [A, d] | db1 [A] | dW2 [K, A] | db2 [K] (laid out as a partial) |
//      staging of a step's NP = 4 G positions: x [NP, d] | dpre [NP, A] | ds t [NP, A] | ds [NP] | sel [NP]
template <int LPR>
__global__ __launch_bounds__(kBlock) void cr_bwd_kernel(CrBwdArgs a) {
  constexpr int G = 64 / LPR, NP = kCrWaves * G;
  extern __shared__ __attribute__((aligned(16))) float cr_lds[];
  const int d = a.d, A = a.A, K = a.K, L = a.L, dq = d / 4;
  float* W1s = cr_lds;
  float* b1s = W1s + A * d;
  float* W2s = b1s + A;
  float* accs = cr_lds + cr_align4(A * d + A + K * A);
  float* dW1s = accs;
  float* db1s = dW1s + A * d;
  float* dW2s = db1s + A;
  float* db2s = dW2s + K * A;
  float* xs = accs + a.part_stride;
  float* dps = xs + NP * d;
  float* tws = dps + NP * A;
  float* dsv = tws + NP * A;
  int* selp = reinterpret_cast<int*>(dsv + NP);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane / LPR, li = lane % LPR;
  for (int i = threadIdx.x; i < A * d; i += kBlock) W1s[i] = a.W1[i];
  for (int i = threadIdx.x; i < A; i += kBlock) b1s[i] = a.b1[i];
  for (int i = threadIdx.x; i < K * A; i += kBlock) W2s[i] = a.W2[i];
  for (int i = threadIdx.x; i < a.part_stride; i += kBlock) accs[i] = 0.f;
  __syncthreads();
  const bool on = li < dq;
  const float4* W1q = reinterpret_cast<const float4*>(W1s);
  float4* dW1q = reinterpret_cast<float4*>(dW1s);
  float4* xq = reinterpret_cast<float4*>(xs);
  const int p = wave * G + grp;   // this lane group's staging slot

  for (int64_t base = (int64_t)blockIdx.x * kCrWaves; base < a.B; base += (int64_t)gridDim.x * kCrWaves) {   // (workgroup-uniform)
    const int64_t b = base + wave;
    const bool ok = b < a.B;
    const int64_t len = ok ? a.len[b] : 0;
    int sb = ok ? a.sel[b] : 0;
    sb = sb < 0 ? 0 : (sb >= K ? K - 1 : sb);
    float4 du = cr_zero4(), uu = cr_zero4();
    if (ok && on) {
      du = *reinterpret_cast<const float4*>(a.d_user + b * d + 4 * li);
      uu = *reinterpret_cast<const float4*>(a.user + b * d + 4 * li);
    }
    const float cdot = row_allreduce_sum<LPR>(dot4(du, uu));   // sum_l a[sel, l] <d_user, h_l> = <d_user, user>
    for (int l0 = 0; l0 < L; l0 += G) {
      const int l = l0 + grp;
      const bool inl = ok && l < L;
      const int64_t id = inl ? a.hist[b * L + l] : 0;
      float4 h, x;
      const bool valid = cr_load_rows(a.item, a.pos, id, a.n_items, len, l, a.n_pos, d, li, on, h, x);
      const float aw = valid ? a.attn[(b * K + sb) * L + l] : 0.f;
      const float e = row_allreduce_sum<LPR>(dot4(du, h));
      const float ds = valid ? aw * (e - cdot) : 0.f;
      float4 dx = cr_zero4();
      for (int j = 0; j < A; ++j) {
        const float4 w = on ? W1q[j * dq + li] : cr_zero4();
        const float pa = row_allreduce_sum<LPR>(dot4(x, w));
        const float t = tanhf(pa + b1s[j]);
        const float dp = ds * W2s[sb * A + j] * (1.f - t * t);
        dx = cr_fma4(dp, w, dx);
        if (li == 0) {
          dps[p * A + j] = dp;
          tws[p * A + j] = ds * t;
        }
      }
      if (li == 0) {
        dsv[p] = ds;
        selp[p] = sb;
      }
      if (on) xq[p * dq + li] = x;
      if (inl && on) {
        const float4 gh = valid ? cr_fma4(aw, du, dx) : cr_zero4();   // rows at invalid positions are written as zeros
        *reinterpret_cast<float4*>(a.g_hist + (b * L + l) * d + 4 * li) = gh;
        if (a.g_x != nullptr) *reinterpret_cast<float4*>(a.g_x + (b * L + l) * d + 4 * li) = valid ? dx : cr_zero4();
      }
      __syncthreads();
      // every accumulator element has ONE owner thread, which adds the step's positions in ascending slot order
      for (int i = threadIdx.x; i < A * dq; i += kBlock) {
        const int j = i / dq, c = i - j * dq;
        float4 acc = dW1q[i];
        for (int q = 0; q < NP; ++q) acc = cr_fma4(dps[q * A + j], xq[q * dq + c], acc);
        dW1q[i] = acc;
      }
      if (threadIdx.x < A) {
        float acc = db1s[threadIdx.x];
        for (int q = 0; q < NP; ++q) acc += dps[q * A + threadIdx.x];
        db1s[threadIdx.x] = acc;
      }
      for (int i = threadIdx.x; i < K * A; i += kBlock) {
        const int k = i / A, j = i - k * A;
        float acc = dW2s[i];
        for (int q = 0; q < NP; ++q)
          if (selp[q] == k) acc += tws[q * A + j];
        dW2s[i] = acc;
      }
      if (threadIdx.x < K) {
        float acc = db2s[threadIdx.x];
        for (int q = 0; q < NP; ++q)
          if (selp[q] == (int)threadIdx.x) acc += dsv[q];
        db2s[threadIdx.x] = acc;
      }
      __syncthreads();
    }
  }
  float* out = a.part + (int64_t)blockIdx.x * a.part_stride;
  for (int i = threadIdx.x; i < a.part_stride; i += kBlock) out[i] = accs[i];
}

// out[e] = sum_j part[j][e], j ascending: thread (jl, el) adds partials jl, jl + 16, ... of element e0 + el in double, the 16
// phases are added in phase order.  The partial's layout is dW1 | db1 | dW2 | db2.
__global__ __launch_bounds__(kBlock) void cr_reduce_kernel(const float* __restrict__ part, int n_part, int stride, int n1, int n2, int n3,
                                                           int n4, float* __restrict__ o1, float* __restrict__ o2, float* __restrict__ o3,
                                                           float* __restrict__ o4) {
  __shared__ double red[kCrRedJ][kCrRedE];
  const int el = threadIdx.x % kCrRedE, jl = threadIdx.x / kCrRedE;
  const int e = blockIdx.x * kCrRedE + el;
  const int n = n1 + n2 + n3 + n4;
  double acc = 0.0;
  if (e < n)
    for (int j = jl; j < n_part; j += kCrRedJ) acc += (double)part[(int64_t)j * stride + e];
  red[jl][el] = acc;
  __syncthreads();
  if (jl == 0 && e < n) {
    double t = 0.0;
    for (int j = 0; j < kCrRedJ; ++j) t += red[j][el];
    const float v = (float)t;
    if (e < n1) o1[e] = v;
    else if (e < n1 + n2) o2[e - n1] = v;
    else if (e < n1 + n2 + n3) o3[e - n1 - n2] = v;
    else o4[e - n1 - n2 - n3] = v;
  }
}

// ---- evaluation head -----------------------------------------------------------------------------------------------------------
// grid (B, chunks of 1,024 candidates); the sequence's K interests in LDS.  An id outside the table reads no memory and scores NaN.
template <int LPR>
__global__ __launch_bounds__(kBlock) void cr_score_kernel(const float* __restrict__ interests, const float* __restrict__ item,
                                                          const int64_t* __restrict__ iid, int64_t C, int d, int K, int64_t n_items,
                                                          float* __restrict__ pred) {
  constexpr int G = 64 / LPR;
  extern __shared__ __attribute__((aligned(16))) float cr_lds[];
  float4* Is = reinterpret_cast<float4*>(cr_lds);
  const int dq = d / 4;
  const int64_t b = blockIdx.x;
  const float4* src = reinterpret_cast<const float4*>(interests + b * K * d);
  for (int i = threadIdx.x; i < K * dq; i += kBlock) Is[i] = src[i];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane / LPR, li = lane % LPR;
  const bool on = li < dq;
  const int64_t c0 = (int64_t)blockIdx.y * kCrScoreChunk;
  const int64_t c1 = c0 + kCrScoreChunk < C ? c0 + kCrScoreChunk : C;
  for (int64_t cb = c0; cb < c1; cb += kCrWaves * G) {   // (workgroup-uniform)
    const int64_t c = cb + wave * G + grp;
    const bool live = c < c1;
    const int64_t id = live ? iid[b * C + c] : -1;
    const bool inr = id >= 0 && id < n_items;
    const float4 r = (inr && on) ? *reinterpret_cast<const float4*>(item + id * d + 4 * li) : cr_zero4();
    float best = 0.f;
    for (int k = 0; k < K; ++k) {
      const float v = row_allreduce_sum<LPR>(on ? dot4(Is[k * dq + li], r) : 0.f);
      best = (k == 0 || v > best) ? v : best;
    }
    if (live && li == 0) pred[b * C + c] = inr ? best : NAN;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int cr_lpr(int d) {
  int lpr = 1;
  while (lpr < d / 4) lpr <<= 1;
  return lpr;
}
static int cr_kp(int K) {
  int kp = 1;
  while (kp < K) kp <<= 1;
  return kp;
}

// the one statement of the envelope: every entry point checks it, rc_comirec_check_shape reports it to the host
static int cr_shape(const char* fn, int d, int A, int K, int L) {
  if (d % 4 == 0 && d >= 4 && d <= kCrMaxD && A >= 1 && A <= kCrMaxA && K >= 1 && K <= kCrMaxK && L >= 1 && L <= kCrMaxL) return RC_OK;
  return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (emb_size a multiple of 4 in [4, 256], attn_size in [1, 64], K in [1, 16], "
              "history_max in [1, 256]): emb_size=%d attn_size=%d K=%d history_max=%d", fn, d, A, K, L);
}

static int cr_batch(const char* fn, int64_t B) {
  RC_REQUIRE(B >= 1 && B <= ((int64_t)1 << 24), "%s: batch must be in [1, 16777216], got %lld", fn, (long long)B);
  return RC_OK;
}

static size_t cr_fwd_lds(int d, int A, int K, int L) {
  return ((size_t)cr_align4(A * d + A + K * A + K) + (size_t)kCrWaves * cr_align4(K * L + 2 * cr_kp(K))) * sizeof(float);
}
static size_t cr_bwd_lds(int d, int A, int K) {
  const int np = kCrWaves * (64 / cr_lpr(d));
  return ((size_t)cr_align4(A * d + A + K * A) + cr_part_floats(d, A, K) + (size_t)np * d + 2 * (size_t)np * A + 2 * (size_t)np) * sizeof(float);
}

template <int LPR>
static int cr_launch_fwd(const CrFwdArgs& a, unsigned grid, size_t lds, hipStream_t st) {
  return dispatch_or_fail<1, 2, 4, 8, 16>("rc_comirec_fwd", "K rounded to a power of two", cr_kp(a.K), [&](auto kp) {
    auto kern = cr_fwd_kernel<LPR, decltype(kp)::value>;
    RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, a);
    RC_LAUNCH_CHECK();
    return (int)RC_OK;
  });
}

}  // namespace rc

extern "C" int rc_comirec_check_shape(int d, int attn_size, int K, int L) {
  return rc::cr_shape("rc_comirec_check_shape", d, attn_size, K, L);
}

extern "C" size_t rc_comirec_workspace_bytes(int d, int attn_size, int K, int L, int64_t batch) {
  if (rc::cr_shape("rc_comirec_workspace_bytes", d, attn_size, K, L) != RC_OK || batch < 1) return 0;
  return rc::align_up((size_t)rc::cr_bwd_blocks(batch) * rc::cr_part_floats(d, attn_size, K) * sizeof(float), 256);
}

extern "C" int rc_comirec_fwd(const float* item_tab, int64_t n_items, const float* pos_tab, int n_pos, const float* W1, const float* b1,
                              const float* W2, const float* b2, const int64_t* hist, const int64_t* lengths, const int64_t* targets,
                              int64_t batch, int L, int d, int attn_size, int K, float* interests, float* attn, int* sel, float* user,
                              rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_comirec_fwd";
  RC_TRY(cr_shape(fn, d, attn_size, K, L));
  RC_TRY(cr_batch(fn, batch));
  RC_REQUIRE(item_tab && W1 && b1 && W2 && b2 && hist && lengths && interests, "%s: null pointer", fn);
  RC_REQUIRE(n_items >= 1 && (pos_tab == nullptr || n_pos >= 1), "%s: empty table", fn);
  RC_REQUIRE((targets == nullptr) == (sel == nullptr) && (sel == nullptr) == (user == nullptr),
             "%s: targets, sel and user come together", fn);
  RC_REQUIRE(aligned16(item_tab, pos_tab, interests, user), "%s: tables and row outputs must be 16-byte aligned", fn);
  const size_t lds = cr_fwd_lds(d, attn_size, K, L);
  RC_REQUIRE(lds <= 160 * 1024, "%s: %zu bytes of LDS needed", fn, lds);
  CrFwdArgs a{item_tab, pos_tab, W1, b1, W2, b2, hist, lengths, targets, batch, n_items, L, d, attn_size, K, n_pos, interests, attn,
              user, sel};
  int64_t grid = (batch + kCrWaves - 1) / kCrWaves;
  if (grid > kCrFwdBlocks) grid = kCrFwdBlocks;
  const hipStream_t st = as_stream(stream);
  return dispatch_or_fail<1, 2, 4, 8, 16, 32, 64>(fn, "lane group", cr_lpr(d), [&](auto lpr) {
    return cr_launch_fwd<decltype(lpr)::value>(a, (unsigned)grid, lds, st);
  });
}

extern "C" int rc_comirec_bwd(const float* item_tab, int64_t n_items, const float* pos_tab, int n_pos, const float* W1, const float* b1,
                              const float* W2, const int64_t* hist, const int64_t* lengths, const float* attn, const int* sel,
                              const float* user, const float* d_user, int64_t batch, int L, int d, int attn_size, int K, float* g_hist,
                              float* g_x, float* dW1, float* db1, float* dW2, float* db2, void* workspace, size_t ws_bytes,
                              rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_comirec_bwd";
  RC_TRY(cr_shape(fn, d, attn_size, K, L));
  RC_TRY(cr_batch(fn, batch));
  RC_REQUIRE(item_tab && W1 && b1 && W2 && hist && lengths && attn && sel && user && d_user && g_hist && dW1 && db1 && dW2 && db2 &&
             workspace, "%s: null pointer", fn);
  RC_REQUIRE(n_items >= 1 && (pos_tab == nullptr || n_pos >= 1), "%s: empty table", fn);
  RC_REQUIRE((pos_tab == nullptr) == (g_x == nullptr), "%s: g_x comes with the position table", fn);
  RC_REQUIRE(aligned16(item_tab, pos_tab, user, d_user, g_hist, g_x, workspace), "%s: tables, rows and workspace must be 16-byte aligned", fn);
  const size_t need = rc_comirec_workspace_bytes(d, attn_size, K, L, batch);
  if (ws_bytes < need) return fail(RC_ERR_WORKSPACE, "%s: workspace %zu < %zu", fn, ws_bytes, need);
  const size_t lds = cr_bwd_lds(d, attn_size, K);
  RC_REQUIRE(lds <= 160 * 1024, "%s: %zu bytes of LDS needed", fn, lds);
  const int stride = cr_part_floats(d, attn_size, K);
  const int64_t grid = cr_bwd_blocks(batch);
  CrBwdArgs a{item_tab, pos_tab, W1, b1, W2, hist, lengths, attn, user, d_user, sel, batch, n_items, L, d, attn_size, K, n_pos, g_hist,
              g_x, static_cast<float*>(workspace), stride};
  const hipStream_t st = as_stream(stream);
  RC_TRY((dispatch_or_fail<1, 2, 4, 8, 16, 32, 64>(fn, "lane group", cr_lpr(d), [&](auto lpr) {
    auto kern = cr_bwd_kernel<decltype(lpr)::value>;
    RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kBlock), lds, st, a);
    RC_LAUNCH_CHECK();
    return (int)RC_OK;
  })));
  const int n1 = attn_size * d, n2 = attn_size, n3 = K * attn_size, n4 = K;
  const int n = n1 + n2 + n3 + n4;
  hipLaunchKernelGGL(cr_reduce_kernel, dim3((unsigned)((n + kCrRedE - 1) / kCrRedE)), dim3(kBlock), 0, st, a.part, (int)grid, stride, n1,
                     n2, n3, n4, dW1, db1, dW2, db2);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

extern "C" int rc_comirec_score_max(const float* interests, const float* item_tab, int64_t n_items, const int64_t* iid, int64_t batch,
                                    int64_t C, int d, int K, float* pred, rc_stream_t stream) {
  using namespace rc;
  const char* fn = "rc_comirec_score_max";
  RC_TRY(cr_shape(fn, d, 1, K, 1));
  RC_TRY(cr_batch(fn, batch));
  RC_REQUIRE(interests && item_tab && iid && pred, "%s: null pointer", fn);
  RC_REQUIRE(n_items >= 1 && C >= 1 && (C + kCrScoreChunk - 1) / kCrScoreChunk <= 65535, "%s: bad candidate count %lld", fn, (long long)C);
  RC_REQUIRE(aligned16(interests, item_tab), "%s: interests and table must be 16-byte aligned", fn);
  const dim3 grid((unsigned)batch, (unsigned)((C + kCrScoreChunk - 1) / kCrScoreChunk));
  const size_t lds = (size_t)K * d * sizeof(float);
  const hipStream_t st = as_stream(stream);
  return dispatch_or_fail<1, 2, 4, 8, 16, 32, 64>(fn, "lane group", cr_lpr(d), [&](auto lpr) {
    hipLaunchKernelGGL((cr_score_kernel<decltype(lpr)::value>), grid, dim3(kBlock), lds, st, interests, item_tab, iid, C, d, K, n_items,
                       pred);
    RC_LAUNCH_CHECK();
    return (int)RC_OK;
  });
}
