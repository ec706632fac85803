// kda.hip -- KDA's first level, RelationalDynamicAggregation (Wang et al., TOIS 2021; reference models/sequential/KDA.py:265-303).
// For every candidate c of batch row b and every relation r:
//     ri       = (rel[r] + value[b, c, r]) * target[b, c]          (without include_val: rel[r] * target[b, c])
//     a[l]     = <seq[b, l], ri>,   p = softmax of a over the valid l (hist[b, l] > 0),   maximum taken per (b, c, r)
//     x[b,l,r] = (1 / 2F) sum_{k < F} (cos(w_k) real[r, k] - sin(w_k) imag[r, k]),   w_k = (2 pi f_k) delta_t[b, l],  f_k = k / (F - 1) / 2
//                -- the reference's mean over the 2F conjugate-symmetric terms, halved: the terms k and k + F are equal
//     context[b, c, r] = sum_l p[l] clamp(x[b, l, r], 0, 1) seq[b, l]
// A row without any valid position gives a ZERO context and zero gradients here (the reference's softmax over nothing is NaN); the
// sequential readers never produce such a row.  Invalid positions may sit anywhere in the row.  sinf / cosf are the accurate ones.
//
// One workgroup owns one batch row at a time: the history rows, the validity flags and the row's decay[l, r] (computed ONCE per batch
// row by the threads l < L, never per candidate) live in LDS; a lane-group of V / 4 lanes holds one float4 of every V-wide row.
//   kda_fwd_kernel     a lane-group takes the (c, r) pairs g, g + GPB, ...; one pass over l with a running maximum (online softmax)
//   kda_bwd_kernel     a workgroup takes rows b = blockIdx, blockIdx + G, ...  Tiles of GPB candidates, relation by relation: phase 1,
//                      per lane-group, recomputes a[l] and dw[l] = <d_context, seq[l]>, the softmax and its backward, and leaves
//                      w[l] = p dec, da[l] and p[l] dw[l] plus the rows d_context, ri and dvalue in LDS; phase 2, thread-owned
//                      outputs summed over the tile's candidates in candidate order: dseq[l, :] (registers), ddecay[l, r] and
//                      drel[r, :] (LDS).  dtarget is the lane-group's own sum over r.  After the row: the decay's backward, thread k
//                      owning frequency k.  drel / dfreq_* go to the workgroup's slice of the workspace.
//   kda_reduce_kernel  sums the slices in workgroup order.
// No atomics of any kind; every sum has a fixed order: two runs are bit-equal.  Nothing of size B C L R exists.
#include "common.hpp"

namespace rc {

constexpr int kKdaMaxL = 64, kKdaMaxR = 8, kKdaMaxF = 129;
constexpr int kKdaMaxGroups = 1024;    // workgroups of the backward = slices of its workspace
constexpr float kKdaTwoPi = 6.28318530717958647692f;

struct KdaArgs {
  const float* seq;       // [B, L, V]
  const int64_t* hist;    // [B, L]
  const float* dt;        // [B, L]
  const float* target;    // [B, C, V]
  const float* value;     // [B, C, R, V] (include_val only)
  const float* rel;       // [R, V]
  const float* fre;       // [R, F]
  const float* fim;       // [R, F]
  int64_t B;
  int C, L, R, F, include_val;
  float* ctx;             // [B, C, R, V]           forward
  const float* dctx;      // [B, C, R, V]           backward
  float* dseq;            // [B, L, V]
  float* dtarget;         // [B, C, V]
  float* dvalue;          // [B, C, R, V] (include_val only)
  float* partial;         // [G, stride]: drel [R, V] | dfreq_real [R, F] | dfreq_imag [R, F]
  int stride;
};

__device__ __forceinline__ float4 kadd4(const float4& x, const float4& y) { return make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w); }
__device__ __forceinline__ float4 kmul4(const float4& x, const float4& y) { return make_float4(x.x * y.x, x.y * y.y, x.z * y.z, x.w * y.w); }
__device__ __forceinline__ float4 kfma4(float s, const float4& x, const float4& y) {
  return make_float4(fmaf(s, x.x, y.x), fmaf(s, x.y, y.y), fmaf(s, x.z, y.z), fmaf(s, x.w, y.w));
}

// f_k of np.linspace(0, 1, F) / 2 as the reference's float32 tensor holds it, times float32(2 pi) (KDA.py:272-273, :281)
__device__ __forceinline__ float kda_omega(int k, int F) {
  const float fk = (float)((double)k * (1.0 / (double)(F - 1)) * 0.5);
  return kKdaTwoPi * fk;
}

// Row b into LDS: history rows, validity, delta_t and the decay (clamped; 0 on invalid positions) with its clamp-pass mask.
// Ends with a barrier; the caller has made sure nobody still reads the previous row.
template <int V>
__device__ __forceinline__ void kda_stage_row(const KdaArgs& a, int64_t b, float4* seq_s, float* dec_s, float* pass_s, float* dt_s,
                                              int* valid_s) {
  constexpr int LPR = V / 4;
  const int tid = threadIdx.x;
  const float4* src = reinterpret_cast<const float4*>(a.seq + b * a.L * V);
  for (int i = tid; i < a.L * LPR; i += kBlock) seq_s[i] = src[i];
  if (tid < a.L) {
    const bool valid = a.hist[b * a.L + tid] > 0;
    const float t = a.dt[b * a.L + tid];
    valid_s[tid] = valid ? 1 : 0;
    dt_s[tid] = t;
    float x[kKdaMaxR];
#pragma unroll
    for (int r = 0; r < kKdaMaxR; ++r) x[r] = 0.f;
    for (int k = 0; k < a.F; ++k) {
      float sn, cs;
      sincosf(kda_omega(k, a.F) * t, &sn, &cs);
#pragma unroll
      for (int r = 0; r < kKdaMaxR; ++r)
        if (r < a.R) x[r] += cs * a.fre[r * a.F + k] - sn * a.fim[r * a.F + k];
    }
    const float inv2f = 1.0f / (float)(2 * a.F);
#pragma unroll
    for (int r = 0; r < kKdaMaxR; ++r)
      if (r < a.R) {
        const float xv = x[r] * inv2f;
        dec_s[tid * a.R + r] = valid ? fminf(fmaxf(xv, 0.f), 1.f) : 0.f;
        pass_s[tid * a.R + r] = (valid && xv >= 0.f && xv <= 1.f) ? 1.f : 0.f;   // clamp's backward passes on [0, 1], bounds included
      }
  }
  __syncthreads();
}

template <int V>
__device__ __forceinline__ float4 kda_ri(const KdaArgs& a, int64_t bc, int r, int l4, const float4& tg, float4* rv_out) {
  constexpr int LPR = V / 4;
  float4 rv = reinterpret_cast<const float4*>(a.rel)[r * LPR + l4];
  if (a.include_val) rv = kadd4(rv, reinterpret_cast<const float4*>(a.value)[(bc * a.R + r) * LPR + l4]);
  *rv_out = rv;
  return kmul4(rv, tg);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kBlock) void kda_fwd_kernel(KdaArgs a) {
  constexpr int LPR = V / 4, GPB = kBlock / LPR;
  __shared__ float4 seq_s[kKdaMaxL * LPR];
  __shared__ float dec_s[kKdaMaxL * kKdaMaxR], pass_s[kKdaMaxL * kKdaMaxR], dt_s[kKdaMaxL];
  __shared__ int valid_s[kKdaMaxL];
  const int64_t b = blockIdx.x;
  kda_stage_row<V>(a, b, seq_s, dec_s, pass_s, dt_s, valid_s);
  const int g = threadIdx.x / LPR, l4 = threadIdx.x % LPR;
  const int P = a.C * a.R;
  for (int j = g; j < P; j += GPB) {   // uniform over the lane-group; no workgroup barrier below
    const int c = j / a.R, r = j % a.R;
    const int64_t bc = b * a.C + c;
    const float4 tg = reinterpret_cast<const float4*>(a.target)[bc * LPR + l4];
    float4 rv;
    const float4 ri = kda_ri<V>(a, bc, r, l4, tg, &rv);
    float m = -INFINITY, s = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l = 0; l < a.L; ++l) {
      if (!valid_s[l]) continue;       // uniform over the workgroup
      const float4 sv = seq_s[l * LPR + l4];
      const float av = row_allreduce_sum<LPR>(dot4(sv, ri));
      const float mn = fmaxf(m, av);
      const float sc = expf(m - mn), e = expf(av - mn);   // the first valid position: exp(-inf) = 0 on s = 0, acc = 0
      const float ed = e * dec_s[l * a.R + r];
      s = s * sc + e;
      acc = make_float4(fmaf(ed, sv.x, acc.x * sc), fmaf(ed, sv.y, acc.y * sc), fmaf(ed, sv.z, acc.z * sc), fmaf(ed, sv.w, acc.w * sc));
      m = mn;
    }
    const float inv = s > 0.f ? 1.0f / s : 0.f;          // no valid position: a zero context
    reinterpret_cast<float4*>(a.ctx)[(bc * a.R + r) * LPR + l4] = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kBlock) void kda_bwd_kernel(KdaArgs a, int G) {
  constexpr int LPR = V / 4;
  constexpr int GPB = (kBlock / LPR) < 32 ? (kBlock / LPR) : 32;   // candidates of a tile (V = 16: the upper half of the workgroup sits out phase 1)
  constexpr int Q = (kKdaMaxL * LPR + kBlock - 1) / kBlock;        // dseq float4s a thread owns
  __shared__ float4 seq_s[kKdaMaxL * LPR];
  __shared__ float4 g_s[GPB * LPR], ri_s[GPB * LPR], dv_s[GPB * LPR];
  __shared__ float4 drel_s[kKdaMaxR * LPR];
  __shared__ float x0_s[GPB * kKdaMaxL], x1_s[GPB * kKdaMaxL], x2_s[GPB * kKdaMaxL];
  __shared__ float dec_s[kKdaMaxL * kKdaMaxR], pass_s[kKdaMaxL * kKdaMaxR], ddec_s[kKdaMaxL * kKdaMaxR], dt_s[kKdaMaxL];
  __shared__ int valid_s[kKdaMaxL];
  const int tid = threadIdx.x;
  const int g = tid / LPR, l4 = tid % LPR;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float fr[kKdaMaxR], fi[kKdaMaxR];
#pragma unroll
  for (int r = 0; r < kKdaMaxR; ++r) fr[r] = fi[r] = 0.f;
  for (int i = tid; i < kKdaMaxR * LPR; i += kBlock) drel_s[i] = zero4;

  for (int64_t b = blockIdx.x; b < a.B; b += G) {
    __syncthreads();                                     // the previous row's decay backward has read ddec_s / pass_s / dt_s
    for (int i = tid; i < a.L * a.R; i += kBlock) ddec_s[i] = 0.f;
    kda_stage_row<V>(a, b, seq_s, dec_s, pass_s, dt_s, valid_s);
    float4 dacc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) dacc[q] = zero4;

    for (int c0 = 0; c0 < a.C; c0 += GPB) {
      const int jn = (a.C - c0) < GPB ? (a.C - c0) : GPB;
      const bool active = g < jn;                        // uniform over the lane-group
      const int64_t bc = b * a.C + c0 + (active ? g : 0);
      float4 tg = zero4, dtg = zero4;
      if (active) tg = reinterpret_cast<const float4*>(a.target)[bc * LPR + l4];
      for (int r = 0; r < a.R; ++r) {
        if (active) {
          // phase 1: this lane-group's (c, r).  Every lane of the group writes the SAME reduced value to the group's slot and reads
          // back what it wrote itself.
          float* x0 = x0_s + g * kKdaMaxL;
          float* x1 = x1_s + g * kKdaMaxL;
          float* x2 = x2_s + g * kKdaMaxL;
          float4 rv;
          const float4 ri = kda_ri<V>(a, bc, r, l4, tg, &rv);
          const float4 g4 = reinterpret_cast<const float4*>(a.dctx)[(bc * a.R + r) * LPR + l4];
          float m = -INFINITY;
          for (int l = 0; l < a.L; ++l) {
            if (!valid_s[l]) continue;
            const float4 sv = seq_s[l * LPR + l4];
            const float av = row_allreduce_sum<LPR>(dot4(sv, ri));
            const float dw = row_allreduce_sum<LPR>(dot4(sv, g4));
            x0[l] = av;
            x1[l] = dw;
            m = fmaxf(m, av);
          }
          float s = 0.f, T = 0.f;
          for (int l = 0; l < a.L; ++l) {
            if (!valid_s[l]) continue;
            const float e = expf(x0[l] - m);
            s += e;
            T = fmaf(e * x1[l], dec_s[l * a.R + r], T);
            x0[l] = e;
          }
          const float inv = s > 0.f ? 1.0f / s : 0.f;
          const float S = T * inv;                       // sum_l p[l] dw[l] dec[l]
          float4 dri = zero4;
          for (int l = 0; l < a.L; ++l) {
            float w = 0.f, da = 0.f, pdw = 0.f;
            if (valid_s[l]) {
              const float p = x0[l] * inv, dw = x1[l], d = dec_s[l * a.R + r];
              w = p * d;
              da = p * (dw * d - S);
              pdw = p * dw;
              dri = kfma4(da, seq_s[l * LPR + l4], dri);
            }
            x0[l] = w;
            x1[l] = da;
            x2[l] = pdw;
          }
          const float4 dv = kmul4(dri, tg);              // d(rel[r] + value[b, c, r])
          if (a.include_val) reinterpret_cast<float4*>(a.dvalue)[(bc * a.R + r) * LPR + l4] = dv;
          dtg = make_float4(fmaf(dri.x, rv.x, dtg.x), fmaf(dri.y, rv.y, dtg.y), fmaf(dri.z, rv.z, dtg.z), fmaf(dri.w, rv.w, dtg.w));
          g_s[g * LPR + l4] = g4;
          ri_s[g * LPR + l4] = ri;
          dv_s[g * LPR + l4] = dv;
        }
        __syncthreads();
        // phase 2: thread-owned outputs, the tile's candidates in order
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const int i = tid + q * kBlock;
          if (i < a.L * LPR) {
            const int l = i / LPR, v = i % LPR;
            float4 acc = dacc[q];
            for (int j = 0; j < jn; ++j) {
              acc = kfma4(x0_s[j * kKdaMaxL + l], g_s[j * LPR + v], acc);
              acc = kfma4(x1_s[j * kKdaMaxL + l], ri_s[j * LPR + v], acc);
            }
            dacc[q] = acc;
          }
        }
        if (tid < a.L) {
          float sum = ddec_s[tid * a.R + r];
          for (int j = 0; j < jn; ++j) sum += x2_s[j * kKdaMaxL + tid];
          ddec_s[tid * a.R + r] = sum;
        }
        if (tid < LPR) {
          float4 sum = drel_s[r * LPR + tid];
          for (int j = 0; j < jn; ++j) sum = kadd4(sum, dv_s[j * LPR + tid]);
          drel_s[r * LPR + tid] = sum;
        }
        __syncthreads();
      }
      if (active) reinterpret_cast<float4*>(a.dtarget)[bc * LPR + l4] = dtg;
    }

    float4* dst = reinterpret_cast<float4*>(a.dseq + b * a.L * V);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = tid + q * kBlock;
      if (i < a.L * LPR) dst[i] = dacc[q];
    }
    // the decay's backward: thread k owns frequency k of every relation (ddec_s is complete: the tile loop ended on a barrier)
    if (tid < a.F) {
      const float om = kda_omega(tid, a.F);
      for (int l = 0; l < a.L; ++l) {
        if (!valid_s[l]) continue;
        float sn, cs;
        sincosf(om * dt_s[l], &sn, &cs);
#pragma unroll
        for (int r = 0; r < kKdaMaxR; ++r)
          if (r < a.R) {
            const float dx = ddec_s[l * a.R + r] * pass_s[l * a.R + r];
            fr[r] = fmaf(dx, cs, fr[r]);
            fi[r] = fmaf(-dx, sn, fi[r]);
          }
      }
    }
  }

  __syncthreads();
  float* part = a.partial + (int64_t)blockIdx.x * a.stride;
  for (int i = tid; i < a.R * LPR; i += kBlock) reinterpret_cast<float4*>(part)[i] = drel_s[i];
  if (tid < a.F) {
    const float inv2f = 1.0f / (float)(2 * a.F);
#pragma unroll
    for (int r = 0; r < kKdaMaxR; ++r)
      if (r < a.R) {
        part[a.R * V + r * a.F + tid] = fr[r] * inv2f;
        part[a.R * V + (a.R + r) * a.F + tid] = fi[r] * inv2f;
      }
  }
}

// element i of [drel | dfreq_real | dfreq_imag]: the G slices in workgroup order, four loads in flight
__global__ __launch_bounds__(kBlock) void kda_reduce_kernel(const float* partial, int stride, int G, int n_rel, int n_freq, float* drel,
                                                            float* dfre, float* dfim) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_rel + 2 * n_freq) return;
  float acc = 0.f;
  for (int g0 = 0; g0 < G; g0 += 4) {
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = partial[(int64_t)(g0 + q < G ? g0 + q : g0) * stride + i];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (g0 + q < G) acc += v[q];
  }
  if (i < n_rel) drel[i] = acc;
  else if (i < n_rel + n_freq) dfre[i - n_rel] = acc;
  else dfim[i - n_rel - n_freq] = acc;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static int kda_shape_check(const char* who, int V, int L, int R, int F) {
  RC_REQUIRE(V == 16 || V == 32 || V == 64 || V == 128, "%s: emb_size V=%d has no kernel (16, 32, 64, 128)", who, V);
  RC_REQUIRE(L >= 1 && L <= kKdaMaxL, "%s: history length L=%d outside [1, %d]", who, L, kKdaMaxL);
  RC_REQUIRE(R >= 1 && R <= kKdaMaxR, "%s: R=%d relations outside [1, %d]", who, R, kKdaMaxR);
  RC_REQUIRE(F >= 2 && F <= kKdaMaxF, "%s: F=%d frequencies outside [2, %d]", who, F, kKdaMaxF);
  return RC_OK;
}

static int kda_bwd_groups(int64_t B) { return (int)(B < 1 ? 1 : (B < kKdaMaxGroups ? B : kKdaMaxGroups)); }
static int kda_stride(int R, int V, int F) { return (R * V + 2 * R * F + 3) / 4 * 4; }

static size_t kda_bwd_ws_bytes(int64_t B, int R, int V, int F) {
  if (kda_shape_check("rc_kda_aggregate_bwd_workspace_bytes", V, 1, R, F) != RC_OK) return 0;
  return align_up((size_t)kda_bwd_groups(B) * kda_stride(R, V, F) * sizeof(float), 256);
}

static int kda_fill_args(const char* who, KdaArgs* a, const float* seq, const int64_t* hist, const float* dt, const float* target,
                         const float* value, const float* rel, const float* fre, const float* fim, int64_t B, int C, int L, int R, int V,
                         int F, int include_val) {
  RC_TRY(kda_shape_check(who, V, L, R, F));
  RC_REQUIRE(B >= 1 && C >= 1, "%s: need B >= 1 and C >= 1, got B=%lld C=%d", who, (long long)B, C);
  RC_REQUIRE(B <= kMaxGridX && (int64_t)C * R < ((int64_t)1 << 31), "%s: B=%lld or C * R = %lld too large", who, (long long)B,
             (long long)C * R);
  RC_REQUIRE(seq && hist && dt && target && rel && fre && fim && (value || !include_val), "%s: null pointer", who);
  RC_REQUIRE(aligned16(seq, target, value, rel), "%s: seq, target, value and rel must be 16-byte aligned", who);
  memset(a, 0, sizeof(*a));
  a->seq = seq; a->hist = hist; a->dt = dt; a->target = target; a->value = include_val ? value : nullptr; a->rel = rel;
  a->fre = fre; a->fim = fim; a->B = B; a->C = C; a->L = L; a->R = R; a->F = F; a->include_val = include_val ? 1 : 0;
  return RC_OK;
}

static int kda_fwd_impl(const float* seq, const int64_t* hist, const float* dt, const float* target, const float* value,
                        const float* rel, const float* fre, const float* fim, int64_t B, int C, int L, int R, int V, int F,
                        int include_val, float* context, rc_stream_t stream) {
  static const char* who = "rc_kda_aggregate_fwd";
  if (B == 0) return RC_OK;
  KdaArgs a;
  RC_TRY(kda_fill_args(who, &a, seq, hist, dt, target, value, rel, fre, fim, B, C, L, R, V, F, include_val));
  RC_REQUIRE(context != nullptr && aligned16(context), "%s: context must be a 16-byte aligned buffer", who);
  a.ctx = context;
  hipStream_t s = as_stream(stream);
  return dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", V, [&](auto VV) -> int {
    hipLaunchKernelGGL((kda_fwd_kernel<VV()>), dim3((unsigned)B), dim3(kBlock), 0, s, a);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

static int kda_bwd_impl(const float* seq, const int64_t* hist, const float* dt, const float* target, const float* value,
                        const float* rel, const float* fre, const float* fim, const float* d_context, int64_t B, int C, int L, int R,
                        int V, int F, int include_val, float* dseq, float* dtarget, float* dvalue, float* drel, float* dfre,
                        float* dfim, void* ws, size_t ws_bytes, rc_stream_t stream) {
  static const char* who = "rc_kda_aggregate_bwd";
  if (B == 0) return RC_OK;
  KdaArgs a;
  RC_TRY(kda_fill_args(who, &a, seq, hist, dt, target, value, rel, fre, fim, B, C, L, R, V, F, include_val));
  RC_REQUIRE(d_context && dseq && dtarget && drel && dfre && dfim && ws && (dvalue || !include_val), "%s: null pointer", who);
  RC_REQUIRE(aligned16(d_context, dseq, dtarget, dvalue, ws), "%s: d_context, dseq, dtarget, dvalue and the workspace must be 16-byte aligned",
             who);
  const size_t need = kda_bwd_ws_bytes(B, R, V, F);
  if (ws_bytes < need) return fail(RC_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, need);
  const int G = kda_bwd_groups(B);
  a.dctx = d_context; a.dseq = dseq; a.dtarget = dtarget; a.dvalue = include_val ? dvalue : nullptr;
  a.partial = reinterpret_cast<float*>(ws);
  a.stride = kda_stride(R, V, F);
  hipStream_t s = as_stream(stream);
  return dispatch_or_fail<16, 32, 64, 128>(who, "emb_size", V, [&](auto VV) -> int {
    hipLaunchKernelGGL((kda_bwd_kernel<VV()>), dim3(G), dim3(kBlock), 0, s, a, G);
    RC_LAUNCH_CHECK();
    const int n = R * V + 2 * R * F;
    hipLaunchKernelGGL(kda_reduce_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, a.partial, a.stride, G, R * V, R * F, drel,
                       dfre, dfim);
    RC_LAUNCH_CHECK();
    return RC_OK;
  });
}

}  // namespace rc

using namespace rc;

extern "C" enum rc_status rc_kda_check_shape(int V, int L, int R, int F) {
  return (enum rc_status)kda_shape_check("rc_kda_check_shape", V, L, R, F);
}

extern "C" enum rc_status rc_kda_aggregate_fwd(const float* seq, const int64_t* hist, const float* delta_t, const float* target,
                                               const float* value, const float* rel, const float* freq_real, const float* freq_imag,
                                               int64_t B, int C, int L, int R, int V, int F, int include_val, float* context,
                                               rc_stream_t stream) {
  return (enum rc_status)kda_fwd_impl(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, B, C, L, R, V, F, include_val, context,
                                      stream);
}

extern "C" size_t rc_kda_aggregate_bwd_workspace_bytes(int64_t B, int R, int V, int F) { return kda_bwd_ws_bytes(B, R, V, F); }

extern "C" enum rc_status rc_kda_aggregate_bwd(const float* seq, const int64_t* hist, const float* delta_t, const float* target,
                                               const float* value, const float* rel, const float* freq_real, const float* freq_imag,
                                               const float* d_context, int64_t B, int C, int L, int R, int V, int F, int include_val,
                                               float* dseq, float* dtarget, float* dvalue, float* drel, float* dfreq_real,
                                               float* dfreq_imag, void* ws, size_t ws_bytes, rc_stream_t stream) {
  return (enum rc_status)kda_bwd_impl(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, d_context, B, C, L, R, V, F, include_val,
                                      dseq, dtarget, dvalue, drel, dfreq_real, dfreq_imag, ws, ws_bytes, stream);
}
