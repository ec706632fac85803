// lgcn.hip -- LightGCN's graph propagation over the normalised user-item adjacency  (reference: models/general/LightGCN.py:137-154)
//
//   forward   out = mean(E_0, A E_0, ..., A^L E_0)                      E_0 = (user table | item table), A symmetric
//   backward  dE_0 = sum_{l=0..L} A^l G / (L+1) = g + A (g + A (g + ...)),  g = G / (L+1)   (Horner form: L products)
//
// Every product is an SpMM over a static CSR (int64 row offsets, int32 column ids, fp32 values) driven by a plan built once on
// the host (rechorus_amd/lgcn.py): a list of work items (destination row, edge range, partial slot), longest first.  Rows longer
// than the plan's chunk length are split into chunks whose partial sums are stored, then added per row in chunk order by a
// second pass (the skew rule of a per-destination gather: one wave per hub row would run as long as the hub).  No atomics:
// every sum has a fixed order, so results are bitwise reproducible run to run.
//
// One wave per work item.  A row of d floats is covered by LPR lanes holding one float4 each (LPR = the power of two >= d/4),
// so a wave works on G = 64 / LPR neighbours at once, U of them per lane group in flight; lane group k sums edges k, k + G, ...
// in order, and the groups are combined by a fixed butterfly.  The epilogue of a layer folds the running mean:
//   out[r] = (add[r] / add_div + y[r]) / out_div,   optionally y[r] stored for the next layer.
#include "common.hpp"

namespace rc {

struct LgcnRows {              // a node table split at n_u: rows < n_u in u, the others in i (E_0 straight from the two parameters)
  const float* u;
  const float* i;
};
struct LgcnOut {
  float* u;
  float* i;
};

__device__ __forceinline__ int64_t lgcn_off(int64_t r, int64_t n_u, int d, bool& in_u) {
  in_u = r < n_u;
  return (in_u ? r : r - n_u) * (int64_t)d;
}

struct LgcnEpi {
  LgcnRows add;    // add.u == nullptr: nothing to add
  float add_div;
  float out_div;
  float* ystore;   // [N, d] or nullptr
  LgcnOut out;
};

__device__ __forceinline__ float4 lgcn_div4(float4 a, float s) { return make_float4(a.x / s, a.y / s, a.z / s, a.w / s); }

__device__ __forceinline__ void lgcn_epilogue(const LgcnEpi& ep, int64_t row, int64_t n_u, int d, int l, float4 y) {
  bool in_u;
  const int64_t o = lgcn_off(row, n_u, d, in_u) + 4 * l;
  float4 r = y;
  if (ep.add.u != nullptr) {
    const float4 a = lgcn_div4(*reinterpret_cast<const float4*>((in_u ? ep.add.u : ep.add.i) + o), ep.add_div);
    r = make_float4(a.x + y.x, a.y + y.y, a.z + y.z, a.w + y.w);
  }
  r = lgcn_div4(r, ep.out_div);
  if (ep.ystore != nullptr) *reinterpret_cast<float4*>(ep.ystore + row * d + 4 * l) = y;
  *reinterpret_cast<float4*>((in_u ? ep.out.u : ep.out.i) + o) = r;
}

template <int LPR, int U>
__global__ __launch_bounds__(kBlock) void lgcn_spmm_kernel(const int32_t* __restrict__ indices, const float* __restrict__ values,
                                                           const int32_t* __restrict__ w_row, const int64_t* __restrict__ w_beg,
                                                           const int32_t* __restrict__ w_len, const int32_t* __restrict__ w_part,
                                                           int64_t n_work, int64_t n_u, int d, LgcnRows x, LgcnEpi ep,
                                                           float* __restrict__ partials) {
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPR;
  const int l = lane % LPR;
  const bool on = 4 * l < d;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); w < n_work; w += nw) {   // (wave-uniform)
    const int64_t row = w_row[w];
    const int64_t beg = w_beg[w];
    const int len = w_len[w];
    const int part = w_part[w];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = grp; k0 < len; k0 += G * U) {
      int c[U];
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * G;
        c[u] = k < len ? indices[beg + k] : 0;
        v[u] = k < len ? values[beg + k] : 0.f;
      }
      float4 r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        r[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on && k0 + u * G < len) {
          bool in_u;
          const int64_t o = lgcn_off(c[u], n_u, d, in_u) + 4 * l;
          r[u] = *reinterpret_cast<const float4*>((in_u ? x.u : x.i) + o);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k0 + u * G < len) {
          acc.x = fmaf(v[u], r[u].x, acc.x);
          acc.y = fmaf(v[u], r[u].y, acc.y);
          acc.z = fmaf(v[u], r[u].z, acc.z);
          acc.w = fmaf(v[u], r[u].w, acc.w);
        }
      }
    }
    if (G > 1) {
      acc.x = groups_allreduce_sum<LPR, 64>(acc.x);
      acc.y = groups_allreduce_sum<LPR, 64>(acc.y);
      acc.z = groups_allreduce_sum<LPR, 64>(acc.z);
      acc.w = groups_allreduce_sum<LPR, 64>(acc.w);
    }
    if (grp == 0 && on) {
      if (part >= 0)
        *reinterpret_cast<float4*>(partials + (int64_t)part * d + 4 * l) = acc;
      else
        lgcn_epilogue(ep, row, n_u, d, l, acc);
    }
  }
}

// the rows split into chunks: partial sums added in chunk order, then the layer's epilogue.  One wave per row, lane l holds float4 l.
__global__ __launch_bounds__(kBlock) void lgcn_combine_kernel(const int32_t* __restrict__ long_row, const int32_t* __restrict__ long_ptr,
                                                              int64_t n_long, int64_t n_u, int d, const float* __restrict__ partials,
                                                              LgcnEpi ep) {
  const int l = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); w < n_long; w += nw) {
    if (4 * l >= d) continue;
    const int p0 = long_ptr[w], p1 = long_ptr[w + 1];
    float4 y = *reinterpret_cast<const float4*>(partials + (int64_t)p0 * d + 4 * l);
    for (int p = p0 + 1; p < p1; ++p) {
      const float4 q = *reinterpret_cast<const float4*>(partials + (int64_t)p * d + 4 * l);
      y = make_float4(y.x + q.x, y.y + q.y, y.z + q.z, y.w + q.w);
    }
    lgcn_epilogue(ep, long_row[w], n_u, d, l, y);
  }
}

// out[r] = src[r] / div over all N rows (E_0 when L = 0; g = G / (L+1) in front of the backward products)
__global__ __launch_bounds__(kBlock) void lgcn_rows_div_kernel(LgcnRows src, LgcnOut out, int64_t n_u, int64_t n_nodes, int d, float div) {
  const int dq = d / 4;
  const int64_t total = n_nodes * dq;
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
    const int64_t r = t / dq;
    const int q = (int)(t - r * dq);
    bool in_u;
    const int64_t o = lgcn_off(r, n_u, d, in_u) + 4 * q;
    const float4 a = *reinterpret_cast<const float4*>((in_u ? src.u : src.i) + o);
    *reinterpret_cast<float4*>((in_u ? out.u : out.i) + o) = lgcn_div4(a, div);
  }
}

constexpr int kLgcnUnroll = 4;

static unsigned lgcn_grid(int64_t waves) {
  const int64_t blocks = (waves + kBlock / 64 - 1) / (kBlock / 64);
  return (unsigned)(blocks < 1 ? 1 : (blocks > kMaxGridX ? kMaxGridX : blocks));
}

template <int LPR>
static int lgcn_spmm_launch(const rc_lgcn_graph* g, int d, LgcnRows x, const LgcnEpi& ep, float* partials, hipStream_t st) {
  if (g->n_work > 0) {
    hipLaunchKernelGGL((lgcn_spmm_kernel<LPR, kLgcnUnroll>), dim3(lgcn_grid(g->n_work)), dim3(kBlock), 0, st, g->indices, g->values,
                       g->work_row, g->work_beg, g->work_len, g->work_part, g->n_work, g->n_users, d, x, ep, partials);
    RC_LAUNCH_CHECK();
  }
  if (g->n_long > 0) {
    hipLaunchKernelGGL(lgcn_combine_kernel, dim3(lgcn_grid(g->n_long)), dim3(kBlock), 0, st, g->long_row, g->long_part_ptr, g->n_long,
                       g->n_users, d, (const float*)partials, ep);
    RC_LAUNCH_CHECK();
  }
  return RC_OK;
}

// one product A x with the epilogue ep
static int lgcn_spmm(const rc_lgcn_graph* g, int d, LgcnRows x, const LgcnEpi& ep, float* partials, hipStream_t st) {
  const int dq = d / 4;
  if (dq <= 1) return lgcn_spmm_launch<1>(g, d, x, ep, partials, st);
  if (dq <= 2) return lgcn_spmm_launch<2>(g, d, x, ep, partials, st);
  if (dq <= 4) return lgcn_spmm_launch<4>(g, d, x, ep, partials, st);
  if (dq <= 8) return lgcn_spmm_launch<8>(g, d, x, ep, partials, st);
  if (dq <= 16) return lgcn_spmm_launch<16>(g, d, x, ep, partials, st);
  if (dq <= 32) return lgcn_spmm_launch<32>(g, d, x, ep, partials, st);
  return lgcn_spmm_launch<64>(g, d, x, ep, partials, st);
}

static int lgcn_rows_div(const rc_lgcn_graph* g, int d, LgcnRows src, LgcnOut out, float div, hipStream_t st) {
  const int64_t n = g->n_users + g->n_items;
  const int64_t total = n * (d / 4);
  if (total == 0) return RC_OK;
  int64_t blocks = (total + kBlock - 1) / kBlock;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(lgcn_rows_div_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, src, out, g->n_users, n, d, div);
  RC_LAUNCH_CHECK();
  return RC_OK;
}

// the one statement of the envelope: every entry point checks it, rc_lgcn_check_shape reports it to the host
static int lgcn_shape(const char* fn, int d, int n_layers, int64_t n_nodes, int64_t nnz) {
  const bool ok = d % 4 == 0 && d >= 4 && d <= 256 && n_layers >= 0 && n_layers <= 8 && n_nodes >= 0 &&
                  n_nodes < ((int64_t)1 << 31) && nnz >= 0 && nnz < ((int64_t)1 << 31);
  if (ok) return RC_OK;
  return fail(RC_ERR_UNSUPPORTED, "%s: outside the envelope (emb_size a multiple of 4 in [4, 256], n_layers in [0, 8], N < 2^31, "
              "nnz < 2^31): emb_size=%d n_layers=%d N=%lld nnz=%lld", fn, d, n_layers, (long long)n_nodes, (long long)nnz);
}

static bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

static int lgcn_check(const char* fn, const rc_lgcn_graph* g, int d, int n_layers, const float* a, const float* b, const float* c,
                      const float* e, float* buf_a, float* buf_b, float* partials, int need_a, int need_b) {
  RC_REQUIRE(g != nullptr, "%s: null pointer (graph)", fn);
  RC_TRY(lgcn_shape(fn, d, n_layers, g->n_users + g->n_items, g->nnz));
  RC_REQUIRE(g->n_users >= 0 && g->n_items >= 0 && g->n_work >= 0 && g->n_long >= 0 && g->n_parts >= 0, "%s: negative sizes", fn);
  RC_REQUIRE(a != nullptr && b != nullptr && c != nullptr && e != nullptr, "%s: null pointer (tables)", fn);
  RC_REQUIRE(aligned16(a) && aligned16(b) && aligned16(c) && aligned16(e), "%s: tables must be 16-byte aligned", fn);
  if (n_layers > 0) {
    RC_REQUIRE(g->indptr != nullptr && (g->nnz == 0 || (g->indices != nullptr && g->values != nullptr)), "%s: null pointer (CSR)", fn);
    RC_REQUIRE(g->n_work == 0 || (g->work_row && g->work_beg && g->work_len && g->work_part), "%s: null pointer (plan)", fn);
    RC_REQUIRE(g->n_long == 0 || (g->long_row && g->long_part_ptr), "%s: null pointer (plan long rows)", fn);
    RC_REQUIRE(g->n_parts == 0 || (partials != nullptr && aligned16(partials)), "%s: null pointer (partials)", fn);
    RC_REQUIRE(g->n_long <= g->n_parts, "%s: more long rows than partial slots", fn);
  }
  RC_REQUIRE(!need_a || (buf_a != nullptr && aligned16(buf_a)), "%s: null pointer (buf_a: needed at n_layers=%d)", fn, n_layers);
  RC_REQUIRE(!need_b || (buf_b != nullptr && aligned16(buf_b)), "%s: null pointer (buf_b: needed at n_layers=%d)", fn, n_layers);
  return RC_OK;
}

}  // namespace rc

extern "C" int rc_lgcn_check_shape(int d, int n_layers, int64_t n_nodes, int64_t nnz) {
  return rc::lgcn_shape("rc_lgcn_check_shape", d, n_layers, n_nodes, nnz);
}

extern "C" int rc_lgcn_propagate_fwd(const rc_lgcn_graph* g, const float* user_emb, const float* item_emb, int d, int n_layers,
                                     float* buf_a, float* buf_b, float* partials, float* out, rc_stream_t stream) {
  using namespace rc;
  RC_TRY(lgcn_check("rc_lgcn_propagate_fwd", g, d, n_layers, user_emb, item_emb, out, out, buf_a, buf_b, partials,
                    n_layers >= 2, n_layers >= 3));
  const hipStream_t st = as_stream(stream);
  const LgcnRows e0{user_emb, item_emb};
  const LgcnOut o{out, out + g->n_users * (int64_t)d};
  if (n_layers == 0) return lgcn_rows_div(g, d, e0, o, 1.f, st);
  const LgcnRows acc{out, out + g->n_users * (int64_t)d};
  float* bufs[2] = {buf_a, buf_b};
  LgcnRows x = e0;
  for (int k = 1; k <= n_layers; ++k) {
    const bool last = k == n_layers;
    LgcnEpi ep;
    ep.add = k == 1 ? e0 : acc;      // layer 1 writes E_0 + E_1, later layers add to the running sum in `out`
    ep.add_div = 1.f;
    ep.out_div = last ? (float)(n_layers + 1) : 1.f;
    ep.ystore = last ? nullptr : bufs[(k - 1) & 1];    // E_L itself is never stored
    ep.out = o;
    RC_TRY(lgcn_spmm(g, d, x, ep, partials, st));
    if (!last) x = LgcnRows{ep.ystore, ep.ystore + g->n_users * (int64_t)d};
  }
  return RC_OK;
}

extern "C" int rc_lgcn_propagate_bwd(const rc_lgcn_graph* g, const float* grad_user, const float* grad_item, int d, int n_layers,
                                     float* buf_a, float* buf_b, float* partials, float* grad_user_emb, float* grad_item_emb,
                                     rc_stream_t stream) {
  using namespace rc;
  RC_TRY(lgcn_check("rc_lgcn_propagate_bwd", g, d, n_layers, grad_user, grad_item, grad_user_emb, grad_item_emb, buf_a, buf_b,
                    partials, n_layers >= 1, n_layers >= 2));
  const hipStream_t st = as_stream(stream);
  const LgcnRows gin{grad_user, grad_item};
  const LgcnOut gout{grad_user_emb, grad_item_emb};
  const float div = (float)(n_layers + 1);
  if (n_layers == 0) return lgcn_rows_div(g, d, gin, gout, 1.f, st);
  const int64_t half = g->n_users * (int64_t)d;
  RC_TRY(lgcn_rows_div(g, d, gin, LgcnOut{buf_a, buf_a + half}, div, st));       // h = g = G / (L+1)
  float* bufs[2] = {buf_a, buf_b};
  LgcnRows x{buf_a, buf_a + half};
  for (int k = 1; k <= n_layers; ++k) {                                           // h = A h + g, L times
    const bool last = k == n_layers;
    float* nxt = bufs[k & 1];
    LgcnEpi ep;
    ep.add = gin;
    ep.add_div = div;
    ep.out_div = 1.f;
    ep.ystore = nullptr;
    ep.out = last ? gout : LgcnOut{nxt, nxt + half};
    RC_TRY(lgcn_spmm(g, d, x, ep, partials, st));
    x = LgcnRows{nxt, nxt + half};
  }
  return RC_OK;
}
