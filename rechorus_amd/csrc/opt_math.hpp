// opt_math.hpp -- element-wise optimizer arithmetic shared by every kernel that updates a
// table row (segmented update, dense update, the fused BPRMF singleton path).
// Formulas: torch/optim/{sgd,adam,adagrad}.py single-tensor paths, which the reference
// reaches through helpers/BaseRunner.py:110-114 (construction) and :206 (step).
#pragma once
#include "common.hpp"

namespace rc {

enum { MODE_SGD = 0, MODE_ADAM = 1, MODE_ADAGRAD = 2, MODE_DENSE_GRAD = 3, MODE_NONE = 4, MODE_ADADELTA = 5 };

// which optimizer state tensors a mode reads and writes (m: exp_avg / state_sum / square_avg, v: exp_avg_sq / acc_delta)
constexpr bool mode_has_m(int mode) { return mode == MODE_ADAM || mode == MODE_ADAGRAD || mode == MODE_ADADELTA; }
constexpr bool mode_has_v(int mode) { return mode == MODE_ADAM || mode == MODE_ADADELTA; }

// python-double hyper-parameters narrowed to fp32 at the points where torch narrows them
struct OptScalars {
  float neg_lr;    // SGD/Adagrad: -lr
  float l2;        // weight_decay
  float one_m_b1;  // Adam: 1 - beta1
  float b2;        // Adam: beta2
  float one_m_b2;  // Adam: 1 - beta2
  float neg_step;  // Adam: -(lr / (1 - beta1^t))
  float bc2_sqrt;  // Adam: sqrt(1 - beta2^t)
  float eps;
};

// who: the entry point, for the refusals' text
inline int fill_opt_scalars(const char* who, const rc_opt_hyper* h, OptScalars* a, bool dense = false) {
  RC_REQUIRE(h != nullptr, "%s: optimizer hyper-parameters missing", who);
  RC_REQUIRE(h->opt == RC_OPT_SGD || h->opt == RC_OPT_ADAM || h->opt == RC_OPT_ADAGRAD || (dense && h->opt == RC_OPT_ADADELTA),
             h->opt == RC_OPT_ADADELTA ? "%s: Adadelta (optimizer %d) is built for dense steps only (rc_dense_update*)"
                                       : "%s: unknown optimizer %d", who, h->opt);
  a->l2 = (float)h->l2;
  a->neg_lr = (float)(-h->lr);
  a->eps = (float)h->eps;
  a->one_m_b1 = a->b2 = a->one_m_b2 = a->neg_step = 0.f;
  a->bc2_sqrt = 1.f;
  if (h->opt == RC_OPT_ADADELTA) {  // torch/optim/adadelta.py: rho in beta1
    a->b2 = (float)h->beta1;
    a->one_m_b2 = (float)(1.0 - h->beta1);
  }
  if (h->opt == RC_OPT_ADAM) {
    RC_REQUIRE(h->step >= 1, "%s: Adam needs step >= 1 (got %lld)", who, (long long)h->step);
    const double bc1 = 1.0 - pow(h->beta1, (double)h->step);
    const double bc2 = 1.0 - pow(h->beta2, (double)h->step);
    a->one_m_b1 = (float)(1.0 - h->beta1);
    a->b2 = (float)h->beta2;
    a->one_m_b2 = (float)(1.0 - h->beta2);
    a->neg_step = (float)(-(h->lr / bc1));
    a->bc2_sqrt = (float)sqrt(bc2);
  }
  return RC_OK;
}

inline int mode_of(const rc_opt_hyper* h) {
  return h->opt == RC_OPT_SGD ? MODE_SGD : (h->opt == RC_OPT_ADAM ? MODE_ADAM : (h->opt == RC_OPT_ADADELTA ? MODE_ADADELTA : MODE_ADAGRAD));
}

// the state tensors a row-update entry point needs for its optimizer (have_m / have_v: every table of the call has them)
inline int opt_state_check(const char* who, int mode, bool have_m, bool have_v) {
  RC_REQUIRE(mode != MODE_ADAM || (have_m && have_v), "%s: Adam needs m and v (exp_avg, exp_avg_sq)", who);
  RC_REQUIRE(mode != MODE_ADAGRAD || have_m, "%s: Adagrad needs m (state_sum)", who);
  return RC_OK;
}

#if defined(__HIPCC__)
template <int MODE>
__device__ __forceinline__ void opt_elem(const OptScalars& a, float g, float& w, float& m,
                                         float& v) {
  if (MODE == MODE_SGD) {
    g = fmaf(a.l2, w, g);  // grad.add(param, alpha=weight_decay)
    w = fmaf(a.neg_lr, g, w);
  } else if (MODE == MODE_ADAM) {
    g = fmaf(a.l2, w, g);
    m = fmaf(a.one_m_b1, g - m, m);         // exp_avg.lerp_(grad, 1-beta1)
    v = fmaf(a.one_m_b2, g * g, v * a.b2);  // mul_(beta2).addcmul_(g, g, 1-beta2)
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    w = fmaf(a.neg_step, m / denom, w);     // addcdiv_(exp_avg, denom, -step_size)
  } else if (MODE == MODE_ADAGRAD) {
    g = fmaf(a.l2, w, g);
    m = fmaf(g, g, m);                      // state_sum.addcmul_(g, g, 1)
    w = fmaf(a.neg_lr, g / (sqrtf(m) + a.eps), w);
  } else if (MODE == MODE_ADADELTA) {       // torch/optim/adadelta.py, single-tensor path
    g = fmaf(a.l2, w, g);
    m = fmaf(a.one_m_b2, g * g, m * a.b2);  // square_avg.mul_(rho).addcmul_(g, g, 1 - rho)
    const float std = sqrtf(m + a.eps);     // square_avg.add(eps).sqrt_()
    const float delta = sqrtf(v + a.eps) / std * g;   // acc_delta.add(eps).sqrt_().div_(std).mul_(g)
    v = fmaf(a.one_m_b2, delta * delta, v * a.b2);    // acc_delta.mul_(rho).addcmul_(delta, delta, 1 - rho)
    w = fmaf(a.neg_lr, delta, w);           // param.add_(delta, alpha=-lr)
  } else if (MODE == MODE_DENSE_GRAD) {     // no optimizer: the "table" is a gradient buffer, its row := the summed gradient
    w = g;
  }
}

// row write-back: the row is not read again in this step -> non-temporal store
__device__ __forceinline__ void store_row4(float4* p, const float4& x) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  v4f v = {x.x, x.y, x.z, x.w};
  __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(p));
}

// Stateless SGD often returns the bits it was given: at a large batch lr * g is far below half an ulp of the weight, and
// w = fmaf(-lr, g, w) rounds back to w in every element of the row.  Storing such a row moves bytes
// the result does not need, so the SGD write-back of a row that an aligned group of LPR lanes holds (a float4 each) stores
// it only if some lane's slice changed.  The comparison is on the bit patterns (-0.0 vs 0.0, NaN payloads and denormals
// count as they are), and the store is the whole row or nothing: a partly written line costs more per byte than a row.
// The vote is a wave ballot restricted to the group's own lanes, so it may stand in a divergent branch that whole
// lane-groups take together: lanes outside the branch contribute no bits, lanes of other groups are masked off.
// (1-D workgroups of whole waves, like every kernel of this library.)
template <int LPR>
__device__ __forceinline__ bool row_group_any(bool pred) {
  static_assert(LPR >= 1 && LPR <= 64 && 64 % LPR == 0, "a row's lane-group must be an aligned part of a wave");
  const uint64_t b = (uint64_t)__ballot(pred);
  if (LPR == 64) return b != 0ull;
  const unsigned first = (threadIdx.x & 63u) & ~(unsigned)(LPR - 1);   // the group's first lane
  const uint32_t half = (first & 32u) ? (uint32_t)(b >> 32) : (uint32_t)b;
  if (LPR == 32) return half != 0u;
  return ((half >> (first & 31u)) & ((1u << (LPR & 31)) - 1u)) != 0u;
}

__device__ __forceinline__ bool bits_differ4(const float4& a, const float4& b) {
  return (__float_as_uint(a.x) != __float_as_uint(b.x)) | (__float_as_uint(a.y) != __float_as_uint(b.y)) |
         (__float_as_uint(a.z) != __float_as_uint(b.z)) | (__float_as_uint(a.w) != __float_as_uint(b.w));
}

// write-back of a row's new W slice (w0: the slice as it was read).  SGD: only if the row changed; every other mode stores
// unconditionally (their state rows change with every step, and MODE_DENSE_GRAD's old row is not the row's history)
template <int MODE, int LPR>
__device__ __forceinline__ void store_row4_changed(float4* p, const float4& w, const float4& w0) {
  if (MODE == MODE_SGD) {
    if (row_group_any<LPR>(bits_differ4(w, w0))) store_row4(p, w);
  } else {
    store_row4(p, w);
  }
}

// the optimizer on one float4 slice held in registers (state already loaded)
template <int MODE>
__device__ __forceinline__ void opt_apply4(const OptScalars& a, float4& w, float4& m, float4& v, const float4& g) {
  opt_elem<MODE>(a, g.x, w.x, m.x, v.x);
  opt_elem<MODE>(a, g.y, w.y, m.y, v.y);
  opt_elem<MODE>(a, g.z, w.z, m.z, v.z);
  opt_elem<MODE>(a, g.w, w.w, m.w, v.w);
}

// update one float4 slice of a table row in place (row index `row`, slice l of LPR)
template <int MODE>
__device__ __forceinline__ void opt_row4(const OptScalars& a, float* __restrict__ W,
                                         float* __restrict__ M, float* __restrict__ V, size_t idx4,
                                         float4 w, const float4& g) {
  float4 m = make_float4(0, 0, 0, 0), v = make_float4(0, 0, 0, 0);
  if (mode_has_m(MODE)) m = load_stream4(reinterpret_cast<const float4*>(M) + idx4);
  if (mode_has_v(MODE)) v = load_stream4(reinterpret_cast<const float4*>(V) + idx4);
  opt_apply4<MODE>(a, w, m, v, g);
  store_row4(reinterpret_cast<float4*>(W) + idx4, w);
  if (mode_has_m(MODE)) store_row4(reinterpret_cast<float4*>(M) + idx4, m);
  if (mode_has_v(MODE)) store_row4(reinterpret_cast<float4*>(V) + idx4, v);
}

// opt_row4 where the whole row is held by an aligned group of LPR lanes that run this call together (slice idx4 of each
// lane belongs to the same row; pair mode: to the same row of two tables): SGD leaves an unchanged row unwritten
template <int MODE, int LPR>
__device__ __forceinline__ void opt_row4_group(const OptScalars& a, float* __restrict__ W, float* __restrict__ M,
                                               float* __restrict__ V, size_t idx4, float4 w, const float4& g) {
  if (MODE == MODE_SGD) {
    const float4 w0 = w;
    float4 m = make_float4(0, 0, 0, 0), v = make_float4(0, 0, 0, 0);
    opt_apply4<MODE>(a, w, m, v, g);
    store_row4_changed<MODE, LPR>(reinterpret_cast<float4*>(W) + idx4, w, w0);
  } else {
    opt_row4<MODE>(a, W, M, V, idx4, w, g);
  }
}
#endif

}  // namespace rc
