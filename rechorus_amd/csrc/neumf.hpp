// neumf.hpp -- what neumf.hip and neumf_step.hip share on the host side.
#pragma once
#include "common.hpp"

namespace rc {

// out[i] = sum_w p[w][i] for the three partial arrays of one backward call (n_wg workgroups' partials, fixed order) -> dW1, db1, dw_out
int neumf_reduce_partials(const float* pW1, const float* pb1, const float* pwout, float* dW1, float* db1, float* dw_out, int cW, int cb,
                          int co, int n_wg, hipStream_t s);

}  // namespace rc
