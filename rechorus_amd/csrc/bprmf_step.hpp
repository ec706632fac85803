// bprmf_step.hpp -- internal interface of the BPRMF training step (rc_bprmf_train_step / _ahead): the argument record of
// one step and the launch sequences that train_step.hip calls in other files.  The entry point checks the arguments,
// fills ONE BprmfStep and hands it on; a callee adds only what is its own (plan buffers, the small step's extra buffer).
#pragma once
#include "common.hpp"
#include "opt_math.hpp"
#include "plan.hpp"

namespace rc {

struct SmallPlanArgs;   // small_plan.hpp

struct BprmfStep {
  float *U, *I;                    // tables [n_users, d], [n_items, d]
  float *mU, *vU, *mI, *vI;        // optimizer state (null where the optimizer has none)
  const int64_t* uid;              // [B]
  const int64_t* iid;              // [B, C]
  int B, C, d;
  int64_t n_users, n_items;
  const rc_opt_hyper* h;           // validated by the entry point: `o` and `mode` are what fill_opt_scalars / mode_of make of it
  OptScalars o;
  int mode;
  float inv_b;
  float* loss_out;
  float* pred;                     // may be null
  float *gpred, *ugrad, *loss_vec; // carved scratch: [B, C], [B, d], [B]
  hipStream_t s;
  int64_t n_i() const { return (int64_t)B * C; }
};

// ---- small batches (small_step.hip): two launches ---------------------------------------------------
bool small_step_supported(int64_t n_i, int64_t B, int64_t n_items, int64_t n_users, int d);
size_t small_step_extra_bytes(int64_t n, int64_t B, int d);   // workspace beyond gpred / ugrad / loss_vec
// ev_mid: null, or two events recorded between the launches ([0] closes the front launch, [1] opens the update launch)
int small_step_launch(const BprmfStep& st, void* extra, hipEvent_t* ev_mid);
// first launch of the small-batch step (bprmf_fused.hip); the caller checked rc_bprmf_fused_supported(d, C)
int small_front_launch(const BprmfStep& st, float* ub, const SmallPlanArgs& plan);

// ---- bucket plan (plan_update.hip): the two update launches behind the fused kernel -----------------
// lw, med: the hot and the medium rows as the plan registered them (emit_long)
// ev_items_done: null, or an event recorded between the item-row launch and the last launch
int plan_bprmf_step_updates(const BprmfStep& st, const rc_plan_row* rows_i, const uint32_t* n_rows_i, const rc_plan_row* rows_u,
                            const uint32_t* n_rows_u, const uint32_t* occ, uint32_t* counters, const PlanLongWs& lw,
                            const PlanMedList& med, hipEvent_t* ev_items_done);

}  // namespace rc
