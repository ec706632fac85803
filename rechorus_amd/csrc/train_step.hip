// train_step.hip -- one BaseRunner.fit iteration for BPRMF as a single C-ABI call
// (reference: helpers/BaseRunner.py:193-206 around models/general/BPRMF.py:34-45 and
// models/BaseModel.py:182-185).  All phases are enqueued on the caller's stream with no
// host synchronisation (grid sizes depend only on B, C), so the call can be captured in a
// hipGraph; with `phase_ms` it brackets the phases with hipEvents and synchronises.
//
// Three pipelines (rc_bprmf_step_pipeline):
//   small batches (<= 32,768 row ids)   two launches: small_step.hip
//   bucket plan (default otherwise)     partition -> [flags] -> fused kernel || per-bucket pass on a second stream
//                                       -> row updates; with rc_bprmf_train_step_ahead the whole plan of the NEXT batch
//                                       runs beside this step on the second stream
//   sort pipeline (wide id spaces)      joint radix sort -> segment heads -> fused kernel -> segmented updates
// phase_ms slots (all pipelines): [0] sort / partition (+ flags) [7] segment heads / per-bucket pass when on the caller's
// stream [2] fused kernel [3] loss mean (0 when folded into the last update launch) [4] item-row update [5] user-row update.
//
// Structure: train_step_impl checks (every refusal that needs only the arguments comes before the workspace-size check,
// and that before anything is enqueued), fills ONE BprmfStep (bprmf_step.hpp), chooses (choose_pipeline) and runs
// step_small / step_plan / step_sort.  PhaseMarks owns the profiling events, ticket_take / ticket_issue the look-ahead.
//
// Ordering constraints: the item-row update reads U (pre-step values, to rebuild g*U[u]) so it runs
// before the user rows are rewritten; the fused kernel reads both tables before either is updated.
#include <mutex>

#include "bprmf_step.hpp"

// The second stream of the step.  The bucket plan's per-bucket pass (row records + grouped positions) is index work
// that only the updates need; the fused kernel needs at most the multi-occurrence bitmap.  So the step forks: the fused
// kernel runs on the caller's stream while plan_launch_back runs on this side stream, and the updates wait for both.
// One record per device, created on first use (non-blocking stream: the caller's stream may be the legacy null
// stream); fork / join are event dependencies, so the call stays capturable in a hipGraph.  rc_bprmf_step_pipeline(2)
// keeps everything on one stream.  These are resources (a stream, four events), not batch state: what was prepared for which
// batch lives in the CALLER's rc_step_ticket.
namespace {
struct StepSide {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr, fork2 = nullptr, front_done = nullptr;
  bool tried = false, ok = false;
};
constexpr int kMaxDevices = 64;
StepSide* step_side(int* device_out = nullptr) {
  static StepSide sides[kMaxDevices];
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
  if (device_out) *device_out = dev;
  std::lock_guard<std::mutex> lock(mu);
  StepSide& x = sides[dev];
  if (!x.tried) {
    x.tried = true;
    x.ok = hipStreamCreateWithFlags(&x.stream, hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&x.join, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&x.fork2, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&x.front_done, hipEventDisableTiming) == hipSuccess;
  }
  return x.ok ? &x : nullptr;
}
}  // namespace

using namespace rc;

namespace {
// one complete bucket plan of a batch: partition buffers, row records, grouped positions, multi-occurrence bitmap.
// Two slots: the step works from one while the look-ahead writes the plan of the following batch into the other.
struct PlanSlot {
  PlanWs plan;
  rc_plan_row* rows_i;
  rc_plan_row* rows_u;
  uint32_t* occ;
  uint32_t* bitmap;
  PlanLongWs plan_long;   // hot rows of this plan: long-row records, chunk list (+ the chunk partial sums of its updates)
};
struct StepWs {
  uint32_t* keys_i;
  uint32_t* perm_i;
  uint32_t* keys_u;
  uint32_t* perm_u;
  float* gpred;
  float* ugrad;
  float* loss_vec;
  uint8_t* single;
  uint32_t* heads_i;
  uint32_t* n_heads_i;
  void* sort_ws;
  size_t sort_ws_bytes;
  void* seg_ws;
  size_t seg_ws_bytes;
  // bucket-plan step (the default where the id space allows it)
  PlanSlot slot[2];
  void* small_extra;     // small-batch step (small_step.hip): user-row snapshot, per-workgroup row / position segments
  size_t total;
};

StepWs carve_step_ws(void* base, int B, int C, int d) {
  const size_t n_i = (size_t)B * C;
  Carver cv(base);
  StepWs w;
  // item and user ids are sorted together: [0, n_i) is the item segment, [n_i, n_i+B) the users'
  w.keys_i = cv.take<uint32_t>(n_i + (size_t)B);
  w.perm_i = cv.take<uint32_t>(n_i + (size_t)B);
  w.keys_u = w.keys_i + n_i;
  w.perm_u = w.perm_i + n_i;
  w.gpred = cv.take<float>(n_i);
  w.ugrad = cv.take<float>((size_t)B * d);
  w.loss_vec = cv.take<float>((size_t)B);
  const size_t plan_off = cv.off;
  w.single = cv.take<uint8_t>(n_i);
  w.heads_i = cv.take<uint32_t>(n_i);
  w.n_heads_i = cv.take<uint32_t>(1);
  w.sort_ws_bytes = rc_sort_workspace_bytes((int64_t)n_i + B);
  w.sort_ws = cv.take<char>(w.sort_ws_bytes);
  w.seg_ws_bytes = rc_segmented_workspace_bytes((int64_t)n_i, d);
  w.seg_ws = cv.take<char>(w.seg_ws_bytes);
  // the pipelines never run in the same call: the plan buffers overlay the sort / segment scratch
  // (everything after loss_vec)
  Carver pv(base);
  pv.off = plan_off;
  for (int k = 0; k < 2; ++k) {
    const PlanWs pw = carve_plan_ws(base ? reinterpret_cast<char*>(base) + pv.off : nullptr, (int64_t)n_i + B);
    w.slot[k].plan = pw;
    pv.off += align_up(pw.total, 256);
    w.slot[k].rows_i = pv.take<rc_plan_row>(n_i);
    w.slot[k].rows_u = pv.take<rc_plan_row>((size_t)B);
    w.slot[k].occ = pv.take<uint32_t>(n_i + (size_t)B);
    w.slot[k].bitmap = pv.take<uint32_t>(kPlanBitmapWords);
    const PlanLongWs lw = carve_plan_long_ws(base ? reinterpret_cast<char*>(base) + pv.off : nullptr, (int64_t)n_i + B, d);
    w.slot[k].plan_long = lw;
    pv.off += align_up(lw.total, 256);
  }
  w.total = cv.off > pv.off ? cv.off : pv.off;
  // the small-batch step's buffers overlay the same region (the pipelines never run in the same call)
  w.small_extra = base ? reinterpret_cast<char*>(base) + plan_off : nullptr;
  if ((int64_t)n_i + B <= 32768) {
    const size_t need = plan_off + small_step_extra_bytes((int64_t)n_i + B, B, d);
    if (need > w.total) w.total = need;
  }
  return w;
}

// the plan of one batch in slot `k`
PlanArgs slot_plan_args(const StepWs& w, int k, const int64_t* uid, const int64_t* iid, int64_t n_i, int B, int64_t n_users,
                        int64_t n_items, const PlanGeom& geom, bool fused_upd) {
  PlanArgs pa;
  memset(&pa, 0, sizeof(pa));
  const PlanSlot& sl = w.slot[k];
  pa.ids_a = iid; pa.ids_b = uid; pa.n_a = (uint32_t)n_i; pa.n = (uint32_t)(n_i + B);
  pa.range_a = n_items; pa.range_b = n_users;
  pa.g = geom;
  pa.w = sl.plan;
  pa.list_single_a = fused_upd ? 0 : 1;
  pa.single_a = nullptr;
  pa.bitmap_a = fused_upd ? sl.bitmap : nullptr;
  pa.flags_done = 1;   // singleton information, where needed, is the bitmap
  pa.rows_a = sl.rows_i; pa.rows_b = sl.rows_u;
  pa.n_rows_a = &sl.plan.counters[PC_ROWS_A]; pa.n_rows_b = &sl.plan.counters[PC_ROWS_B];
  pa.occ = sl.occ;
  pa.emit_long = 1;
  pa.lw = sl.plan_long;
  // medium rows (5..32 occurrences of an item, 3..32 of a user), listed from the end of the row-record arrays
  pa.med.end[0] = sl.rows_i + n_i; pa.med.cap[0] = (uint32_t)n_i; pa.med.over[0] = kPlanIdxOcc;    // items: plan_rows_indexed_body
  pa.med.end[1] = sl.rows_u + B; pa.med.cap[1] = (uint32_t)B; pa.med.over[1] = kPlanBodyOcc;       // users: plan_rows_body
  return pa;
}
}  // namespace

// 0 = automatic (two-launch step for small batches; else the bucket plan, its per-bucket pass on a second stream behind
// the fused kernel), 1 = always the sort pipeline, 2 = bucket plan on ONE stream, 3 = bucket plan on two streams whatever
// the batch size; 0 until rc_bprmf_step_pipeline sets another
static int& step_pipeline() {
  static int mode = 0;
  return mode;
}

extern "C" int rc_bprmf_step_pipeline(int mode) {
  const int prev = step_pipeline();
  if (mode >= 0 && mode <= 3) step_pipeline() = mode;
  return prev;
}

extern "C" size_t rc_bprmf_step_workspace_bytes(int B, int C, int d) {
  if (B < 1 || C < 1 || d < 1) return 0;
  return carve_step_ws(nullptr, B, C, d).total;
}

// ---- phase marks -------------------------------------------------------------------------------------
// Profiling mode (phase_ms != nullptr): eight hipEvents recorded on the step's stream between its phases.  Without
// phase_ms nothing is created and mark() does nothing; the destructor destroys what was created on every return path.
namespace {
class PhaseMarks {
 public:
  static constexpr int kMarks = 8;
  PhaseMarks() = default;
  PhaseMarks(const PhaseMarks&) = delete;
  PhaseMarks& operator=(const PhaseMarks&) = delete;
  ~PhaseMarks() {
    for (int i = 0; i < n_; ++i) (void)hipEventDestroy(ev_[i]);
  }
  int open(const float* phase_ms, hipStream_t s) {
    s_ = s;
    if (phase_ms != nullptr)
      for (; n_ < kMarks; ++n_) RC_HIP(hipEventCreate(&ev_[n_]));
    return RC_OK;
  }
  bool on() const { return n_ == kMarks; }
  int mark(int i) {
    if (on()) RC_HIP(hipEventRecord(ev_[i], s_));
    return RC_OK;
  }
  // marks [i, ...) for a callee that records them itself (null when off)
  hipEvent_t* at(int i) { return on() ? &ev_[i] : nullptr; }
  // waits for the last mark; event i opens: 0 sort items, 1 mark singletons, 2 sort users, 3 fused, 4 loss mean,
  // 5 item update, 6 user update; reported in the header's slot order
  int report(float* phase_ms) {
    if (!on()) return RC_OK;
    RC_HIP(hipEventSynchronize(ev_[kMarks - 1]));
    const int slot[7] = {0, 7, 1, 2, 3, 4, 5};
    for (int i = 0; i < 7; ++i) RC_HIP(hipEventElapsedTime(&phase_ms[slot[i]], ev_[i], ev_[i + 1]));
    RC_HIP(hipEventElapsedTime(&phase_ms[6], ev_[0], ev_[kMarks - 1]));
    return RC_OK;
  }

 private:
  hipEvent_t ev_[kMarks];
  int n_ = 0;
  hipStream_t s_ = nullptr;
};

// ---- pipeline choice ---------------------------------------------------------------------------------
enum StepPipeline { STEP_SMALL, STEP_PLAN, STEP_SORT };
struct StepChoice {
  StepPipeline pipeline;
  PlanGeom geom;
  bool fused_upd;     // the fused kernel updates single-occurrence item rows itself
  bool two_streams;   // bucket plan: its per-bucket pass (and the look-ahead) on the side stream
  int flavour;        // what a prepared plan contains: 1 = bitmap + multi rows, 2 = every row listed
};

StepChoice choose_pipeline(const BprmfStep& st, bool side_ok) {
  const int mode = step_pipeline();
  const int64_t n_i = st.n_i();
  const bool fused_ok = rc_bprmf_fused_supported(st.d, st.C) != 0;
  StepChoice c;
  // The singleton fast path (update single-occurrence item rows inside the fused kernel) pays for
  // SGD only: with optimizer state the m/v rows have to be fetched at the kernel's tail, where nothing
  // hides their latency (measured at config 2, Adam: 2.98 ms/step fused vs 2.31 ms through the
  // segmented update, which already streams 6 row-units per touched row at the HBM rate).
  // (a hashed plan geometry -- very wide / sparse id spaces -- has no id-indexed bitmap: every row is listed then)
  const bool want_bitmap = fused_ok && st.h->opt == RC_OPT_SGD;   // -> id-range buckets if at all possible
  c.geom = plan_geometry(n_i, st.B, st.n_items, st.n_users, want_bitmap ? 0 : -1);
  // (narrow geometry = dense batch, several occurrences per row of the table: hardly any row occurs once, the singleton
  //  fast path has nothing to win there)
  c.fused_upd = want_bitmap && !c.geom.hashed && !c.geom.narrow;
  c.flavour = c.fused_upd ? 1 : 2;
  c.two_streams = (mode == 0 || mode == 3) && side_ok;
  // Small batches (<= 32,768 row ids, e.g. the reference's default B = 256 with K = 99): two launches (small_step.hip).
  // Otherwise the bucket plan (bucket_plan.hip + plan_update.hip) where the register-resident fused kernel exists and
  // the joint id space fits one bucket level; otherwise (and in pipeline mode 1) the round-1 pipeline: joint radix
  // sort -> segment heads -> fused -> segmented updates.
  if (mode == 0 && fused_ok && small_step_supported(n_i, st.B, st.n_items, st.n_users, st.d) && aligned16(st.U, st.I))
    c.pipeline = STEP_SMALL;
  else if (mode != 1 && c.geom.ok && fused_ok && (st.d == 16 || st.d == 32 || st.d == 64 || st.d == 128))
    c.pipeline = STEP_PLAN;
  else
    c.pipeline = STEP_SORT;
  return c;
}

// ---- look-ahead tickets ------------------------------------------------------------------------------
// What rc_bprmf_train_step_ahead adds to the plain step (ticket == nullptr: the plain step), the device and side
// stream the call runs with, and what ticket_take found.
struct StepAhead {
  rc_step_ticket* ticket;
  uint64_t generation;
  const int64_t* next_uid;
  const int64_t* next_iid;
  uint64_t next_generation;
  int device;
  StepSide* side;
  bool hit;   // the ticket held the plan of exactly this batch ...
  int slot;   // ... in this plan slot (0 without a hit: the step plans into slot 0)
};

bool ticket_matches(const rc_step_ticket* t, uint64_t generation, const void* ws, int device, const BprmfStep& st, int flavour) {
  return t != nullptr && generation != 0 && t->generation == generation && t->ws == reinterpret_cast<uintptr_t>(ws) &&
         t->device == device && t->B == st.B && t->C == st.C && t->d == st.d && t->n_users == st.n_users &&
         t->n_items == st.n_items && t->flavour == flavour && (t->slot == 0 || t->slot == 1);
}

// A plan prepared ahead by an earlier call (rc_step_ticket, caller-owned): usable when it was made for exactly this
// batch -- the caller's generation id, not a pointer, says so -- workspace, geometry and plan flavour.  In every case
// the side stream's writes into the workspace have to be finished before this call touches the plan buffers.
int ticket_take(StepAhead& ah, const void* ws, const BprmfStep& st, int flavour) {
  ah.hit = false;
  ah.slot = 0;
  rc_step_ticket* t = ah.ticket;
  if (t == nullptr || t->generation == 0) return RC_OK;
  RC_REQUIRE(t->device == ah.device, "rc_bprmf_train_step_ahead: the ticket was prepared on device %d, current device %d",
             t->device, ah.device);
  RC_REQUIRE(ah.side != nullptr, "rc_bprmf_train_step_ahead: side stream unavailable on device %d", ah.device);
  ah.hit = ticket_matches(t, ah.generation, ws, ah.device, st, flavour);
  if (ah.hit) ah.slot = t->slot;
  RC_HIP(hipStreamWaitEvent(st.s, ah.side->front_done, 0));
  t->generation = 0;
  return RC_OK;
}

// the plan of the next batch has been enqueued into `slot` on the side stream
void ticket_issue(const StepAhead& ah, const void* ws, int slot, const BprmfStep& st, int flavour) {
  rc_step_ticket* t = ah.ticket;
  t->generation = ah.next_generation;
  t->ws = reinterpret_cast<uintptr_t>(ws);
  t->slot = slot; t->device = ah.device; t->B = st.B; t->C = st.C; t->d = st.d;
  t->flavour = flavour; t->n_users = st.n_users; t->n_items = st.n_items;
}

// ---- the three pipelines -----------------------------------------------------------------------------
inline rc_stream_t as_rc_stream(hipStream_t s) { return reinterpret_cast<rc_stream_t>(s); }

int step_small(const BprmfStep& st, const StepWs& w, PhaseMarks& pm) {
  for (int i = 0; i < 4; ++i) RC_TRY(pm.mark(i));
  RC_TRY(small_step_launch(st, w.small_extra, pm.at(4)));  // marks 4, 5
  RC_TRY(pm.mark(6));
  return pm.mark(7);
}

int step_plan(const BprmfStep& st, const StepWs& w, void* ws, const StepChoice& ch, const StepAhead& ah, PhaseMarks& pm) {
  hipStream_t s = st.s;
  StepSide* side = ah.side;
  const int64_t n_i = st.n_i();
  const bool fused_upd = ch.fused_upd, two_streams = ch.two_streams;
  RC_TRY(plan_prepare());
  const PlanArgs pa = slot_plan_args(w, ah.slot, st.uid, st.iid, n_i, st.B, st.n_users, st.n_items, ch.geom, fused_upd);
  // Look-ahead: the WHOLE plan of the next batch (partition, bitmap, row records, grouped positions) into the other
  // slot, on the side stream.  Not under stream capture (the next call's wait on front_done would cross graphs).
  // (Also in profiling mode: a profiled step is then exactly a step of the steady state, the next plan beside it.)
  bool look_ahead = two_streams && ah.ticket != nullptr && ah.next_generation != 0 && ah.next_uid != nullptr && ah.next_iid != nullptr;
  if (look_ahead) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    look_ahead = hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
  }
  RC_TRY(pm.mark(0));
  if (ah.hit) {
    // the plan is complete (prepared beside the previous step): this step starts with its fused kernel
    RC_TRY(pm.mark(1));
  } else if (two_streams) {
    // caller's stream: partition (+ bitmap when the fused kernel updates singleton rows) -> fused kernel
    // side stream:     per-bucket pass (row records, grouped positions), joined before the updates
    // (without the singleton fast path the fused kernel needs nothing from the plan: all of it runs on the side stream)
    if (fused_upd) RC_TRY(plan_launch_front(pa, true, s));
    RC_TRY(pm.mark(1));
    RC_HIP(hipEventRecord(side->fork, s));
    RC_HIP(hipStreamWaitEvent(side->stream, side->fork, 0));
    if (!fused_upd) RC_TRY(plan_launch_front(pa, false, side->stream));
    RC_TRY(plan_launch_back(pa, side->stream));
    RC_HIP(hipEventRecord(side->join, side->stream));
  } else {
    RC_TRY(plan_launch_front(pa, fused_upd, s));
    RC_TRY(pm.mark(1));   // after the partition (+ bitmap), before the bucket kernel
    RC_TRY(plan_launch_back(pa, s));
  }
  // The look-ahead is forked here, in front of the fused kernel: the plan's chain of latency-bound kernels stretches
  // about 2.5 x beside the bandwidth-bound row kernels and needs the whole step as its window (0.988 -> 0.945 ms/step
  // at config 2 against a fork behind the fused kernel, profiles/r03d_ab_overlap.txt).
  if (look_ahead) {
    PlanArgs pn = slot_plan_args(w, 1 - ah.slot, ah.next_uid, ah.next_iid, n_i, st.B, st.n_users, st.n_items, ch.geom, fused_upd);
    RC_HIP(hipEventRecord(side->fork2, s));
    RC_HIP(hipStreamWaitEvent(side->stream, side->fork2, 0));
    // a plan prepared as a whole: the bucket kernel writes the multi-occurrence bitmap from the counts it holds anyway
    // (the separate bitmap launch zeroes and counts every bucket a second time: 0.06 ms beside the row kernels)
    pn.bitmap_in_bucket = fused_upd ? 1 : 0;   // (fused_upd implies an id-range geometry: neither hashed nor narrow)
    RC_TRY(plan_launch_front(pn, false, side->stream));
    RC_TRY(plan_launch_back(pn, side->stream));
    RC_HIP(hipEventRecord(side->front_done, side->stream));
    ticket_issue(ah, ws, 1 - ah.slot, st, ch.flavour);
  }
  RC_TRY(pm.mark(2));
  RC_TRY(pm.mark(3));
  if (fused_upd)
    RC_TRY(rc_bprmf_fwd_bwd_update(st.U, st.I, st.mI, st.vI, st.uid, st.iid, nullptr, w.slot[ah.slot].bitmap, st.B, st.C, st.d,
                                   st.inv_b, st.h, st.pred, st.loss_vec, st.gpred, st.ugrad, as_rc_stream(s)));
  else
    RC_TRY(rc_bprmf_fwd_bwd(st.U, st.I, st.uid, st.iid, st.B, st.C, st.d, st.inv_b, st.pred, st.loss_vec, st.gpred, st.ugrad,
                            as_rc_stream(s)));
  if (two_streams && !ah.hit) RC_HIP(hipStreamWaitEvent(s, side->join, 0));
  RC_TRY(pm.mark(4));
  RC_TRY(pm.mark(5));  // (the loss mean is one workgroup of the last update launch)
  RC_TRY(plan_bprmf_step_updates(st, pa.rows_a, pa.n_rows_a, pa.rows_b, pa.n_rows_b, pa.occ, pa.w.counters, pa.lw, pa.med, pm.at(6)));
  return pm.mark(7);
}

int step_sort(const BprmfStep& st, const StepWs& w, bool fused_upd, PhaseMarks& pm) {
  const rc_stream_t stream = as_rc_stream(st.s);
  const int64_t n_i = st.n_i();
  RC_TRY(pm.mark(0));
  // one joint radix sort: keys = item id | n_items + user id (all user keys sort after all item keys)
  RC_TRY(rc_sort_ids(st.iid, n_i, st.uid, st.B, st.n_items, st.n_items + st.n_users, w.keys_i, w.perm_i, w.sort_ws, w.sort_ws_bytes,
                     stream));
  RC_TRY(pm.mark(1));
  if (fused_upd) RC_TRY(rc_segment_heads(w.keys_i, w.perm_i, n_i, 1, w.single, w.heads_i, w.n_heads_i, stream));
  RC_TRY(pm.mark(2));
  RC_TRY(pm.mark(3));  // (the user ids were sorted with the item ids)
  if (fused_upd)
    RC_TRY(rc_bprmf_fwd_bwd_update(st.U, st.I, st.mI, st.vI, st.uid, st.iid, w.single, nullptr, st.B, st.C, st.d, st.inv_b, st.h,
                                   st.pred, st.loss_vec, st.gpred, st.ugrad, stream));
  else
    RC_TRY(rc_bprmf_fwd_bwd(st.U, st.I, st.uid, st.iid, st.B, st.C, st.d, st.inv_b, st.pred, st.loss_vec, st.gpred, st.ugrad, stream));
  RC_TRY(pm.mark(4));
  RC_TRY(rc_reduce_sum(st.loss_vec, st.B, st.inv_b, st.loss_out, stream));
  RC_TRY(pm.mark(5));
  // item rows: grad_r = sum_{(b,c): iid[b,c]=r} g[b,c] * U[uid[b]]
  RC_TRY(rc_segmented_update(st.I, st.mI, st.vI, st.d, w.keys_i, w.perm_i, n_i, st.gpred, st.U, st.uid, st.C, nullptr, n_i,
                             /*key_base=*/0, /*occ_base=*/0, st.h, nullptr, fused_upd ? w.heads_i : nullptr,
                             fused_upd ? w.n_heads_i : nullptr, fused_upd ? RC_SEG_SKIP_SINGLETONS : 0, w.seg_ws, w.seg_ws_bytes,
                             stream));
  RC_TRY(pm.mark(6));
  // user rows: grad_r = sum_{b: uid[b]=r} ugrad[b]
  RC_TRY(rc_segmented_update(st.U, st.mU, st.vU, st.d, w.keys_u, w.perm_u, st.B, nullptr, st.ugrad, nullptr, 1, nullptr, st.B,
                             /*key_base=*/st.n_items, /*occ_base=*/n_i, st.h, nullptr, nullptr, nullptr, 0, w.seg_ws,
                             w.seg_ws_bytes, stream));
  return pm.mark(7);
}

// check -> choose -> run.  Everything that inspects only the arguments is refused before the workspace-size check, and
// that before anything is enqueued.  `ah`: ticket / generations / next batch of rc_bprmf_train_step_ahead, zeroes otherwise.
int train_step_impl(float* U, float* I, float* mU, float* vU, float* mI, float* vI, const int64_t* uid, const int64_t* iid, int B,
                    int C, int d, int64_t n_users, int64_t n_items, const rc_opt_hyper* h, float inv_b, float* loss_out, float* pred,
                    void* ws, size_t ws_bytes, rc_stream_t stream, float* phase_ms, StepAhead ah) {
  static const char* who = "rc_bprmf_train_step";
  RC_REQUIRE(U && I && uid && iid && h && loss_out && ws, "%s: null pointer", who);
  RC_REQUIRE(B >= 1 && C >= 2 && d >= 1, "%s: bad shape B=%d C=%d d=%d", who, B, C, d);
  RC_REQUIRE((int64_t)B * C < ((int64_t)1 << 31), "%s: B*C too large", who);
  RC_REQUIRE(U != I, "%s: user and item tables must be distinct", who);
  const StepWs w = carve_step_ws(ws, B, C, d);
  BprmfStep st;
  memset(&st, 0, sizeof(st));
  RC_TRY(fill_opt_scalars(who, h, &st.o));
  st.mode = mode_of(h);
  RC_TRY(opt_state_check(who, st.mode, mU && mI, vU && vI));
  st.U = U; st.I = I; st.mU = mU; st.vU = vU; st.mI = mI; st.vI = vI; st.uid = uid; st.iid = iid;
  st.B = B; st.C = C; st.d = d; st.n_users = n_users; st.n_items = n_items;
  st.h = h; st.inv_b = inv_b; st.loss_out = loss_out; st.pred = pred;
  st.gpred = w.gpred; st.ugrad = w.ugrad; st.loss_vec = w.loss_vec;
  st.s = as_stream(stream);

  ah.side = step_side(&ah.device);
  const StepChoice ch = choose_pipeline(st, ah.side != nullptr);
  if (ch.pipeline == STEP_SORT)
    RC_REQUIRE(n_items + n_users <= ((int64_t)1 << 32), "%s: n_items + n_users exceeds 2^32", who);
  if (ws_bytes < w.total) return fail(RC_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, w.total);

  PhaseMarks pm;
  RC_TRY(pm.open(phase_ms, st.s));
  RC_TRY(ticket_take(ah, ws, st, ch.flavour));
  switch (ch.pipeline) {
    case STEP_SMALL: RC_TRY(step_small(st, w, pm)); break;
    case STEP_PLAN: RC_TRY(step_plan(st, w, ws, ch, ah, pm)); break;
    case STEP_SORT: RC_TRY(step_sort(st, w, ch.fused_upd, pm)); break;
  }
  return pm.report(phase_ms);
}
}  // namespace

extern "C" int rc_bprmf_train_step(float* U, float* I, float* mU, float* vU, float* mI, float* vI,
                                   const int64_t* uid, const int64_t* iid, int B, int C, int d,
                                   int64_t n_users, int64_t n_items, const rc_opt_hyper* h,
                                   float inv_b, float* loss_out, float* pred, void* ws,
                                   size_t ws_bytes, rc_stream_t stream, float* phase_ms) {
  StepAhead none;
  memset(&none, 0, sizeof(none));
  return train_step_impl(U, I, mU, vU, mI, vI, uid, iid, B, C, d, n_users, n_items, h, inv_b, loss_out, pred, ws, ws_bytes, stream,
                         phase_ms, none);
}

extern "C" int rc_bprmf_train_step_ahead(float* U, float* I, float* mU, float* vU, float* mI, float* vI,
                                         const int64_t* uid, const int64_t* iid, uint64_t generation,
                                         const int64_t* next_uid, const int64_t* next_iid, uint64_t next_generation,
                                         rc_step_ticket* ticket, int B, int C, int d, int64_t n_users, int64_t n_items,
                                         const rc_opt_hyper* h, float inv_b, float* loss_out, float* pred, void* ws,
                                         size_t ws_bytes, rc_stream_t stream, float* phase_ms) {
  RC_REQUIRE(ticket != nullptr, "rc_bprmf_train_step_ahead: ticket missing (caller-owned rc_step_ticket, zero-initialised)");
  StepAhead ah;
  memset(&ah, 0, sizeof(ah));
  ah.ticket = ticket; ah.generation = generation; ah.next_uid = next_uid; ah.next_iid = next_iid; ah.next_generation = next_generation;
  return train_step_impl(U, I, mU, vU, mI, vI, uid, iid, B, C, d, n_users, n_items, h, inv_b, loss_out, pred, ws, ws_bytes, stream,
                         phase_ms, ah);
}

// Forget a prepared plan (the owner of the workspace goes away or re-allocates it): `stream` is made to wait for the
// side stream's writes into that workspace, so that whatever reuses the memory afterwards is ordered behind them.
extern "C" int rc_bprmf_step_ahead_reset(rc_step_ticket* ticket, rc_stream_t stream) {
  RC_REQUIRE(ticket != nullptr, "rc_bprmf_step_ahead_reset: ticket missing");
  if (ticket->generation != 0) {
    int cur = 0;
    RC_HIP(hipGetDevice(&cur));
    if (cur != ticket->device) RC_HIP(hipSetDevice(ticket->device));
    StepSide* side = step_side();
    int rc_ = RC_OK;
    if (side != nullptr && hipStreamWaitEvent(as_stream(stream), side->front_done, 0) != hipSuccess)
      rc_ = fail(RC_ERR_HIP, "rc_bprmf_step_ahead_reset: hipStreamWaitEvent failed");
    if (cur != ticket->device) (void)hipSetDevice(cur);
    ticket->generation = 0;
    return rc_;
  }
  return RC_OK;
}
