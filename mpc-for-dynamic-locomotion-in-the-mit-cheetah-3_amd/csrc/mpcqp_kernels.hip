// mpcqp_kernels.hip -- batched convex-MPC QP engine for MI355X (gfx950, wave64).  Hand-written HIP; no CPU path.
//
// Replaces, for a batch of B independent robots, the solve the reference performs once per control tick:
// CasADi Opti('conic') -> OSQP on the QP of src/mpc.py:58-173, filled at src/mpc.py:242-255, solved at :258.
//
// This translation unit is the C-ABI of include/mpcqp.h, mpcqp_plan.h, mpcqp_sim.h, mpcqp_model.h, mpcqp_joints.h, mpcqp_actuators.h, mpcqp_slip.h,
// mpcqp_estimate.h, mpcqp_observe.h, mpcqp_gate.h, mpcqp_attitude.h, mpcqp_disturb.h and mpcqp_compensate.h,
// in three parts: the handle; its host helpers in one anonymous namespace, in order of use (errors, I/O-type dispatch, the solve, workspaces,
// the device guard and the launch tail `on_device`, grids, the policy behind the configuration's defaults, the engine's tables, the roll-out
// loops, the leg rows, the row tables); one extern "C" block of entry points, each its own checks and its own launches.  The device code is in
//   mpcqp_wrench.h       the engine: wrench-space (Woodbury) form, H = 2 alpha I + T'KT with a 6N x 6N system, one QP per wave
//                        (horizon 10) or per four waves (horizon 20), fp32 or fp64 ADMM, fp64 active-set polish, ADMM-only mode
//   mpcqp_stage.h        stage-wise (Riccati) form of the same engine for any other horizon up to 64 -- the reference's own N = 60
//   mpcqp_leg.h          what both engines call on one leg-stage: its structs, the Anderson step, residuals / right-hand side / projection, lane helpers
//   mpcqp_legmap.h       the leg-stage's 6 x 3 wrench map in its two structured forms (ADMM, polish) and the dense one; plain C++, also compiled on the host
//   mpcqp_common.h       what they share besides: operator-tuple descriptor and expansion elements, policy constants, the dispatch-order pre-pass;  mpcqp_device.h: DPP helpers
//   mpcqp_elementwise.h  the element-wise kernels around the solve: gait-descriptor expansion, closed-loop roll-out (expand / advance),
//                        torque map, leg kinematics
//   mpcqp_plan.h         footstep plans, swing-foot trajectories and the plan clock
//   mpcqp_plant.h        the rigid-body plant that can replace the roll-out's world step
//   mpcqp_gaits.h        per-leg periodic gaits: the phase clock, the touchdown foothold rule and their expansion into an operator tuple
//   mpcqp_model.h        per-robot model rows: the conversion of the caller's table into the engine's
//   mpcqp_joints.h       closed-form leg inverse kinematics and the joint-space log of a roll-out
//   mpcqp_actuators.h    per-robot actuator rows: the conversion of the caller's table and the torque-speed envelope the leg kernels share
//   mpcqp_slip.h         stance feet that slide: the stance drive's rule with slip kinematics, and the foot move of its roll-out
//   mpcqp_estimate.h     the torso state from an IMU and leg kinematics: the IMU rows of a log and the filter over them, without and
//                        with the per-leg trust gate and the velocity-aided attitude rule; the filter's row and the sensor rows as
//                        helpers, written once
//   mpcqp_observe.h      sensors and that filter inside the slip roll-out's tick loop, without and with the gate: the encoder row and
//                        two kernels that call mpcqp_estimate.h's helpers around a tick
//   mpcqp_disturb.h      per-robot disturbance wrench rows: the kernels in front of and behind a solve that shift xdes and add the shift back
//                        to the predicted states, and the wrench observer over a roll-out's logs
//   mpcqp_compensate.h   that observer and the table update inside the tick loop of mpcqp_rollout_observe: one kernel per tick
// DESIGN.md has the derivations.

#include "mpcqp_wrench.h"
#include "mpcqp_stage.h"
#include "mpcqp_elementwise.h"
#include "mpcqp_model.h"
#include "mpcqp_joints.h"
#include "mpcqp_actuators.h"
#include "mpcqp_legdyn.h"
#include "mpcqp_legsim.h"
#include "mpcqp_legroll.h"
#include "mpcqp_drive.h"
#include "mpcqp_slip.h"
#include "mpcqp_score.h"
#include "mpcqp_estimate.h"
#include "mpcqp_observe.h"
#include "mpcqp_disturb.h"
#include "mpcqp_compensate.h"
#include "../../include/mpcqp_gate.h"
#include "../../include/mpcqp_attitude.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <type_traits>

#ifndef MPCQP_DIST_LANE_PER_ELEMENT   // (measurement builds only: the shift and add-back kernels with one lane per element, mpcqp_disturb.h)
#define MPCQP_DIST_LANE_PER_ELEMENT 0
#endif
#ifndef MPCQP_DIAG_LDSPAD   // (diagnostic builds only: dynamic LDS that limits the resident workgroups per CU, profiles/r03f_occupancy_study.txt)
#define MPCQP_DIAG_LDSPAD 0
#endif

// ======================================================================================================
// C-ABI (include/mpcqp.h)
// ======================================================================================================
struct mpcqp_engine {
  MpcQpConfig cfg;
  DevCfg dev;
  DevCfg* dcfg = nullptr;   // device copy of `dev`
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int* order_mem = nullptr;   // dispatch order: [2 x 32 header ints (class counters, queue head), alternating between calls | ORDER_BUCKETS x order_cap indices]
  int order_phase = 0;        // which header set the next ordered launch counts into
  int order_cap = 0;
  int slots = 0;              // workgroups the device holds at once (2 per CU)
  int listed_max = 4;         // device-fills up to which an ordered launch is one workgroup per QP (MpcQpConfig.listed_max)
  double* wr_K = nullptr;     // wrench-space engine (mpcqp_wrench.h): K_q [6][N][N], K_q^-1 [6][N][N] (fp32 / fp64)
  float* wr_kinv32 = nullptr;
  double* wr_kinv64 = nullptr;
  float* wr_klane32 = nullptr;   // ... and K^-1 in lane order [NT][16]: the entries of each lane's 8 x 8 tile (w_tile_init); horizon 10: each
                                 // followed by the lane records [NT][16 values | 8 row words] of w_kq_rows_load (mpcqp_rowtab.h)
  double* wr_klane64 = nullptr;
  void* roll_mem = nullptr;   // roll-out: u [B,N,12], X [B,N+1,13], status / iters [B] of the current tick, then the stance drive's
                              // side buffers: applied forces [B,12], torques [B,4,3], flags u8 [B,4] (mpcqp_rollout_drive), then the
                              // slip rule's: displacements [B,4,2] (mpcqp_rollout_slip)
  int64_t roll_cap = 0;
  void* gait_mem = nullptr;   // gait entry point: the expanded operator tuple [r | xdes | contact] of the current batch
  int64_t gait_cap = 0;
  double* plan_ws = nullptr;  // footstep planner: theta, centre x / y, cos / sin theta per (robot, step) [plan_cap][5]
  int64_t plan_cap = 0;
  double* stage_ws = nullptr; // stage-wise engine: factor workspace of the resident workgroups
  int stage_slots = 0;        // ... and how many of them the device holds
  float* dual_mem = nullptr;  // warm-started engines: multipliers of the previous solve per batch slot [dual_cap][4 N][5]
  int64_t dual_cap = 0;
  double* model_mem = nullptr;   // per-robot model rows (include/mpcqp_model.h): the converted table [model_cap][MODEL_ROW]
  int64_t model_B = 0;        // rows of the table that is set; 0 = none, every QP has the configuration's
  int64_t model_cap = 0;
  double* act_mem = nullptr;     // per-robot actuator rows (include/mpcqp_actuators.h): the converted table [act_cap][ACT_ROW]
  int64_t act_B = 0;          // rows of the table that is set; 0 = none, every clamp reads the call's MpcQpLegInertia.tau_max
  int64_t act_cap = 0;
  double* dist_mem = nullptr;    // per-robot disturbance wrench rows (include/mpcqp_disturb.h): the converted table [dist_cap][DIST_ROW]
  int64_t dist_B = 0;         // rows of the table that is set; 0 = none, a solve launches what it launches without the feature
  int64_t dist_cap = 0;
  void* dshift_mem = nullptr;    // ... and the shifted xdes [dist_cap][N+1][13] in the I/O type that a solve reads while a table is set
  bool timed = false;
  char err[512];
};

namespace {

int fail(mpcqp_engine* e, int code, const char* what, hipError_t he = hipSuccess) {
  if (e) {
    if (he != hipSuccess) snprintf(e->err, sizeof(e->err), "%s: %s", what, hipGetErrorString(he));
    else snprintf(e->err, sizeof(e->err), "%s", what);
  }
  return code;
}

// MPCQP_EINVAL with the text "who: what" (what = head + tail), for the checks that several entry points share.
int bad(mpcqp_engine* e, const char* who, const char* head, const char* tail = "") {
  snprintf(e->err, sizeof(e->err), "%s: %s%s", who, head, tail);
  return MPCQP_EINVAL;
}

// The launch check of the entry points that enqueue element-wise kernels.
int launched(mpcqp_engine* e, const char* what) {
  const hipError_t he = hipGetLastError();
  return he == hipSuccess ? MPCQP_OK : fail(e, MPCQP_EHIP, what, he);
}

// The one place where the handle's I/O type becomes a template argument: f is a generic lambda over a value of that type
// (`using T = decltype(tag)`).
template <typename F>
auto with_io(const mpcqp_engine* h, F&& f) { return h->cfg.dtype == MPCQP_DTYPE_F64 ? f(double{}) : f(float{}); }

size_t io_size(const mpcqp_engine* h) { return with_io(h, [](auto tag) { return sizeof(tag); }); }

// Which of the two engines serves a configuration (a valid one: every velocity weight is positive, which both need -- K positive
// definite / Pi_N > 0).  The dense wrench-space engine needs its per-component tables: horizon 10 or 20 and an omega weight that is
// isotropic in x, y (K block diagonal in the wrench components); everything else -- other horizons (the reference's committed
// N = 60, src/main.py:37), anisotropic omega weights (the recursion carries the 2 x 2 coupled weight), MPCQP_FLAG_STAGE_KERNEL --
// runs on the stage-wise engine.
// (any alpha >= 0: a request below 1e-2 -- the reference's own 0.0 included -- is served by continuation, mpcqp_wrench.h)
bool dense_horizon(const MpcQpConfig& c) { return (c.N == 10 || c.N == 20) && !(c.flags & MPCQP_FLAG_STAGE_KERNEL); }
bool wrench_serves(const MpcQpConfig& c) { return dense_horizon(c) && c.w[6] == c.w[7]; }

// The order buffer of one ordered launch: header set `order_phase` (zeroed by the previous ordered launch's pre-pass, or at
// allocation), the other set handed to this launch's pre-pass for clearing.
static OrderBuf next_order_buf(mpcqp_engine* e) {
  OrderBuf ob;
  int* hdr = e->order_mem + 32 * e->order_phase;
  ob.cnt = hdr; ob.head = hdr + ORDER_BUCKETS; ob.zero = e->order_mem + 32 * (1 - e->order_phase);
  ob.list = e->order_mem + 64; ob.cap = e->order_cap;
  e->order_phase ^= 1;
  return ob;
}

// Wrench-space engine (mpcqp_wrench.h).  Horizon 10: one QP per wave, 2 waves per SIMD = 8 resident workgroups per CU, queued
// launch form for batches that oversubscribe them.  Horizon 20: one QP per 4-wave workgroup, plain launch form.
template <typename TIO, int N>
hipError_t launch_wrench(mpcqp_engine* e, int64_t B, const FastIn<TIO>& in, void* u, void* X, int32_t* st, int32_t* it,
                         float* res, hipStream_t s) {
  dim3 grid((unsigned)B);
  OrderBuf ob = {nullptr, nullptr, 0, nullptr, nullptr};
  {
    const int64_t slots = (N == 10 ? 4 : 1) * (int64_t)e->slots;   // e->slots = 2 per CU: resident workgroups of the horizon-20 kernel
    if (!(e->cfg.flags & MPCQP_FLAG_NATURAL_ORDER) && slots > 0 && B > slots && e->order_cap >= B) {
      ob = next_order_buf(e);
      hipLaunchKernelGGL((mpcqp_order_kernel<TIO, N>), dim3((unsigned)((B + 63) / 64)), dim3(1024), 0, s, in, (int)B, ob);
      // Up to a few device-fills the hardware's own dispatcher does better with the ordered list than resident workgroups on an
      // atomic queue (B = 4096: 0.53-0.56 ms against 0.60-0.63, tools/order_study.py): a resident wave stays on the SIMD it
      // started on, next to whatever partner it was given, while a fresh workgroup goes where there is room.
      if (B <= (int64_t)e->listed_max * slots) ob.head = nullptr;
      else grid = dim3((unsigned)slots);
    }
  }
  const WrTabs tabs = {e->wr_K, e->wr_kinv32, e->wr_kinv64, e->wr_klane32, e->wr_klane64};
  // (MODEL: a handle with a model table runs the instantiations that read it; without one, the kernels are what they were)
  auto launch = [&](auto model) {
    constexpr bool MODEL = decltype(model)::value;
    if (e->cfg.precision == MPCQP_PREC_MIXED)
      hipLaunchKernelGGL((mpcqp_wrench_solve<double, float, double, TIO, N, false, MODEL>), grid, dim3(WG<N>::NT), MPCQP_DIAG_LDSPAD, s, e->dcfg, tabs, in,
                         (TIO*)u, (TIO*)X, st, it, res, ob, (int)B);
    else if (e->dev.refine_admm)   // tight-tolerance ADMM-only runs: the instantiation with a refinement step per linear solve
      hipLaunchKernelGGL((mpcqp_wrench_solve<double, double, double, TIO, N, true, MODEL>), grid, dim3(WG<N>::NT), 0, s, e->dcfg, tabs, in, (TIO*)u,
                         (TIO*)X, st, it, res, ob, (int)B);
    else
      hipLaunchKernelGGL((mpcqp_wrench_solve<double, double, double, TIO, N, false, MODEL>), grid, dim3(WG<N>::NT), 0, s, e->dcfg, tabs, in, (TIO*)u,
                         (TIO*)X, st, it, res, ob, (int)B);
  };
  if (e->model_B > 0) launch(std::true_type{}); else launch(std::false_type{});
  return hipGetLastError();
}

// Stage-wise engine (mpcqp_stage.h): persistent workgroups, one QP at a time each, with a factor workspace per workgroup.
template <typename TIO>
hipError_t launch_stage(mpcqp_engine* e, int64_t B, const FastIn<TIO>& in, void* u, void* X, int32_t* st, int32_t* it, float* res, hipStream_t s) {
  const int64_t slots = e->stage_slots > 0 ? e->stage_slots : 256;
  const dim3 grid((unsigned)(B < slots ? B : slots));
  auto launch = [&](auto model) {
    constexpr bool MODEL = decltype(model)::value;
    if (e->cfg.precision == MPCQP_PREC_F64)
      hipLaunchKernelGGL((mpcqp_stage_solve<double, TIO, MODEL>), grid, dim3(SG_NT), 0, s, e->dcfg, in, (TIO*)u, (TIO*)X, st, it, res, e->stage_ws, e->cfg.N, (int)B);
    else
      hipLaunchKernelGGL((mpcqp_stage_solve<float, TIO, MODEL>), grid, dim3(SG_NT), 0, s, e->dcfg, in, (TIO*)u, (TIO*)X, st, it, res, e->stage_ws, e->cfg.N, (int)B);
  };
  if (e->model_B > 0) launch(std::true_type{}); else launch(std::false_type{});
  return hipGetLastError();
}

// Inputs of a solve in the tuple form.  A warm-started engine reads u_out as the initial guess first and keeps the multipliers of
// the previous solve per batch slot.
template <typename T>
FastIn<T> tuple_in(const mpcqp_engine* h, const void* x0, const void* r, const uint8_t* contact, const void* xdes, const void* mu,
                   const void* u_out) {
  const bool warm = (h->cfg.flags & MPCQP_FLAG_WARM_START) != 0;
  FastIn<T> in = {};
  in.x0 = (const T*)x0; in.r = (const T*)r; in.contact = contact; in.xdes = (const T*)xdes; in.mu = (const T*)mu;
  in.u_init = warm ? (const T*)u_out : nullptr;
  in.y_state = warm ? h->dual_mem : nullptr;
  in.shift = (h->cfg.flags & MPCQP_FLAG_WARM_SHIFT) ? 1 : 0;
  return in;
}

// ... and in the gait form, which the expansion kernel reads.
template <typename T>
FastIn<T> gait_in(const void* x0, const void* mu, const void* ref, const void* feet0, const void* footholds, const int32_t* gait,
                  const uint8_t* feet_id) {
  FastIn<T> in = {};
  in.x0 = (const T*)x0; in.mu = (const T*)mu; in.ref = (const T*)ref; in.feet0 = (const T*)feet0;
  in.footholds = (const T*)footholds; in.gait = gait; in.feet_id = feet_id;
  return in;
}

dim3 blocks(int64_t n, int per = 256);   // (with the launch grids, below)

// Picks the engine and launches it.
template <typename T>
hipError_t enqueue_engine(mpcqp_engine* h, int64_t B, const FastIn<T>& in, T* u, T* X, int32_t* status, int32_t* iters, float* res,
                          hipStream_t st) {
  if (!wrench_serves(h->cfg)) return launch_stage<T>(h, B, in, u, X, status, iters, res, st);
  if (h->cfg.N == 10) return launch_wrench<T, 10>(h, B, in, u, X, status, iters, res, st);
  return launch_wrench<T, 20>(h, B, in, u, X, status, iters, res, st);
}

// What the shift rule of include/mpcqp_disturb.h takes from the configuration, and the model table it reads when one is set.
DistCfg dist_cfg(const mpcqp_engine* h) {
  return {h->cfg.delta, h->dev.theta, h->dev.inv_m, {h->dev.Ib[0], h->dev.Ib[1], h->dev.Ib[2]}};
}
const double* model_table(const mpcqp_engine* h) { return h->model_B > 0 ? h->model_mem : nullptr; }

// The shift kernel on B robots: out = xdes - s.
template <typename T>
void launch_disturb_shift(const mpcqp_engine* h, int64_t B, const T* x0, const T* xdes, T* out, hipStream_t st) {
  const int64_t rows = B * (h->cfg.N + 1);
#if MPCQP_DIST_LANE_PER_ELEMENT
  hipLaunchKernelGGL((mpcqp_disturb_element_kernel<T, false>), blocks(rows * 13), dim3(256), 0, st, (const double*)h->dist_mem, model_table(h),
                     dist_cfg(h), x0, xdes, out, h->cfg.N + 1, rows * 13);
#else
  hipLaunchKernelGGL((mpcqp_disturb_shift_kernel<T>), blocks(rows), dim3(256), 0, st, (const double*)h->dist_mem, model_table(h), dist_cfg(h), x0,
                     xdes, out, h->cfg.N + 1, rows);
#endif
}

// The solve proper, shared by every entry point that solves and every roll-out's tick.  No checks, no events; the caller has
// reserved the workspace for B (reserve_workspace) and holds the device.  This is the single hook of the disturbance table
// (include/mpcqp_disturb.h): while one is set -- the caller has matched its size against B -- the solve reads xdes - s from the
// engine's buffer, written here before anything reads in.xdes (the dispatch-order pre-pass is inside launch_wrench), and s is added
// to X behind it.  Without a table this is enqueue_engine and nothing else.
template <typename T>
hipError_t enqueue_solve(mpcqp_engine* h, int64_t B, const FastIn<T>& in, T* u, T* X, int32_t* status, int32_t* iters, float* res,
                         hipStream_t st) {
  if (h->dist_B == 0) return enqueue_engine<T>(h, B, in, u, X, status, iters, res, st);
  FastIn<T> shifted = in;
  shifted.xdes = (const T*)h->dshift_mem;
  launch_disturb_shift<T>(h, B, in.x0, in.xdes, (T*)h->dshift_mem, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = enqueue_engine<T>(h, B, shifted, u, X, status, iters, res, st);
  if (e != hipSuccess || !X) return e;
  const int64_t rows = B * (h->cfg.N + 1);
#if MPCQP_DIST_LANE_PER_ELEMENT
  hipLaunchKernelGGL((mpcqp_disturb_element_kernel<T, true>), blocks(rows * 13), dim3(256), 0, st, (const double*)h->dist_mem, model_table(h),
                     dist_cfg(h), in.x0, (const T*)X, X, h->cfg.N + 1, rows * 13);
#else
  hipLaunchKernelGGL((mpcqp_disturb_addback_kernel<T>), blocks(rows), dim3(256), 0, st, (const double*)h->dist_mem, model_table(h), dist_cfg(h),
                     in.x0, X, h->cfg.N + 1, rows);
#endif
  return hipGetLastError();
}

// The event pair behind mpcqp_last_kernel_ms: an entry point records ev0 in front of its first launch and ev1 behind its last.
int record(mpcqp_engine* h, hipEvent_t ev, hipStream_t st) {
  if (h->cfg.flags & MPCQP_FLAG_NO_TIMING) return MPCQP_OK;
  const hipError_t he = hipEventRecord(ev, st);
  if (he != hipSuccess) return fail(h, MPCQP_EHIP, "hipEventRecord", he);
  if (ev == h->ev1) h->timed = true;
  return MPCQP_OK;
}

// ... around what a solving entry point enqueues: ev0, enqueue() -> hipError_t (`what` names it when it fails), ev1.
template <typename F>
int timed(mpcqp_engine* h, hipStream_t st, const char* what, F&& enqueue) {
  if (const int rc = record(h, h->ev0, st)) return rc;
  const hipError_t he = enqueue();
  if (he != hipSuccess) return fail(h, MPCQP_EHIP, what, he);
  return record(h, h->ev1, st);
}

// Grows a device buffer to `bytes` (contents are not kept), the first `zero` of them cleared; false when the allocation fails, and
// the old buffer then stays.
template <typename P>
bool grow(P*& buf, size_t bytes, size_t zero = 0) {
  void* mem = nullptr;
  if (hipMalloc(&mem, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }   // (do not leave the error for a launch check)
  if (buf) { (void)hipDeviceSynchronize(); (void)hipFree(buf); }                         // queued work may still read the old one
  if (zero) {
    (void)hipMemset(mem, 0, zero);
    (void)hipDeviceSynchronize();   // (the fill runs on the null stream: work on a non-blocking stream must not overtake it and read garbage)
  }
  buf = (P*)mem;
  return true;
}

// The handle's three per-robot row tables (include/mpcqp_model.h, mpcqp_actuators.h, mpcqp_disturb.h) behind one view: the converted rows, how many of
// them are set (0 = no table) and how many the buffer holds.  (A view, not a member: launch_wrench and launch_stage read model_B by name.)
struct RowTable { double*& mem; int64_t& B; int64_t& cap; };
RowTable models(mpcqp_engine* h) { return {h->model_mem, h->model_B, h->model_cap}; }
RowTable actuators(mpcqp_engine* h) { return {h->act_mem, h->act_B, h->act_cap}; }
RowTable disturbances(mpcqp_engine* h) { return {h->dist_mem, h->dist_B, h->dist_cap}; }
// The converted actuator rows, or null when none are set (launch_act)
const double* act_table(const mpcqp_engine* h) { return h->act_B > 0 ? h->act_mem : nullptr; }

// The batch of a call that reads a table against the table, when one is set: row b belongs to batch slot b.
int table_match(mpcqp_engine* h, const RowTable& t, const char* noun, int64_t B, const char* who) {
  if (t.B == 0 || t.B == B) return MPCQP_OK;
  snprintf(h->err, sizeof(h->err), "%s: batch size %lld, but the %s table has %lld rows", who, (long long)B, noun, (long long)t.B);
  return MPCQP_EINVAL;
}
// ... of an entry point that solves: the two tables a solve reads, the model rows and the disturbance rows.
int solve_tables_match(mpcqp_engine* h, int64_t B, const char* who) {
  if (const int rc = table_match(h, models(h), "model", B, who)) return rc;
  return table_match(h, disturbances(h), "disturbance", B, who);
}
int actuators_match(mpcqp_engine* h, int64_t B, const char* who) { return table_match(h, actuators(h), "actuator", B, who); }

// Room for B rows of `width` doubles, once per size like the mpcqp_reserve workspace (grow waits for the device before it frees the old
// buffer; when the allocation fails -- false -- the old table stays set).  After growth no table is set: the old rows are gone, and until
// the caller's conversion kernel has run nothing may read the new buffer.
bool table_reserve(const RowTable& t, int64_t B, int width) {
  if (t.cap >= B) return true;
  if (!grow(t.mem, (size_t)B * width * sizeof(double))) return false;
  t.cap = B; t.B = 0;
  return true;
}

// Room for a disturbance table of B rows and the shifted xdes a solve reads under it (mpcqp_set_disturbance and the entry of
// mpcqp_rollout_observe_compensated; the caller holds the device).  The buffer first: when it cannot be grown, the table set before stays.
int reserve_disturbance(mpcqp_engine* h, int64_t B, const char* who) {
  if (h->dist_cap >= B) return MPCQP_OK;
  char msg[128];
  if (!grow(h->dshift_mem, (size_t)B * (h->cfg.N + 1) * 13 * io_size(h))) {
    snprintf(msg, sizeof(msg), "%s: buffer allocation failed", who);
    return fail(h, MPCQP_ENOMEM, msg);
  }
  if (!table_reserve(disturbances(h), B, DIST_ROW)) {   // (the buffer is larger than the table's rows need: harmless)
    snprintf(msg, sizeof(msg), "%s: table allocation failed", who);
    return fail(h, MPCQP_ENOMEM, msg);
  }
  return MPCQP_OK;
}

// Workspace that depends on the batch size: the dispatch-order buffer of the queued launch forms and, for warm-started
// engines, the per-slot multiplier record.  Sized by mpcqp_reserve(); a solve at a larger B than reserved grows them on the
// spot (a device-wide synchronisation + allocation -- the only ones a solve can make, and only the first time).
int reserve_workspace(mpcqp_engine* e, int64_t B) {
  if (B <= 0) return MPCQP_OK;
  const bool stage = !wrench_serves(e->cfg);
  if (stage && !e->stage_ws) {   // (fixed size: one factor workspace per resident workgroup)
    const int64_t slots = e->stage_slots > 0 ? e->stage_slots : 256;
    if (!grow(e->stage_ws, (size_t)slots * SG_WS_DOUBLES * sizeof(double))) return MPCQP_ENOMEM;
  }
  if (!stage && e->order_cap < B) {
    const int64_t cap = ((B + 1023) / 1024) * 1024;
    // both header sets start cleared; an allocation failure is tolerated: the batch runs in natural order
    if (grow(e->order_mem, (size_t)(64 + ORDER_BUCKETS * cap) * sizeof(int), 64 * sizeof(int))) { e->order_cap = (int)cap; e->order_phase = 0; }
  }
  if ((e->cfg.flags & MPCQP_FLAG_WARM_START) && e->dual_cap < B) {   // (written out: the only buffer whose old contents are kept)
    float* mem = nullptr;
    const size_t per = (size_t)20 * e->cfg.N;   // 4 N leg-stages x 5 rows
    if (hipMalloc(&mem, (size_t)B * per * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return MPCQP_ENOMEM; }
    (void)hipDeviceSynchronize();
    (void)hipMemset(mem, 0, (size_t)B * per * sizeof(float));   // new slots start at zero = no record
    if (e->dual_mem) { (void)hipMemcpy(mem, e->dual_mem, (size_t)e->dual_cap * per * sizeof(float), hipMemcpyDeviceToDevice); (void)hipFree(e->dual_mem); }
    (void)hipDeviceSynchronize();
    e->dual_mem = mem; e->dual_cap = B;
  }
  return MPCQP_OK;
}

// The two per-batch workspaces of the gait entry point and the roll-out share a layout: [B,N,12] | [B,N+1,13] in the I/O type, then
// a tail per QP -- the operator tuple r | xdes | contact [B,N,4] bytes, and the roll-out's results u | X | status, iters [B] int32.
constexpr size_t tuple_elems(size_t N) { return N * 12 + (N + 1) * 13; }   // r and xdes (or u and X) elements of one QP
size_t ws_bytes(int64_t B, size_t N, size_t el, size_t tail) { return (size_t)B * (tuple_elems(N) * el + tail); }

template <typename T> struct TupleWs { T* r; T* xdes; uint8_t* contact; };
template <typename T> struct ResultWs { T* u; T* X; int32_t* status; int32_t* iters; };
template <typename T> struct DriveWs { T* f; T* tau; uint8_t* flag; };   // behind ResultWs in the roll-out's reserve

template <typename T>
TupleWs<T> tuple_ws(void* base, int64_t B, size_t N) {
  T* r = (T*)base;
  return {r, r + (size_t)B * N * 12, (uint8_t*)(r + (size_t)B * tuple_elems(N))};
}
template <typename T>
ResultWs<T> result_ws(void* base, int64_t B, size_t N) {
  T* u = (T*)base;
  int32_t* status = (int32_t*)(u + (size_t)B * tuple_elems(N));
  return {u, u + (size_t)B * N * 12, status, status + B};
}

template <typename T>
DriveWs<T> drive_ws(void* base, int64_t B, size_t N) {   // (status and iters are 8 B bytes: a double stays aligned)
  T* f = (T*)(result_ws<T>(base, B, N).iters + B);
  return {f, f + (size_t)B * 12, (uint8_t*)(f + (size_t)B * 24)};
}
constexpr size_t drive_tail(size_t el) { return 24 * el + 4; }   // bytes per robot of DriveWs

// The displacement side buffer of mpcqp_rollout_slip, [B,4,2] in the I/O type behind DriveWs (the flags end on a multiple of 4 bytes:
// the buffer starts at the next multiple of 8, which the reserve's 8 spare bytes pay for).
template <typename T>
T* slip_ws(void* base, int64_t B, size_t N) {
  const uintptr_t end = (uintptr_t)(drive_ws<T>(base, B, N).flag + (size_t)B * 4);
  return (T*)((end + 7) & ~(uintptr_t)7);
}
constexpr size_t slip_tail(size_t el) { return 8 * el; }   // bytes per robot of the displacement buffer

// The side buffers of mpcqp_rollout_observe behind the displacement buffer (which ends on a multiple of 8 bytes): the state the
// controller reads, x^ [B,13] and f^eet [B,4,3], and the sensor row its predict step reads back, [B,OBS_SENSE], in the I/O type.
template <typename T>
ObsWs<T> observe_ws(void* base, int64_t B, size_t N) {
  T* xhat = slip_ws<T>(base, B, N) + (size_t)B * 8;
  return {xhat, xhat + (size_t)B * 13, xhat + (size_t)B * 25};
}
constexpr size_t observe_tail(size_t el) { return (25 + OBS_SENSE) * el; }   // bytes per robot of the three

// Tuple workspace of the gait entry point and the roll-out, grown like the rest of the batch-dependent workspace.
int reserve_gait(mpcqp_engine* e, int64_t B) {
  if (B <= e->gait_cap) return MPCQP_OK;
  const size_t N = (size_t)e->cfg.N;
  if (!grow(e->gait_mem, ws_bytes(B, N, io_size(e), N * 4))) return MPCQP_ENOMEM;
  e->gait_cap = B;
  return MPCQP_OK;
}

// Result workspace of the roll-out.  Zeros = "no guess" for a warm-started engine.  One reserve serves every roll-out entry point, so
// all of them pay for the side buffers of the drive, the slip rule and mpcqp_rollout_observe (the last: 33 I/O elements per robot),
// whichever of them the handle goes on to call.
int reserve_roll(mpcqp_engine* e, int64_t B) {
  if (B <= e->roll_cap) return MPCQP_OK;
  const size_t bytes = ws_bytes(B, (size_t)e->cfg.N, io_size(e), 2 * sizeof(int32_t) + drive_tail(io_size(e)) + slip_tail(io_size(e)) +
                                                                               observe_tail(io_size(e))) + 8;
  if (!grow(e->roll_mem, bytes, bytes)) return MPCQP_ENOMEM;
  e->roll_cap = B;
  return MPCQP_OK;
}

// Every entry point runs on the handle's device whatever the caller's current device is, and puts that one back.
struct DeviceGuard {
  int prev = -1; bool switched = false; hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); switched = err == hipSuccess; }
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
// ... as one statement of an entry point, behind its own checks: from here to the end of the scope the handle's device is current.
#define GUARD(h) \
  DeviceGuard guard((h)->cfg.device); \
  if (guard.err != hipSuccess) return fail(h, MPCQP_EHIP, "hipSetDevice", guard.err)

// The tail of every entry point that ends in element-wise launches: the guard, f(tag) with the I/O type (with_io) enqueues, and the
// launch check under the name `what`.
template <typename F>
int on_device(mpcqp_engine* h, const char* what, F&& f) {
  GUARD(h);
  with_io(h, f);
  return launched(h, what);
}

// Launch grids: `per` threads a block over n threads, and the three that recur -- one thread per leg of `rows` robots or log rows, one per
// robot (the roll-outs' advance), one per tuple element (their expand).
dim3 blocks(int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); }
dim3 leg_grid(int64_t rows) { return blocks(4 * rows); }
dim3 advance_grid(int64_t B) { return blocks(B); }
dim3 expand_grid(int64_t B, int N) { return blocks(B * (int64_t)tuple_elems(N)); }

// mpcqp_create, step 1: is this a configuration an engine can serve?
bool config_valid(const MpcQpConfig& c) {
  if (c.N < 1 || c.N > SG_NS) return false;
  if (c.precision < MPCQP_PREC_F32 || c.precision > MPCQP_PREC_F64) return false;
  if (c.dtype != MPCQP_DTYPE_F32 && c.dtype != MPCQP_DTYPE_F64) return false;
  if (c.disc != MPCQP_DISC_EULER && c.disc != MPCQP_DISC_ZOH) return false;
  if (!(c.delta > 0) || !(c.m > 0) || !(c.rho > 0) || !(c.sigma >= 0) || !(c.relax > 0 && c.relax < 2) || c.max_iter < 1 ||
      c.max_iter >= MPCQP_ITERS_WIDE || c.check_every < 1 || c.polish_max < 0 || !(c.alpha >= 0) || !(c.f_max >= c.f_min))
    return false;
  for (int i = 0; i < 13; ++i)
    if (!(c.w[i] >= 0)) return false;
  for (int i = 6; i < 12; ++i)
    if (!(c.w[i] > 0)) return false;   // (a zero velocity weight: no engine serves it)
  return true;
}

// mpcqp_create, step 2: the configuration and the policy behind its defaults, resolved into what the kernels read.  Host arithmetic
// only.  Engine tuning fields of the configuration: 0 = default (include/mpcqp.h).  The library reads no environment variables.
void resolve_policy(const MpcQpConfig& cfg, DevCfg& d, int& listed_max) {
  const int N = cfg.N;
  const bool wrench = wrench_serves(cfg), polish = (cfg.flags & MPCQP_FLAG_POLISH) != 0;
  d.delta = cfg.delta; d.inv_m = 1.0 / cfg.m;
  for (int i = 0; i < 3; ++i) d.Ib[i] = cfg.Ibody_inv[i];
  for (int i = 0; i < 12; ++i) { d.w[i] = cfg.w[i]; d.sw[i] = sqrt(cfg.w[i]); }
  d.alpha = cfg.alpha; d.fmin = cfg.f_min; d.fmax = cfg.f_max;
  d.rho = cfg.rho; d.sigma = cfg.sigma; d.relax = cfg.relax;
  d.eps_abs = cfg.eps_abs; d.eps_rel = cfg.eps_rel;
  d.theta = cfg.disc == MPCQP_DISC_ZOH ? 0.5 : 0.0;
  d.max_iter = cfg.max_iter; d.check_every = cfg.check_every; d.polish_max = cfg.polish_max;
  d.flags = cfg.flags;
  // Stage-wise engine: the recursion's solve carries ~10 x the error of the dense fp64 sweep (tools/stage_proto.py), and the Woodbury
  // form amplifies it by 1 / (2 alpha): the alpha = 0 continuation of this engine ends at 2e-5 (objective within 2e-7, states within
  // 9e-5 of the alpha = 0 optimum on the golden log ticks at N = 10 / 20 / 60; at 1e-5 the polish refinement stops contracting at
  // N = 60, tools/stage_floor.py)
  d.alpha_floor = cfg.alpha_floor > 0 ? cfg.alpha_floor : (wrench ? ALPHA_FLOOR : SG_ALPHA_FLOOR);
  // the regulariser a solve ends with and the one it starts with (continuation, mpcqp_wrench.h): decided here, not per QP on the device
  d.alpha_target = d.alpha > 0.0 ? d.alpha : (polish ? d.alpha_floor : 0.0);
  d.alpha_start = (polish && d.alpha < ALPHA_EASY) ? ALPHA_EASY : d.alpha;
  // Early rho check (wrench engine): the ratio beyond which a QP is given a larger penalty and a longer block.  The all-fp64 ADMM
  // sees a clean dual residual and larger ratios than the fp32-tile one, whose dual residual carries the solve's rounding noise;
  // chosen on batches of other seeds than the bench's (tools/adapt_sweep.py).
  d.adapt_thr = cfg.adapt_thr > 0 ? cfg.adapt_thr : (cfg.precision == MPCQP_PREC_F64 ? 15.f : (N > 10 ? 10.f : 6.f));
  // Anderson acceleration of the ADMM blocks (mpcqp_wrench.h): with the polish only -- an ADMM-only run stays OSQP's algorithm 1.
  // The dense engine runs it in its fp32 iterations (MIXED; next to an fp64 iteration tile the history does not fit).
  d.accel_p = !polish ? 0 : (cfg.accel > 0 ? cfg.accel : (cfg.accel < 0 ? 0 : 5));
  const bool accel_runs = d.accel_p > 0 && (!wrench || cfg.precision != MPCQP_PREC_F64);
  // (the block lengths below were swept with the acceleration on the dense engine only.  They are keyed on the dense engine's
  //  horizons and arithmetic, not on the engine: an anisotropic omega weight at horizon 10 or 20 runs the stage-wise engine with them)
  const bool accel_dense = d.accel_p > 0 && cfg.precision != MPCQP_PREC_F64 && dense_horizon(cfg);
  const bool accel_n10 = accel_dense && N == 10;
  // The early rho check (iteration 25) was built for the plain iteration: it buys a slowly converging QP a larger penalty and a
  // longer block up front.  With the acceleration it costs more than it brings -- the residual ratio it reads is taken a few iterations
  // after an extrapolation, the rebuild restarts the history, and the extrapolation does for those QPs what the penalty did.  Never
  // flagging: horizon 10 held-out mean 9.9 -> 10.7 M QP/s, B = 65 536 15.6 -> 16.4 M; stage-wise engine at N = 60: the 1000 logged
  // ticks 143 -> 221 k QP/s (MIXED: every tick solved in its first block), synthetic 62 -> 93 k (profiles/r03f_early_check.txt).
  // Horizon 20 (config 5): 1.32 -> 1.65 M.  So where the acceleration runs the check is off unless the caller asks for it with an explicit adapt_thr.
  d.early_check = (cfg.adapt_thr > 0 || !accel_runs) ? 1 : 0;
  d.accel_restart = (d.accel_p > 0 && cfg.accel_restart > 0) ? cfg.accel_restart : 0;
  // A cold solve's first ADMM block is 0.7 check_every long: most QPs have their active set by then (mean iterations 114 -> 82 at
  // N = 10, B = 65 536: 14.6 -> 16.2 M QP/s, N = 20: +10 %), the others go on in full blocks; at B = 4096, where the launch is as
  // long as its hardest QPs, neutral (eight batches of other seeds, tools/adapt_sweep.py).  With the polish only: an ADMM-only
  // run keeps OSQP's uniform check interval.
  // With the acceleration the active set is there sooner: 0.6 check_every (tools/accel_sweep.py, profiles/r03_accel_sweep.txt).
  const int first_block = polish ? ((accel_dense ? 6 : 7) * cfg.check_every) / 10 : 0;
  d.first_block = cfg.first_block > 0 ? cfg.first_block : (cfg.first_block < 0 ? 0 : first_block);
  const int incr_legs = cfg.incr_legs < MPCQP_W_INCR_LEGS ? cfg.incr_legs : MPCQP_W_INCR_LEGS;
  d.incr_legs = cfg.incr_legs > 0 ? incr_legs : (cfg.incr_legs < 0 ? 0 : MPCQP_W_INCR_LEGS);
  listed_max = cfg.listed_max > 0 ? cfg.listed_max : (cfg.listed_max < 0 ? 0 : 4);
  d.patience = cfg.polish_patience > 0 ? cfg.polish_patience : POLISH_PATIENCE;
  // (horizon 10 only by default: at N = 20 an update of the 120 x 120 inverse costs four times as much, and config 5 lost 7 % with the rule on)
  d.cheap_steps = cfg.polish_cheap_steps > 0 ? cfg.polish_cheap_steps : (cfg.polish_cheap_steps < 0 || N > 10 ? 0 : POLISH_CHEAP_STEPS);
  d.cheap_legs = cfg.polish_cheap_legs > 0 ? cfg.polish_cheap_legs : POLISH_CHEAP_LEGS;
  // A QP that the early rho check flags gets a first block three times the normal one at horizon 10 (seven batches of other seeds than
  // the bench's, tools/patience_sweep.py, profiles/r03_hard_block_sweep.txt: x2 / x2.5 / x3 / x3.5 -> 8.62 / 8.63 / 9.15 / 9.13 M QP/s on
  // their mean at B = 4096: fewer of them need a third round, and the launch is as long as its longest QP; B = 65 536 pays 3 % for the
  // extra iterations).  Horizon 20 keeps x2 (not re-swept).
  // With the acceleration the longer block buys nothing (x1 / x1.5 / x2 / x3: same held-out mean within run-to-run spread, the large
  // batch fastest at x1): a flagged QP gets the larger penalty and the normal block.
  d.hard_x10 = cfg.hard_block_x10 > 0 ? cfg.hard_block_x10 : (N > 10 ? 10 * HARD_ITER_FACTOR : (accel_n10 ? 10 : 30));
  // The round that nothing follows (iteration cap reached) used to run its whole polish budget; it now gives up after four steps that
  // fail to halve the KKT violation (horizon 10: 9.04 -> 9.35 M on the held-out mean, the same QPs solved, profiles/r03_last_patience_sweep.txt)
  d.last_patience = cfg.polish_last_patience > 0 ? cfg.polish_last_patience : (cfg.polish_last_patience < 0 || N > 10 ? 0 : 4);
  d.model = nullptr;   // (the device copy's is set by mpcqp_set_models)
  d.refine_admm = (!polish && cfg.precision == MPCQP_PREC_F64 && cfg.eps_abs < 1e-6) ? 1 : 0;
}

// A host array that owns its memory and reads as the pointer to it; null (no exception) when there is none.
template <typename T>
struct HostArray {
  T* const p;
  explicit HostArray(size_t n) : p(new (std::nothrow) T[n]) {}
  HostArray(const HostArray&) = delete;
  ~HostArray() { delete[] p; }
  operator T*() const { return p; }
};

// A device buffer of `bytes` filled from the host.
template <typename P>
hipError_t upload(P*& dst, const void* src, size_t bytes) {
  const hipError_t he = hipMalloc((void**)&dst, bytes);
  return he == hipSuccess ? hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) : he;
}

// Inverse of a small SPD matrix by Gauss-Jordan with partial pivoting (host, fp64); returns false when singular.
bool invert_small(int n, const double* A, double* Ai) {
  const HostArray<double> M((size_t)2 * n * n);
  if (!M) return false;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) { M[i * 2 * n + j] = A[i * n + j]; M[i * 2 * n + n + j] = i == j ? 1.0 : 0.0; }
  bool ok = true;
  for (int k = 0; k < n && ok; ++k) {
    int piv = k;
    for (int i = k + 1; i < n; ++i) if (fabs(M[i * 2 * n + k]) > fabs(M[piv * 2 * n + k])) piv = i;
    if (!(fabs(M[piv * 2 * n + k]) > 0)) { ok = false; break; }
    if (piv != k) for (int j = 0; j < 2 * n; ++j) { const double t = M[k * 2 * n + j]; M[k * 2 * n + j] = M[piv * 2 * n + j]; M[piv * 2 * n + j] = t; }
    const double p = 1.0 / M[k * 2 * n + k];
    for (int j = 0; j < 2 * n; ++j) M[k * 2 * n + j] *= p;
    for (int i = 0; i < n; ++i) {
      if (i == k) continue;
      const double f = M[i * 2 * n + k];
      if (f != 0) for (int j = 0; j < 2 * n; ++j) M[i * 2 * n + j] -= f * M[k * 2 * n + j];
    }
  }
  if (ok) for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) Ai[i * n + j] = M[i * 2 * n + n + j];
  return ok;
}

// mpcqp_create, step 3 for the wrench-space engine (mpcqp_wrench.h): K_q = 2 (wP_q c1 + wQ_q c0) and its inverse per wrench
// component, the latter in fp64 and rounded to fp32, from the coefficient tables
//   c0[j][j'] = delta^2 (N - max(j,j')),   c1[j][j'] = delta^4 sum_{k > max(j,j')}^{N} (k-1-j+theta)(k-1-j'+theta)
// MPCQP_OK, or why the tables are not there (out of memory; MPCQP_EINVAL for weights that leave a K_q singular in fp64).
//
// The lane-order table: lane t = G gr + gc of the tile grid holds rows R = 8 gr + r, columns C = 8 gc + c of
//   S0 = [ K^-1 in stage-major order (index 6 j + q: S0[R][C] = Ki[q][R / 6][C / 6] iff R = C (mod 6), else 0)   0 ]
//        [ 0                                                                                                      I ]   (8 G x 8 G)
// Row r of the tile has its first K^-1 entry at tile column c0 = (r + 2 k) mod 6 with k = (gr - gc) mod 3, and a second one at
// c0 + 6 when c0 < 2: slot [t][r] = S0[R][8 gc + c0], slot [t][8 + r] = S0[R][8 gc + c0 + 6] (0 when c0 >= 2).
template <int N>
void lane_order_kinv(const double* Ki, double* lane) {
  constexpr int G = WG<N>::G, NQ = WG<N>::NQ;
  auto S0 = [&](int R, int C) -> double {
    if (R >= NQ || C >= NQ) return R == C ? 1.0 : 0.0;
    return R % 6 == C % 6 ? Ki[((R % 6) * N + R / 6) * N + C / 6] : 0.0;
  };
  for (int t = 0; t < G * G; ++t) {
    const int gr = t / G, gc = t % G, k = ((gr - gc) % 3 + 3) % 3;
    for (int r = 0; r < 8; ++r) {
      const int c0 = (r + 2 * k) % 6;
      lane[16 * t + r] = S0(8 * gr + r, 8 * gc + c0);
      lane[16 * t + 8 + r] = c0 < 2 ? S0(8 * gr + r, 8 * gc + c0 + 6) : 0.0;
    }
  }
}

template <int N>
int build_wrench_tables(mpcqp_engine* e) {
  const MpcQpConfig& c = e->cfg;
  constexpr int NK = 6 * N * N, NLANE = 16 * WG<N>::NT;
  // The device images of the two lane tables: [NT][16] values and, at horizon 10 (whose MIXED kernels read them), one record per lane
  // behind them -- the same sixteen values and the lane's eight row words of the tile build (mpcqp_rowtab.h)
  constexpr int NREC = N == 10 ? WG<N>::NT : 0;
  constexpr size_t L32 = sizeof(float) * NLANE + NREC * mpcqp_rowtab::record_bytes<float>();
  constexpr size_t L64 = sizeof(double) * NLANE + NREC * mpcqp_rowtab::record_bytes<double>();
  const HostArray<double> tab(2 * N * N), K(NK), Ki(NK), Kl(NLANE);   // tab: c0 | c1
  const HostArray<float> Ki32(NK), Kl32(NLANE);
  const HostArray<unsigned> rows(mpcqp_rowtab::ROW_WORDS * WG<N>::NT);
  const HostArray<unsigned char> img(L32 + L64);
  if (!(tab && K && Ki && Ki32 && Kl && Kl32 && rows && img)) return MPCQP_ENOMEM;
  const double dl = c.delta, th = e->dev.theta;
  for (int a = 0; a < N; ++a)
    for (int bq = 0; bq < N; ++bq) {
      const int mx = a > bq ? a : bq;
      tab[a * N + bq] = dl * dl * (double)(N - mx);
      double sacc = 0;
      for (int k = mx + 1; k <= N; ++k) sacc += ((double)(k - 1 - a) + th) * ((double)(k - 1 - bq) + th);
      tab[N * N + a * N + bq] = dl * dl * dl * dl * sacc;
    }
  for (int q = 0; q < 6; ++q) {
    for (int i = 0; i < N * N; ++i) K[q * N * N + i] = 2.0 * (c.w[q] * tab[N * N + i] + c.w[6 + q] * tab[i]);
    if (!invert_small(N, K + q * N * N, Ki + q * N * N)) return MPCQP_EINVAL;
  }
  if (NREC > 0 && !mpcqp_rowtab::lane_order_rows(N, WG<N>::G, rows)) return MPCQP_EINVAL;   // (a rule of N alone: holds for N = 10)
  for (int i = 0; i < NK; ++i) Ki32[i] = (float)Ki[i];
  lane_order_kinv<N>(Ki, Kl);
  for (int i = 0; i < NLANE; ++i) Kl32[i] = (float)Kl[i];   // (the same rounding of the same fp64 entries as Ki32)
  memcpy(img, Kl32, sizeof(float) * NLANE);
  memcpy(img + L32, Kl, sizeof(double) * NLANE);
  if (NREC > 0) {
    mpcqp_rowtab::pack_records<float>(NREC, Kl32, rows, img + sizeof(float) * NLANE);
    mpcqp_rowtab::pack_records<double>(NREC, Kl, rows, img + L32 + sizeof(double) * NLANE);
  }
  hipError_t he = upload(e->wr_K, K, sizeof(double) * NK);
  if (he == hipSuccess) he = upload(e->wr_kinv32, Ki32, sizeof(float) * NK);
  if (he == hipSuccess) he = upload(e->wr_kinv64, Ki, sizeof(double) * NK);
  if (he == hipSuccess) he = upload(e->wr_klane32, img, L32);
  if (he == hipSuccess) he = upload(e->wr_klane64, img + L32, L64);
  if (he == hipSuccess) return MPCQP_OK;
  (void)hipGetLastError();   // (what has been allocated stays with the handle: mpcqp_create frees it)
  return MPCQP_ENOMEM;
}

void free_engine(mpcqp_engine* h) {
  for (void* p : {(void*)h->dcfg, (void*)h->order_mem, (void*)h->dual_mem, (void*)h->model_mem, (void*)h->act_mem, (void*)h->dist_mem, h->dshift_mem, h->gait_mem, h->roll_mem,
                  (void*)h->plan_ws, (void*)h->wr_K, (void*)h->wr_kinv32, (void*)h->wr_kinv64, (void*)h->wr_klane32, (void*)h->wr_klane64,
                  (void*)h->stage_ws})
    if (p) (void)hipFree(p);
  for (hipEvent_t ev : {h->ev0, h->ev1})
    if (ev) (void)hipEventDestroy(ev);
  delete h;
}

// Roll-out arguments of the plant (mpcqp_rollout_plant); null for mpcqp_rollout, whose world step is x <- X[:,1].
struct RolloutPlantArgs { const void* body; const void* push; const int32_t* push_ticks; int n; };

PlantModel plant_model(const mpcqp_engine* h) {
  return {h->cfg.m, 1.0 / h->cfg.Ibody_inv[0], 1.0 / h->cfg.Ibody_inv[1], 1.0 / h->cfg.Ibody_inv[2]};
}

// The roll-out loop behind mpcqp_rollout, mpcqp_rollout_plant and mpcqp_rollout_phase: workspace reserved once, then 3 launches per
// tick on the caller's stream, no host synchronisation and no copies in between.  expand(tag, x, ref, w, it) launches the tick's expand
// kernel into the tuple workspace w, advance(tag, x, ref, o, it) the advance kernel on the results o; tag carries the I/O type.
// xc(tag) is the state the controller reads, the solve's x0 -- a buffer the expand fills inside the roll-out's reserve, which is why it
// is asked for after the reserve --, or null for x itself.
// The caller has made its checks; the device guard is here.  (mpcqp_last_kernel_ms after a roll-out: all T ticks)
struct ReadsPlant { template <typename TIO> const TIO* operator()(TIO) const { return nullptr; } };
template <typename Expand, typename Advance, typename Reads = ReadsPlant>
int rollout_loop(mpcqp_handle h, const char* who, int64_t B, int32_t T, void* x, void* ref, const void* mu, void* stream, Expand&& expand,
                 Advance&& advance, Reads&& xc = ReadsPlant()) {
  GUARD(h);
  if (reserve_workspace(h, B) != MPCQP_OK || reserve_gait(h, B) != MPCQP_OK || reserve_roll(h, B) != MPCQP_OK) {
    snprintf(h->err, sizeof(h->err), "%s: workspace allocation failed", who);
    return MPCQP_ENOMEM;
  }
  const int N = h->cfg.N;
  hipStream_t st = (hipStream_t)stream;
  return timed(h, st, "roll-out kernel launch", [&] { return with_io(h, [&](auto tag) {
    using TIO = decltype(tag);
    const TupleWs<TIO> w = tuple_ws<TIO>(h->gait_mem, B, N);
    const ResultWs<TIO> o = result_ws<TIO>(h->roll_mem, B, N);
    const TIO* xr = xc(tag);
    const FastIn<TIO> in = tuple_in<TIO>(h, xr ? (const void*)xr : x, w.r, w.contact, w.xdes, mu, o.u);
    TIO* xs = (TIO*)x;
    TIO* rf = (TIO*)ref;
    for (int it = 0; it < T; ++it) {
      expand(tag, xs, rf, w, it);
      hipError_t e = enqueue_solve<TIO>(h, B, in, o.u, o.X, o.status, o.iters, nullptr, st);
      if (e != hipSuccess) return e;
      advance(tag, xs, rf, o, it);
      e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }); });
}

// "Expand into the tuple workspace, then solve", behind the checks of mpcqp_solve_batch_gait_steps and mpcqp_solve_batch_phase: expand(tag, w)
// launches the expansion into the engine's tuple workspace w, the normal solve runs on that tuple; the timing covers both.
template <typename Expand>
int solve_expanded(mpcqp_handle h, int64_t B, const void* x0, const void* mu, void* u_out, void* X_out, int32_t* status, int32_t* iters,
                   float* res, hipStream_t st, const char* no_memory, const char* no_launch, Expand&& expand) {
  GUARD(h);
  if (reserve_workspace(h, B) != MPCQP_OK || reserve_gait(h, B) != MPCQP_OK) return fail(h, MPCQP_ENOMEM, no_memory);
  return timed(h, st, no_launch, [&] { return with_io(h, [&](auto tag) {
    using T = decltype(tag);
    const TupleWs<T> w = tuple_ws<T>(h->gait_mem, B, (size_t)h->cfg.N);
    expand(tag, w);
    return enqueue_solve<T>(h, B, tuple_in<T>(h, x0, w.r, w.contact, w.xdes, mu, u_out), (T*)u_out, (T*)X_out, status, iters, res, st);
  }); });
}

// The per-leg gait rows of include/mpcqp_plan.h as the phase kernels take them, and their expansion of B robots at (x, ref, tick) into w.
template <typename T>
PhaseRows<T> phase_rows(const void* feet, const int32_t* gait, const void* stand, const void* gain) {
  return {(const T*)feet, gait, (const T*)stand, (const T*)gain};
}
template <typename T>
void launch_phase_expand(const mpcqp_engine* h, int64_t B, hipStream_t st, const T* x, const T* ref, const PhaseRows<T>& ph, const int32_t* tick,
                         const TupleWs<T>& w) {
  hipLaunchKernelGGL((mpcqp_phase_expand_kernel<T>), expand_grid(B, h->cfg.N), dim3(256), 0, st, x, ref, ph, tick, h->cfg.delta, h->cfg.N, B, w.r,
                     w.contact, w.xdes);
}

template <typename TIO>
PlantIn<TIO> plant_in(const mpcqp_engine* h, const RolloutPlantArgs& p) {
  return {(const TIO*)p.body, (const TIO*)p.push, p.push_ticks, plant_model(h), p.n, h->cfg.delta / p.n};
}

// The roll-out on a plan table: mpcqp_rollout (plant = null) and mpcqp_rollout_plant.
int rollout_run(mpcqp_handle h, int64_t B, int32_t T, int32_t S, void* x, void* ref, const void* plan_pos, const uint8_t* plan_feet_id,
                const int32_t* plan_meta, int32_t* tick, const void* mu, void* actual, void* desired, void* forces, int32_t* solved,
                void* stream, const RolloutPlantArgs* plant) {
  const int N = h->cfg.N;
  const double d = h->cfg.delta;
  const dim3 ge = expand_grid(B, N), ga = advance_grid(B), nt(256);
  hipStream_t st = (hipStream_t)stream;
  return rollout_loop(h, "mpcqp_rollout", B, T, x, ref, mu, stream,
    [&](auto tag, auto* xs, auto* rf, const auto& w, int) {
      using TIO = decltype(tag);
      const RolloutPlan<TIO> plan = {(const TIO*)plan_pos, plan_feet_id, plan_meta};
      hipLaunchKernelGGL((mpcqp_rollout_expand_kernel<TIO>), ge, nt, 0, st, xs, rf, plan, tick, d, N, (int)S, B, w.r, w.contact, w.xdes);
    },
    [&](auto tag, auto* xs, auto* rf, const auto& o, int it) {
      using TIO = decltype(tag);
      const RolloutPlan<TIO> plan = {(const TIO*)plan_pos, plan_feet_id, plan_meta};
      if (plant) {
        hipLaunchKernelGGL((mpcqp_rollout_advance_kernel<TIO, PlantIn<TIO>>), ga, nt, 0, st, xs, rf, plan, tick, plant_in<TIO>(h, *plant), o.u,
                           o.status, d, N, B, (int)T, it, (int)S, (TIO*)actual, (TIO*)desired, (TIO*)forces, solved);
      } else {
        const ModelWorld<TIO> world = {o.X};
        hipLaunchKernelGGL((mpcqp_rollout_advance_kernel<TIO, ModelWorld<TIO>>), ga, nt, 0, st, xs, rf, plan, tick, world, o.u, o.status, d, N, B,
                           (int)T, it, (int)S, (TIO*)actual, (TIO*)desired, (TIO*)forces, solved);
      }
    });
}

// substeps of include/mpcqp_sim.h: 0 means the default, [1, 1000] as given; -1 for out of range
int plant_substeps(int32_t substeps) {
  if (substeps < 0 || substeps > PLANT_MAX_SUBSTEPS) return -1;
  return substeps == 0 ? PLANT_DEFAULT_SUBSTEPS : substeps;
}

// leg_substeps / substeps of include/mpcqp_joints.h for a tick of `delta`: as given, or for 0 the default control period, the fewest
// periods of at most SWING_H0 (the caller has checked the range [0, SWING_MAX_SUBSTEPS])
int swing_substeps(double delta, int32_t substeps) {
  if (substeps != 0) return substeps;
  int n = (int)std::ceil(delta / SWING_H0);
  while (n > 1 && delta / (n - 1) <= SWING_H0) --n;   // (delta / h0 a whole number up to rounding)
  return n < 1 ? 1 : (n > SWING_MAX_SUBSTEPS ? SWING_MAX_SUBSTEPS : n);
}

// One launch, 256 threads a block, of a kernel whose last template argument is the actuator pack (act_rows, mpcqp_actuators.h): `k` = K<TIO>
// on `args` without a table, `ka` = K<TIO, double> on (args..., the table) with one.  A handle with a table runs the instantiations that
// read it; without one, the kernels are what they were.
template <typename... P, typename... A>
void launch_act(const mpcqp_engine* h, dim3 grid, hipStream_t st, void (*k)(P...), void (*ka)(P..., const double*), const A&... args) {
  if (const double* act = act_table(h)) hipLaunchKernelGGL(ka, grid, dim3(256), 0, st, args..., act);
  else hipLaunchKernelGGL(k, grid, dim3(256), 0, st, args...);
}

// The leg geometry of a call (null = the Lite3's) as the kernels take it, or the text of what does not fit.  closed_form: the geometry of
// include/mpcqp_joints.h, a HipX joint about +-e_x followed by a planar chain about +-e_y; otherwise as mpcqp_leg_jacobians takes it, any
// chain with non-zero joint axes.  g gets unit axes either way.
int leg_geometry(mpcqp_handle h, const char* who, const MpcQpLegGeometry* geo, bool closed_form, LegGeoDev& g) {
  MpcQpLegGeometry lite3;
  if (!geo) { (void)mpcqp_default_leg_geometry(&lite3); geo = &lite3; }
  if (geo->size != sizeof(MpcQpLegGeometry)) return bad(h, who, "geometry struct size mismatch");
  memcpy(g.hx, geo->hip_x, sizeof(g.hx)); memcpy(g.hy, geo->hip_y, sizeof(g.hy));
  memcpy(g.kn, geo->knee, sizeof(g.kn)); memcpy(g.ft, geo->foot, sizeof(g.ft));
  if (!closed_form) {
    for (int k = 0; k < 2; ++k) {   // unit axes (Rodrigues' formula assumes them)
      const double* a = k ? geo->axis_y : geo->axis_x;
      const double nrm = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
      if (!(nrm > 0) || !std::isfinite(nrm)) return bad(h, who, "zero joint axis");
      for (int c = 0; c < 3; ++c) (k ? g.ay : g.ax)[c] = a[c] / nrm;
    }
    return MPCQP_OK;
  }
  const char* field = nullptr;
  const auto fin3 = [](const double* a) { return std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]); };
  if (!fin3(geo->axis_x) || geo->axis_x[0] == 0.0 || geo->axis_x[1] != 0.0 || geo->axis_x[2] != 0.0) field = "axis_x is not +-e_x";
  else if (!fin3(geo->axis_y) || geo->axis_y[1] == 0.0 || geo->axis_y[0] != 0.0 || geo->axis_y[2] != 0.0) field = "axis_y is not +-e_y";
  else if (!fin3(geo->knee) || geo->knee[0] != 0.0 || geo->knee[1] != 0.0 || !(geo->knee[2] < 0.0)) field = "knee is not (0, 0, -l1), l1 > 0";
  else if (!fin3(geo->foot) || geo->foot[0] != 0.0 || geo->foot[1] != 0.0 || !(geo->foot[2] < 0.0)) field = "foot is not (0, 0, -l2), l2 > 0";
  for (int l = 0; l < 4 && !field; ++l) {
    if (!fin3(geo->hip_y[l]) || geo->hip_y[l][0] != 0.0 || geo->hip_y[l][2] != 0.0) field = "hip_y is not (0, d, 0)";
    else if (!fin3(geo->hip_x[l])) field = "hip_x is not finite";
  }
  if (field) return bad(h, who, "the closed form needs the Lite3's leg structure: ", field);
  for (int c = 0; c < 3; ++c) { g.ax[c] = 0.0; g.ay[c] = 0.0; }
  g.ax[0] = geo->axis_x[0] > 0.0 ? 1.0 : -1.0;
  g.ay[1] = geo->axis_y[1] > 0.0 ? 1.0 : -1.0;
  return MPCQP_OK;
}

// The inertial row of include/mpcqp_joints.h (null = the Lite3's): fills r or names the field that is not valid.
int leg_inertia_row(mpcqp_handle h, const char* who, const MpcQpLegInertia* inr, LegInrDev& r) {
  MpcQpLegInertia lite3;
  if (!inr) { (void)mpcqp_default_leg_inertia(&lite3); inr = &lite3; }
  if (inr->size != sizeof(MpcQpLegInertia)) return bad(h, who, "inertia struct size mismatch");
  const char* field = nullptr;
  const auto fin = [](const double* a, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false; return true; };
  if (!fin(&inr->mass[0][0], 12)) field = "mass is not finite";
  else if (!fin(&inr->com[0][0][0], 36)) field = "com is not finite";
  else if (!fin(&inr->inertia[0][0][0], 72)) field = "inertia is not finite";
  else if (!fin(inr->q_min, 3)) field = "q_min is not finite";
  else if (!fin(inr->q_max, 3)) field = "q_max is not finite";
  else if (!fin(inr->qd_max, 3)) field = "qd_max is not finite";
  else if (!fin(inr->tau_max, 3)) field = "tau_max is not finite";
  else if (!std::isfinite(inr->gravity) || !(inr->gravity < 0.0)) field = "gravity is not negative and finite";
  for (int i = 0; i < 12 && !field; ++i) if ((&inr->mass[0][0])[i] < 0.0) field = "mass is negative";
  for (int j = 0; j < 3 && !field; ++j) {
    if (inr->q_min[j] > inr->q_max[j]) field = "q_min > q_max";
    else if (inr->qd_max[j] < 0.0) field = "qd_max is negative";
    else if (inr->tau_max[j] < 0.0) field = "tau_max is negative";
  }
  if (field) return bad(h, who, "invalid leg inertia row: ", field);
  LegLinkInr* link[3] = {&r.k0, &r.k1, &r.k2};
  for (int l = 0; l < 4; ++l)
    for (int k = 0; k < 3; ++k) {
      link[k]->m[l] = inr->mass[l][k];
      memcpy(link[k]->c[l], inr->com[l][k], sizeof(link[k]->c[l]));
      memcpy(link[k]->I[l], inr->inertia[l][k], sizeof(link[k]->I[l]));
    }
  memcpy(r.lim.qmin, inr->q_min, sizeof(r.lim.qmin)); memcpy(r.lim.qmax, inr->q_max, sizeof(r.lim.qmax));
  memcpy(r.lim.qdmax, inr->qd_max, sizeof(r.lim.qdmax)); memcpy(r.lim.taumax, inr->tau_max, sizeof(r.lim.taumax));
  r.lim.g = inr->gravity;
  return MPCQP_OK;
}

// The two rows of a leg call in the order every entry point checks them: the geometry, then the inertia.
int leg_rows(mpcqp_handle h, const char* who, const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, bool closed_form, LegGeoDev& g,
             LegInrDev& r) {
  if (const int rc = leg_geometry(h, who, geo, closed_form, g)) return rc;
  return leg_inertia_row(h, who, inr, r);
}

// What mpcqp_rollout_drive adds to mpcqp_rollout_legs: the drive mode, the ground's friction [B] or null, the commanded-force log or null.
struct RolloutDriveArgs { int32_t drive; const void* ground; void* cmd_log; };
// What mpcqp_rollout_slip adds to mpcqp_rollout_drive: the feet's effective mass [B], the slip state [B,4,2], its two logs or null.
struct RolloutSlipArgs { const void* foot_mass; double* slip; double* slip_log; void* disp_log; };
// What mpcqp_rollout_observe adds to mpcqp_rollout_slip: what the MPC reads, the filter state [B,131], the optional operands of the
// sensors and the filter, the checked parameters, the seven logs or null; for mpcqp_rollout_observe_gated the checked thresholds (null: no
// gate) and the trust log or null; for mpcqp_rollout_observe_aided the checked gains (null: not aided), att_state [B,8] and the bias log
// or null.
struct RolloutObserveArgs {
  int32_t feed; double* est_state; const void *est_init, *height, *bias, *noise, *enc_noise; EstPar par;
  void *imu_log, *q_enc_log, *qd_enc_log, *est_log, *feet_est_log, *sigma_log, *nis_log;
  const EstGate* gate; void* trust_log;
  const EstAid* aid; double* att_state; void* bias_log;
};
// What mpcqp_rollout_observe_compensated adds to mpcqp_rollout_observe (include/mpcqp_compensate.h): where the observer reads, the ticks
// between two table updates, the checked observer parameters, the body it believes or null, its state [B,40] and its two logs or null.
struct RolloutCompensateArgs { int32_t source, hold; DistPar par; const void* obs_body; double* dist_state; void *dist_log, *resid_log; };

// The table a compensated roll-out begins with: B rows from dist_state[:,0:6], set as mpcqp_set_disturbance sets its rows.
int compensate_enter(mpcqp_handle h, const char* who, int64_t B, const double* dist_state, hipStream_t st) {
  GUARD(h);
  if (const int rc = reserve_disturbance(h, B, who)) return rc;
  with_io(h, [&](auto tag) {
    hipLaunchKernelGGL((mpcqp_compensate_enter_kernel<decltype(tag)>), blocks(B), dim3(256), 0, st, dist_state, h->dist_mem, B);
  });
  const int rc = launched(h, "compensate table kernel launch");
  h->dist_B = rc == MPCQP_OK ? B : 0;
  return rc;
}

// mpcqp_rollout_legs (dr = null), mpcqp_rollout_drive, mpcqp_rollout_slip (sl, with dr), mpcqp_rollout_observe (ob, with both) and
// mpcqp_rollout_observe_compensated (cp, with all three): one argument check, one loop.
int rollout_legs_run(mpcqp_handle h, const char* who, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                     const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                     const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains, int32_t leg_substeps,
                     const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, void* actual, void* desired, void* forces,
                     void* feet_log, uint8_t* contact_log, int32_t* solved, void* swing_log, void* q_log, void* qd_log, void* tau_log,
                     void* foot_log, void* err_log, uint8_t* flag_log, void* miss_log, void* stream, const RolloutDriveArgs* dr,
                     const RolloutSlipArgs* sl = nullptr, const RolloutObserveArgs* ob = nullptr,
                     const RolloutCompensateArgs* cp = nullptr) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || B * (int64_t)T > 0x7fffffff) return bad(h, who, "size out of range");
  const int n = plant_substeps(substeps);
  if (n < 0) return bad(h, who, "substeps out of range [0, 1000]");
  if (leg_substeps < 0 || leg_substeps > SWING_MAX_SUBSTEPS) return bad(h, who, "leg_substeps out of range [0, 1000]");
  if (land != MPCQP_LAND_RULE && land != MPCQP_LAND_ACTUAL) return bad(h, who, "land is neither MPCQP_LAND_RULE nor MPCQP_LAND_ACTUAL");
  if (dr && dr->drive != MPCQP_DRIVE_IDEAL && dr->drive != MPCQP_DRIVE_LIMITED)
    return bad(h, who, "drive is neither MPCQP_DRIVE_IDEAL nor MPCQP_DRIVE_LIMITED");
  if (push && !push_ticks) return bad(h, who, "push without push_ticks");
  if (B > 0 && (!x || !ref || !feet || !legs || !gait || !stand || !tick || !mu || !step_height)) return bad(h, who, "null buffer");
  if (B > 0 && sl && (!dr->ground || !sl->foot_mass || !sl->slip)) return bad(h, who, "null buffer");
  if (B > 0 && ob && !ob->est_state) return bad(h, who, "null buffer");
  if (B > 0 && ob && ob->aid && !ob->att_state) return bad(h, who, "null att_state buffer");
  if (B > 0 && cp && !cp->dist_state) return bad(h, who, "null dist_state buffer");
  LegGeoDev g;
  LegInrDev r;
  if (const int rc = leg_rows(h, who, geo, inr, true, g, r)) return rc;
  if (B == 0 || T == 0) return MPCQP_OK;
  if (cp) {   // the call sets the disturbance table itself, once the other tables have passed: a call that is refused leaves it alone
    if (const int rc = table_match(h, models(h), "model", B, who)) return rc;
    if (const int rc = actuators_match(h, B, who)) return rc;
    if (const int rc = compensate_enter(h, who, B, cp->dist_state, (hipStream_t)stream)) return rc;
  }
  if (const int rc = solve_tables_match(h, B, who)) return rc;
  if (const int rc = actuators_match(h, B, who)) return rc;
  const int nl = swing_substeps(h->cfg.delta, leg_substeps);
  const RolloutPlantArgs plant = {body, push, push ? push_ticks : nullptr, n};
  const int N = h->cfg.N;
  const double d = h->cfg.delta;
  const dim3 ga = advance_grid(B), gl = leg_grid(B), nt(256);
  hipStream_t st = (hipStream_t)stream;
  // the roll-out loop of mpcqp_rollout_phase with the legs step in front of its advance and the landing behind it: 5 launches per tick.
  // With a drive, the rule runs between the solve and the legs step and leaves the applied forces in a [B,12] side buffer, which the legs
  // step and the advance read as a force buffer of horizon 1 (the solve's own buffer, its next warm start, is not altered); after the legs
  // step the rule's torques and bits go into the stance rows of tau_log / flag_log: 6 launches, 7 with one of those two logs.
  // With the slip rule in the drive's place the log step waits until after the landing and moves the feet in the same launch: 7.
  // With the estimator (ob) its update runs in front of the expand and its predict between the slip rule and the legs step: 9; with
  // MPCQP_FEED_ESTIMATE the expand and the solve read the update's side buffers in place of x and feet.
  // With the wrench observer (cp) its tick kernel runs in front of the advance, while x and feet are still the tick's: 10, the shift and
  // add-back kernels of the table it keeps not counted (they are the solve's).
  const auto observe_in = [&](auto tag) {
    using TIO = decltype(tag);
    return ObsIn<TIO>{(const TIO*)ob->est_init, (const TIO*)ob->height, (const TIO*)ob->bias, (const TIO*)ob->noise, (const TIO*)ob->enc_noise};
  };
  const auto observe_out = [&](auto tag) {
    using TIO = decltype(tag);
    return ObsOut<TIO>{(TIO*)ob->imu_log, (TIO*)ob->q_enc_log, (TIO*)ob->qd_enc_log, (TIO*)ob->est_log, (TIO*)ob->feet_est_log,
                       (TIO*)ob->sigma_log, (TIO*)ob->nis_log};
  };
  const bool fed = ob && ob->feed == MPCQP_FEED_ESTIMATE;
  return rollout_loop(h, who, B, T, x, ref, mu, stream,
    [&](auto tag, auto* xs, auto* rf, const auto& w, int it) {
      using TIO = decltype(tag);
      if (!ob) return launch_phase_expand<TIO>(h, B, st, xs, rf, phase_rows<TIO>(feet, gait, stand, gain), tick, w);
      const ObsWs<TIO> ow = observe_ws<TIO>(h->roll_mem, B, N);
      const auto update = ob->aid ? (ob->gate ? mpcqp_observe_update_kernel<TIO, true, true> : mpcqp_observe_update_kernel<TIO, false, true>)
                                  : (ob->gate ? mpcqp_observe_update_kernel<TIO, true> : mpcqp_observe_update_kernel<TIO, false>);
      hipLaunchKernelGGL(update, gl, nt, 0, st, (const TIO*)xs, (const TIO*)rf, phase_rows<TIO>(feet, gait, stand, gain),
                         (const int32_t*)tick, (const double*)sl->slip, (const double*)legs, (const TIO*)step_height, observe_in(tag), ob->par, g,
                         ob->est_state, ow, observe_out(tag), d, B, (int)T, it, ob->gate ? *ob->gate : EstGate{}, (TIO*)ob->trust_log,
                         ob->aid ? *ob->aid : EstAid{}, ob->att_state, (TIO*)ob->bias_log);
      launch_phase_expand<TIO>(h, B, st, fed ? (const TIO*)ow.xhat : (const TIO*)xs, rf, phase_rows<TIO>(fed ? (void*)ow.feet : feet, gait, stand, gain),
                               tick, w);
    },
    [&](auto tag, auto* xs, auto* rf, const auto& o, int it) {
      using TIO = decltype(tag);
      const PhaseRows<TIO> ph = phase_rows<TIO>(feet, gait, stand, gain);
      const LegRollOut<TIO> out = {(TIO*)swing_log, (TIO*)q_log, (TIO*)qd_log, (TIO*)tau_log, (TIO*)foot_log, (TIO*)err_log, flag_log};
      const TIO* u = o.u;   // the forces the legs and the plant see, robot b's at u + b Nu 12
      int Nu = N;
      const DriveWs<TIO> dw = drive_ws<TIO>(h->roll_mem, B, N);
      TIO* const rdisp = sl ? slip_ws<TIO>(h->roll_mem, B, N) : nullptr;
      if (sl) {
        TIO* cmd = dr->cmd_log ? (TIO*)dr->cmd_log + (size_t)it * 12 : nullptr;
        double* slog = sl->slip_log ? sl->slip_log + (size_t)it * 8 : nullptr;
        launch_act(h, gl, st, mpcqp_stance_slip_kernel<TIO>, mpcqp_stance_slip_kernel<TIO, double>, xs, o.u, (int64_t)N * 12,
                   (const TIO*)feet, (const uint8_t*)nullptr, gait, tick, (const TIO*)dr->ground, (const TIO*)sl->foot_mass,
                   (const double*)sl->slip, g, r.lim, (int)dr->drive, n, d / n, d, dw.f, dw.tau, dw.flag, cmd, (int64_t)T * 12, sl->slip, rdisp,
                   slog, (int64_t)T * 8, B);
        u = dw.f; Nu = 1;
        if (ob) {
          const auto predict = ob->aid ? mpcqp_observe_predict_kernel<TIO, true> : mpcqp_observe_predict_kernel<TIO, false>;
          hipLaunchKernelGGL(predict, gl, nt, 0, st, (const TIO*)xs, (const int32_t*)tick, u, plant_in<TIO>(h, plant), observe_in(tag), ob->par,
                             ob->est_state, observe_ws<TIO>(h->roll_mem, B, N), observe_out(tag), B, (int)T, it,
                             ob->aid ? *ob->aid : EstAid{}, ob->att_state, (TIO*)ob->bias_log);
        }
      } else if (dr) {
        TIO* cmd = dr->cmd_log ? (TIO*)dr->cmd_log + (size_t)it * 12 : nullptr;
        launch_act(h, gl, st, mpcqp_stance_drive_kernel<TIO>, mpcqp_stance_drive_kernel<TIO, double>, xs, o.u, (int64_t)N * 12,
                   (const TIO*)feet, (const uint8_t*)nullptr, gait, tick, (const TIO*)dr->ground, g, r.lim, (int)dr->drive, dw.f, dw.tau, dw.flag,
                   cmd, (int64_t)T * 12, B);
        u = dw.f; Nu = 1;
      }
      launch_act(h, gl, st, mpcqp_legs_step_kernel<TIO>, mpcqp_legs_step_kernel<TIO, double>, xs, rf, ph, tick, u, (const TIO*)step_height,
                 (const TIO*)gains, legs, plant_in<TIO>(h, plant), g, r.k0, r.k1, r.k2, r.lim, out, d, Nu, B, (int)T, it, nl, d / nl);
      if (dr && !sl && (tau_log || flag_log))
        hipLaunchKernelGGL((mpcqp_drive_log_kernel<TIO>), gl, nt, 0, st, gait, tick, dw.tau, dw.flag,
                           (int)(dr->drive == MPCQP_DRIVE_IDEAL && !dr->ground), B, (int)T, it, (TIO*)tau_log, flag_log);
      if (cp) {   // the observer's row on the tick's operands and, every `hold` ticks and on the last, the robot's table row
        const bool sensed = cp->source == MPCQP_WRENCH_SENSED, update = (it + 1) % cp->hold == 0 || it == T - 1;
        const ObsWs<TIO> ow = observe_ws<TIO>(h->roll_mem, B, N);
        hipLaunchKernelGGL((mpcqp_compensate_tick_kernel<TIO>), ga, nt, 0, st, sensed ? (const TIO*)ow.xhat : (const TIO*)xs,
                           sensed ? (const TIO*)o.u : u, sensed ? (int64_t)N * 12 : (int64_t)Nu * 12, sensed ? (const TIO*)ow.feet : (const TIO*)feet,
                           sensed ? (const double*)ob->est_state : (const double*)nullptr, (const TIO*)cp->obs_body, plant_model(h), cp->par,
                           cp->dist_state, h->dist_mem, (TIO*)cp->dist_log, (TIO*)cp->resid_log, B, (int)T, it, update);
      }
      hipLaunchKernelGGL((mpcqp_phase_advance_kernel<TIO>), ga, nt, 0, st, xs, rf, (TIO*)feet, ph, tick, plant_in<TIO>(h, plant), u, o.status, d, Nu, B,
                         (int)T, it, (TIO*)actual, (TIO*)desired, (TIO*)forces, (TIO*)feet_log, contact_log, solved);
      hipLaunchKernelGGL((mpcqp_legs_land_kernel<TIO>), gl, nt, 0, st, xs, (TIO*)feet, gait, tick, legs, g, (int)land, B, (int)T, it,
                         (TIO*)miss_log);
      if (sl)
        hipLaunchKernelGGL((mpcqp_slip_finish_kernel<TIO>), gl, nt, 0, st, gait, tick, (const TIO*)dw.tau, (const uint8_t*)dw.flag,
                           (const TIO*)rdisp, B, (int)T, it, (TIO*)feet, sl->slip, (TIO*)tau_log, flag_log, (TIO*)sl->disp_log);
    },
    [&](auto tag) {
      using TIO = decltype(tag);
      return fed ? (const TIO*)observe_ws<TIO>(h->roll_mem, B, N).xhat : (const TIO*)nullptr;
    });
}

// The estimator's parameters of an entry point `who` (null: the defaults), checked and with the handle's delta.
int estimator_row(mpcqp_handle h, const char* who, const MpcQpEstimator* par, EstPar& e) {
  MpcQpEstimator dflt;
  if (!par) { (void)mpcqp_default_estimator(&dflt); par = &dflt; }
  if (par->size != sizeof(MpcQpEstimator)) return bad(h, who, "estimator struct size mismatch");
  const double nn[11] = {par->kappa, par->q_p, par->q_v, par->q_f, par->r_p, par->r_v, par->r_z, par->k_swing, par->p0_p, par->p0_v, par->p0_f};
  if (!std::isfinite(par->gravity) || !(par->gravity < 0)) return bad(h, who, "estimator: gravity must be finite and negative");
  for (const double v : nn)
    if (!std::isfinite(v) || !(v >= 0)) return bad(h, who, "estimator: kappa, q_*, r_*, k_swing and p0_* must be finite and non-negative");
  const double d = h->cfg.delta;
  e = {par->gravity, par->kappa, par->q_p, par->q_v, par->q_f, par->r_p, par->r_v, par->r_z, par->k_swing, par->p0_p, par->p0_v, par->p0_f,
       d, 0.5 * d * d};
  return MPCQP_OK;
}

// The gate's thresholds of an entry point `who` (null: the defaults), checked.
int gate_row(mpcqp_handle h, const char* who, const MpcQpTrustGate* gate, EstGate& e) {
  MpcQpTrustGate dflt;
  if (!gate) { (void)mpcqp_default_trust_gate(&dflt); gate = &dflt; }
  if (gate->size != sizeof(MpcQpTrustGate)) return bad(h, who, "trust gate struct size mismatch");
  if (!std::isfinite(gate->d_lo) || !std::isfinite(gate->d_hi) || !(gate->d_lo >= 0) || !(gate->d_hi > gate->d_lo))
    return bad(h, who, "trust gate: d_lo and d_hi must be finite with 0 <= d_lo < d_hi");
  e = {gate->d_lo, gate->d_hi, gate->d_hi - gate->d_lo};
  return MPCQP_OK;
}

// The aided rule's gains of an entry point `who` (null: the defaults) and its flags, checked, with the estimator's checked row e.
int attitude_row(mpcqp_handle h, const char* who, int32_t flags, const MpcQpAttitude* att, const EstPar& e, EstAid& a) {
  MpcQpAttitude dflt;
  if (!att) { (void)mpcqp_default_attitude(&dflt); att = &dflt; }
  if (flags & ~MPCQP_AIDED_GATE) return bad(h, who, "flags has a bit other than MPCQP_AIDED_GATE");
  if (att->size != sizeof(MpcQpAttitude)) return bad(h, who, "attitude struct size mismatch");
  for (const double v : {att->k_s, att->k_v, att->k_b, att->b_max})
    if (!std::isfinite(v) || !(v >= 0)) return bad(h, who, "attitude: k_s, k_v, k_b and b_max must be finite and non-negative");
  a = {att->k_s, att->k_v, att->k_b * e.d, att->b_max, e.d * std::fabs(e.g)};
  return MPCQP_OK;
}

// The wrench observer's parameters of include/mpcqp_disturb.h (null: the defaults), checked and with the handle's delta.
int observer_row(mpcqp_handle h, const char* who, const MpcQpWrenchObserver* par, DistPar& e) {
  MpcQpWrenchObserver dflt;
  if (!par) { (void)mpcqp_default_wrench_observer(&dflt); par = &dflt; }
  if (par->size != sizeof(MpcQpWrenchObserver)) return bad(h, who, "wrench observer struct size mismatch");
  if (!std::isfinite(par->gravity) || !(par->gravity < 0)) return bad(h, who, "wrench observer: gravity must be finite and negative");
  if (!(par->kappa >= 0 && par->kappa <= 1)) return bad(h, who, "wrench observer: kappa must be in [0, 1]");
  if (!(par->f_lim >= 0) || !(par->t_lim >= 0)) return bad(h, who, "wrench observer: f_lim and t_lim must be non-negative (infinity: no clamp)");
  e = {par->gravity, par->kappa, par->f_lim, par->t_lim, h->cfg.delta};
  return MPCQP_OK;
}

// What mpcqp_estimate_track_aided adds to mpcqp_estimate_track_gated.
struct EstimateAidedArgs { int32_t flags; const MpcQpAttitude* att; double* att_state; void* bias_log; };

// mpcqp_estimate_track (gated = false: no gate, no trust_out), mpcqp_estimate_track_gated and mpcqp_estimate_track_aided (ad: whether
// the gate runs is its flags'): one argument check, one launch each.
int estimate_track_run(mpcqp_handle h, const char* who, int64_t B, int32_t T, const void* imu, const void* q, const void* qd,
                       const uint8_t* contact_log, const void* trust, const void* height, const void* init, const MpcQpEstimator* par,
                       const MpcQpLegGeometry* geo, double* state, void* est, void* feet_est, void* sigma, void* nis, bool gated,
                       const MpcQpTrustGate* gate, void* trust_out, void* stream, const EstimateAidedArgs* ad = nullptr) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || B * (int64_t)T > 0x1fffffff) return bad(h, who, "size out of range");
  if (!est && !feet_est && !sigma && !nis && !trust_out && !(ad && ad->bias_log))
    return bad(h, who, ad      ? "no output buffer (est, feet_est, sigma, nis, trust_out and bias_log are all null)"
                       : gated ? "no output buffer (est, feet_est, sigma, nis and trust_out are all null)"
                               : "no output buffer (est, feet_est, sigma and nis are all null)");
  if (B > 0 && T > 0 && (!imu || !q || !qd)) return bad(h, who, "null buffer (imu, q, qd)");
  if (B > 0 && T > 0 && !init) return bad(h, who, "null init buffer");
  if (B > 0 && T > 0 && !trust && !contact_log) return bad(h, who, "null contact_log buffer without trust");
  EstPar e;
  if (const int rc = estimator_row(h, who, par, e)) return rc;
  EstGate eg = {};
  EstAid ea = {};
  if (ad) {
    if (const int rc = attitude_row(h, who, ad->flags, ad->att, e, ea)) return rc;
    gated = (ad->flags & MPCQP_AIDED_GATE) != 0;
  }
  if (gated)
    if (const int rc = gate_row(h, who, gate, eg)) return rc;
  LegGeoDev g;
  if (const int rc = leg_geometry(h, who, geo, false, g)) return rc;
  if (B == 0 || T == 0) return MPCQP_OK;
  const char* what = ad ? "aided estimate track kernel launch" : (gated ? "gated estimate track kernel launch" : "estimate track kernel launch");
  return on_device(h, what, [&](auto tag) {
    using TIO = decltype(tag);
    const auto track = ad ? (gated ? mpcqp_estimate_track_kernel<TIO, true, true> : mpcqp_estimate_track_kernel<TIO, false, true>)
                          : (gated ? mpcqp_estimate_track_kernel<TIO, true> : mpcqp_estimate_track_kernel<TIO, false>);
    hipLaunchKernelGGL(track, leg_grid(B), dim3(256), 0, (hipStream_t)stream, (const TIO*)imu, (const TIO*)q, (const TIO*)qd, contact_log,
                       (const TIO*)trust, (const TIO*)height, (const TIO*)init, e, g, state, (TIO*)est, (TIO*)feet_est, (TIO*)sigma,
                       (TIO*)nis, B, (int)T, eg, (TIO*)trust_out, ea, ad ? ad->att_state : nullptr, (TIO*)(ad ? ad->bias_log : nullptr));
  });
}

// The slip roll-out's arguments as mpcqp_rollout_slip, _observe and _observe_gated take them, in their order.
struct RolloutSlipCall {
  int64_t B; int32_t T; void *x, *ref, *feet; double* legs; const int32_t* gait; const void *stand, *gain; int32_t* tick;
  const void *mu, *body, *push; const int32_t* push_ticks; int32_t substeps; const void *step_height, *gains; int32_t leg_substeps;
  const MpcQpLegGeometry* geo; const MpcQpLegInertia* inr; int32_t land, drive; const void *ground, *foot_mass; double* slip;
  void *actual, *desired, *forces, *feet_log; uint8_t* contact_log; int32_t* solved; void *swing_log, *q_log, *qd_log, *tau_log, *foot_log,
      *err_log; uint8_t* flag_log; void *miss_log, *cmd_log; double* slip_log; void* disp_log;
};

// mpcqp_rollout_observe (gated = false), mpcqp_rollout_observe_gated and mpcqp_rollout_observe_aided (ad: whether the gate runs is its
// flags'): the checks of what they add to mpcqp_rollout_slip, then its loop.  cp: the checked arguments of
// mpcqp_rollout_observe_compensated, which runs one of the three with the wrench observer in the loop.
int rollout_observe_run(mpcqp_handle h, const char* who, const RolloutSlipCall& c, int32_t feed, double* est_state, const void* est_init,
                        const void* height, const void* bias, const void* noise, const void* enc_noise, const MpcQpEstimator* par,
                        void* imu_log, void* q_enc_log, void* qd_enc_log, void* est_log, void* feet_est_log, void* sigma_log, void* nis_log,
                        bool gated, const MpcQpTrustGate* gate, void* trust_log, void* stream, const EstimateAidedArgs* ad = nullptr,
                        const RolloutCompensateArgs* cp = nullptr) {
  if (!h) return MPCQP_EINVAL;
  if (feed != MPCQP_FEED_TRUTH && feed != MPCQP_FEED_ESTIMATE) return bad(h, who, "feed is neither MPCQP_FEED_TRUTH nor MPCQP_FEED_ESTIMATE");
  RolloutObserveArgs ob = {feed, est_state, est_init, height, bias, noise, enc_noise, {}, imu_log, q_enc_log, qd_enc_log, est_log, feet_est_log,
                           sigma_log, nis_log, nullptr, trust_log, nullptr, nullptr, nullptr};
  if (const int rc = estimator_row(h, who, par, ob.par)) return rc;
  EstAid ea = {};
  if (ad) {
    if (const int rc = attitude_row(h, who, ad->flags, ad->att, ob.par, ea)) return rc;
    gated = (ad->flags & MPCQP_AIDED_GATE) != 0;
    ob.aid = &ea; ob.att_state = ad->att_state; ob.bias_log = ad->bias_log;
  }
  EstGate eg = {};
  if (gated) {
    if (const int rc = gate_row(h, who, gate, eg)) return rc;
    ob.gate = &eg;
  }
  const RolloutDriveArgs dr = {c.drive, c.ground, c.cmd_log};
  const RolloutSlipArgs sl = {c.foot_mass, c.slip, c.slip_log, c.disp_log};
  return rollout_legs_run(h, who, c.B, c.T, c.x, c.ref, c.feet, c.legs, c.gait, c.stand, c.gain, c.tick, c.mu, c.body, c.push, c.push_ticks,
                          c.substeps, c.step_height, c.gains, c.leg_substeps, c.geo, c.inr, c.land, c.actual, c.desired, c.forces, c.feet_log,
                          c.contact_log, c.solved, c.swing_log, c.q_log, c.qd_log, c.tau_log, c.foot_log, c.err_log, c.flag_log, c.miss_log,
                          stream, &dr, &sl, &ob, cp);
}

}  // namespace

extern "C" {

uint32_t mpcqp_version(void) { return MPCQP_VERSION; }

int mpcqp_default_config(MpcQpConfig* c) {
  if (!c) return MPCQP_EINVAL;
  memset(c, 0, sizeof(*c));
  c->size = (uint32_t)sizeof(*c);
  c->N = 10;
  c->delta = 0.03;
  c->m = 8.885;                                                               // src/mpc.py:71
  c->Ibody_inv[0] = 1.0 / 0.24; c->Ibody_inv[1] = 1.0; c->Ibody_inv[2] = 1.0; // src/mpc.py:73-76
  const double w[13] = {1e4, 2.7e4, 1e4, 2.7e5, 2.7e5, 2.7e5, 1e4, 1e4, 1e4, 1.6e4, 1.6e4, 1.6e4, 0.0};
  memcpy(c->w, w, sizeof(w));                                                 // src/mpc.py:122-134
  c->alpha = 1e-2;           // benchmark default; the reference's 0.0 (src/mpc.py:121) leaves the GRFs non-unique
  c->f_min = 3.0; c->f_max = 100.0;                                           // src/mpc.py:45-46
  c->disc = MPCQP_DISC_EULER;                                                 // src/mpc.py:117
  c->dtype = MPCQP_DTYPE_F32;
  c->precision = MPCQP_PREC_MIXED;
  c->flags = MPCQP_FLAG_POLISH;
  c->rho = 1.0; c->sigma = 1e-6; c->relax = 1.6;
  c->max_iter = 400; c->check_every = 100;   // tuned on MI355X: longer ADMM blocks save polish sweeps (profiles/r01_knob_sweep.txt)
  c->eps_abs = 1e-5; c->eps_rel = 1e-6;
  c->polish_max = 4;
  c->device = 0;
  return MPCQP_OK;
}

int mpcqp_create(const MpcQpConfig* cfg, mpcqp_handle* out) {
  if (!cfg || !out || cfg->size != sizeof(MpcQpConfig)) return MPCQP_EINVAL;
  *out = nullptr;
  if (!config_valid(*cfg)) return MPCQP_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) return MPCQP_ENODEV;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return MPCQP_ENODEV;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return MPCQP_ENODEV;  // gfx950 code objects only
  DeviceGuard guard(cfg->device);            // the caller's current device is restored on return
  if (guard.err != hipSuccess) return MPCQP_EHIP;

  mpcqp_engine* e = new (std::nothrow) mpcqp_engine();
  if (!e) return MPCQP_ENOMEM;
  auto reject = [&](int code) { free_engine(e); return code; };
  e->err[0] = 0;
  e->cfg = *cfg;
  // MPCQP_PREC_F32 (everything fp32) was the arithmetic of the round-1 kernels; it held a 2e-2 band at horizon 10 and none at 20.  The
  // request is served with MIXED (fp32 tiles / chains, fp64 residuals and polish), which is no slower and meets the 1e-4 band.
  if (e->cfg.precision == MPCQP_PREC_F32) e->cfg.precision = MPCQP_PREC_MIXED;
  resolve_policy(e->cfg, e->dev, e->listed_max);
  e->slots = 2 * prop.multiProcessorCount;   // the horizon-20 kernel's 256-VGPR, 4-wave workgroups: two per CU (horizon 10: four times that)

  if (wrench_serves(e->cfg)) {
    const int rc = cfg->N == 10 ? build_wrench_tables<10>(e) : build_wrench_tables<20>(e);
    if (rc != MPCQP_OK) return reject(rc);
  } else {   // the stage-wise engine runs as many persistent workgroups as the device holds
    int per_cu = 0;
    const bool f64 = e->cfg.precision == MPCQP_PREC_F64;
    const hipError_t oe = with_io(e, [&](auto tag) {
      using T = decltype(tag);
      return f64 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mpcqp_stage_solve<double, T>, SG_NT, 0)
                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mpcqp_stage_solve<float, T>, SG_NT, 0);
    });
    if (oe != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 1; }
    e->stage_slots = per_cu * prop.multiProcessorCount;
  }
  hipError_t he = upload(e->dcfg, &e->dev, sizeof(DevCfg));
  if (he == hipSuccess) he = hipEventCreate(&e->ev0);
  if (he == hipSuccess) he = hipEventCreate(&e->ev1);
  if (he != hipSuccess) return reject(MPCQP_EHIP);
  *out = e;
  return MPCQP_OK;
}

int mpcqp_destroy(mpcqp_handle h) {
  if (!h) return MPCQP_OK;
  DeviceGuard guard(h->cfg.device);
  free_engine(h);
  return MPCQP_OK;
}

const char* mpcqp_last_error(mpcqp_handle h) { return h ? h->err : "null handle"; }

int mpcqp_reserve(mpcqp_handle h, int64_t B) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_reserve: batch size out of range");
  GUARD(h);
  const int rc = reserve_workspace(h, B);
  return rc == MPCQP_OK ? rc : fail(h, rc, "mpcqp_reserve: workspace allocation failed");
}

int mpcqp_solve_batch(mpcqp_handle h, int64_t B, const void* x0, const void* r, const uint8_t* contact, const void* xdes,
                      const void* mu, void* u_out, void* X_out, int32_t* status, int32_t* iters, float* res, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_solve_batch: batch size out of range");
  if (B > 0 && (!x0 || !r || !contact || !xdes || !mu || !u_out || !status || !iters))
    return fail(h, MPCQP_EINVAL, "mpcqp_solve_batch: null buffer");
  if (B > 0) if (const int rc = solve_tables_match(h, B, "mpcqp_solve_batch")) return rc;
  GUARD(h);
  if (reserve_workspace(h, B) != MPCQP_OK) return fail(h, MPCQP_ENOMEM, "mpcqp_solve_batch: workspace allocation failed");
  hipStream_t st = (hipStream_t)stream;
  return timed(h, st, "kernel launch", [&] {
    if (B == 0) return hipSuccess;
    return with_io(h, [&](auto tag) {
      using T = decltype(tag);
      return enqueue_solve<T>(h, B, tuple_in<T>(h, x0, r, contact, xdes, mu, u_out), (T*)u_out, (T*)X_out, status, iters, res, st);
    });
  });
}

int mpcqp_solve_batch_gait_steps(mpcqp_handle h, int64_t B, int32_t S, const void* x0, const void* ref, const void* feet0, const void* footholds,
                                 const int32_t* gait, const uint8_t* feet_id, const void* mu, void* u_out, void* X_out,
                                 int32_t* status, int32_t* iters, float* res, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (S < 1) return fail(h, MPCQP_EINVAL, "mpcqp_solve_batch_gait_steps: at least one plan step");
  if (B < 0 || B > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_solve_batch_gait_steps: batch size out of range");
  if (B > 0 && (!x0 || !ref || !feet0 || !footholds || !gait || !feet_id || !mu || !u_out || !status || !iters))
    return fail(h, MPCQP_EINVAL, "mpcqp_solve_batch_gait_steps: null buffer");
  if (B == 0) return mpcqp_solve_batch(h, 0, x0, nullptr, nullptr, nullptr, mu, u_out, X_out, status, iters, res, stream);
  if (const int rc = solve_tables_match(h, B, "mpcqp_solve_batch_gait_steps")) return rc;
  hipStream_t st = (hipStream_t)stream;
  return solve_expanded(h, B, x0, mu, u_out, X_out, status, iters, res, st, "mpcqp_solve_batch_gait_steps: workspace allocation failed",
                        "gait expansion / solve kernel launch", [&](auto tag, const auto& w) {
    using T = decltype(tag);
    hipLaunchKernelGGL((mpcqp_gait_expand_kernel<T>), expand_grid(B, h->cfg.N), dim3(256), 0, st,
                       gait_in<T>(x0, mu, ref, feet0, footholds, gait, feet_id), h->cfg.delta, h->cfg.N, (int)S, B, w.r, w.contact, w.xdes);
  });
}

int mpcqp_solve_batch_gait(mpcqp_handle h, int64_t B, const void* x0, const void* ref, const void* feet0, const void* footholds,
                           const int32_t* gait, const uint8_t* feet_id, const void* mu, void* u_out, void* X_out,
                           int32_t* status, int32_t* iters, float* res, void* stream) {
  return mpcqp_solve_batch_gait_steps(h, B, 2, x0, ref, feet0, footholds, gait, feet_id, mu, u_out, X_out, status, iters, res, stream);
}

int mpcqp_rollout(mpcqp_handle h, int64_t B, int32_t T, int32_t S, void* x, void* ref, const void* plan_pos, const uint8_t* plan_feet_id,
                  const int32_t* plan_meta, int32_t* tick, const void* mu, void* actual, void* desired, void* forces, int32_t* solved,
                  void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || S < 1) return fail(h, MPCQP_EINVAL, "mpcqp_rollout: size out of range");
  if (B > 0 && (!x || !ref || !plan_pos || !plan_feet_id || !plan_meta || !tick || !mu)) return fail(h, MPCQP_EINVAL, "mpcqp_rollout: null buffer");
  if (B == 0 || T == 0) return MPCQP_OK;
  if (const int rc = solve_tables_match(h, B, "mpcqp_rollout")) return rc;
  return rollout_run(h, B, T, S, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, actual, desired, forces, solved, stream, nullptr);
}

int mpcqp_rollout_plant(mpcqp_handle h, int64_t B, int32_t T, int32_t S, void* x, void* ref, const void* plan_pos,
                        const uint8_t* plan_feet_id, const int32_t* plan_meta, int32_t* tick, const void* mu, const void* body,
                        const void* push, const int32_t* push_ticks, int32_t substeps, void* actual, void* desired, void* forces,
                        int32_t* solved, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || S < 1) return fail(h, MPCQP_EINVAL, "mpcqp_rollout_plant: size out of range");
  const int n = plant_substeps(substeps);
  if (n < 0) return fail(h, MPCQP_EINVAL, "mpcqp_rollout_plant: substeps out of range [0, 1000]");
  if (push && !push_ticks) return fail(h, MPCQP_EINVAL, "mpcqp_rollout_plant: push without push_ticks");
  if (B > 0 && (!x || !ref || !plan_pos || !plan_feet_id || !plan_meta || !tick || !mu))
    return fail(h, MPCQP_EINVAL, "mpcqp_rollout_plant: null buffer");
  if (B == 0 || T == 0) return MPCQP_OK;
  if (const int rc = solve_tables_match(h, B, "mpcqp_rollout_plant")) return rc;
  const RolloutPlantArgs plant = {body, push, push ? push_ticks : nullptr, n};
  return rollout_run(h, B, T, S, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, actual, desired, forces, solved, stream, &plant);
}

int mpcqp_phase_expand(mpcqp_handle h, int64_t B, const void* x0, const void* ref, const void* feet, const int32_t* gait, const int32_t* tick,
                       const void* stand, const void* gain, void* r, uint8_t* contact, void* xdes, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_phase_expand: batch size out of range");
  if (B > 0 && (!x0 || !ref || !feet || !gait || !tick || !stand || !r || !contact || !xdes))
    return fail(h, MPCQP_EINVAL, "mpcqp_phase_expand: null buffer");
  if (B == 0) return MPCQP_OK;
  return on_device(h, "phase expansion kernel launch", [&](auto tag) {
    using T = decltype(tag);
    launch_phase_expand<T>(h, B, (hipStream_t)stream, (const T*)x0, (const T*)ref, phase_rows<T>(feet, gait, stand, gain), tick,
                           {(T*)r, (T*)xdes, contact});
  });
}

int mpcqp_solve_batch_phase(mpcqp_handle h, int64_t B, const void* x0, const void* ref, const void* feet, const int32_t* gait,
                            const int32_t* tick, const void* stand, const void* gain, const void* mu, void* u_out, void* X_out,
                            int32_t* status, int32_t* iters, float* res, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_solve_batch_phase: batch size out of range");
  if (B > 0 && (!x0 || !ref || !feet || !gait || !tick || !stand || !mu || !u_out || !status || !iters))
    return fail(h, MPCQP_EINVAL, "mpcqp_solve_batch_phase: null buffer");
  if (B == 0) return mpcqp_solve_batch(h, 0, x0, nullptr, nullptr, nullptr, mu, u_out, X_out, status, iters, res, stream);
  if (const int rc = solve_tables_match(h, B, "mpcqp_solve_batch_phase")) return rc;
  hipStream_t st = (hipStream_t)stream;
  return solve_expanded(h, B, x0, mu, u_out, X_out, status, iters, res, st, "mpcqp_solve_batch_phase: workspace allocation failed",
                        "phase expansion / solve kernel launch", [&](auto tag, const auto& w) {
    using T = decltype(tag);
    launch_phase_expand<T>(h, B, st, (const T*)x0, (const T*)ref, phase_rows<T>(feet, gait, stand, gain), tick, w);
  });
}

int mpcqp_rollout_phase(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, const int32_t* gait, const void* stand,
                        const void* gain, int32_t* tick, const void* mu, const void* body, const void* push, const int32_t* push_ticks,
                        int32_t substeps, void* actual, void* desired, void* forces, void* feet_log, uint8_t* contact_log, int32_t* solved,
                        void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || B * (int64_t)T > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_rollout_phase: size out of range");
  const int n = plant_substeps(substeps);
  if (n < 0) return fail(h, MPCQP_EINVAL, "mpcqp_rollout_phase: substeps out of range [0, 1000]");
  if (push && !push_ticks) return fail(h, MPCQP_EINVAL, "mpcqp_rollout_phase: push without push_ticks");
  if (B > 0 && (!x || !ref || !feet || !gait || !stand || !tick || !mu)) return fail(h, MPCQP_EINVAL, "mpcqp_rollout_phase: null buffer");
  if (B == 0 || T == 0) return MPCQP_OK;
  if (const int rc = solve_tables_match(h, B, "mpcqp_rollout_phase")) return rc;
  const RolloutPlantArgs plant = {body, push, push ? push_ticks : nullptr, n};
  hipStream_t st = (hipStream_t)stream;
  return rollout_loop(h, "mpcqp_rollout_phase", B, T, x, ref, mu, stream,
    [&](auto tag, auto* xs, auto* rf, const auto& w, int) {
      using TIO = decltype(tag);
      launch_phase_expand<TIO>(h, B, st, xs, rf, phase_rows<TIO>(feet, gait, stand, gain), tick, w);
    },
    [&](auto tag, auto* xs, auto* rf, const auto& o, int it) {
      using TIO = decltype(tag);
      hipLaunchKernelGGL((mpcqp_phase_advance_kernel<TIO>), advance_grid(B), dim3(256), 0, st, xs, rf, (TIO*)feet, phase_rows<TIO>(feet, gait, stand, gain),
                         tick, plant_in<TIO>(h, plant), o.u, o.status, h->cfg.delta, h->cfg.N, B, (int)T, it, (TIO*)actual, (TIO*)desired,
                         (TIO*)forces, (TIO*)feet_log, contact_log, solved);
    });
}

int mpcqp_set_models(mpcqp_handle h, int64_t B, const double* model, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B <= 0 || B > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_set_models: batch size out of range");
  if (!model) return fail(h, MPCQP_EINVAL, "mpcqp_set_models: null model table");
  GUARD(h);
  // (after growth the device's pointer is the freed buffer until the kernel below has run: if its launch fails, no solve may read it)
  if (!table_reserve(models(h), B, MODEL_ROW)) return fail(h, MPCQP_ENOMEM, "mpcqp_set_models: table allocation failed");
  hipLaunchKernelGGL(mpcqp_model_rows_kernel, blocks(B), dim3(256), 0, (hipStream_t)stream, model, h->model_mem, B, h->dcfg);
  const int rc = launched(h, "model table kernel launch");
  h->model_B = rc == MPCQP_OK ? B : 0;
  return rc;
}

int mpcqp_clear_models(mpcqp_handle h) {
  if (!h) return MPCQP_EINVAL;
  if (h->model_B == 0) return MPCQP_OK;
  GUARD(h);
  // No stream argument: the solves enqueued so far (on whatever stream) finish with the table, every later one starts without it.
  hipError_t he = hipDeviceSynchronize();
  if (he == hipSuccess) { hipLaunchKernelGGL(mpcqp_model_clear_kernel, dim3(1), dim3(1), 0, nullptr, h->dcfg); he = hipGetLastError(); }
  if (he == hipSuccess) he = hipDeviceSynchronize();
  if (he != hipSuccess) return fail(h, MPCQP_EHIP, "mpcqp_clear_models", he);
  h->model_B = 0;
  return MPCQP_OK;
}

// include/mpcqp_disturb.h.  The table is a kernel argument of the two kernels around a solve, so only the host side of the handle knows it.
int mpcqp_set_disturbance(mpcqp_handle h, int64_t B, const double* rows, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B <= 0 || B > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_set_disturbance: batch size out of range");
  if (!rows) return fail(h, MPCQP_EINVAL, "mpcqp_set_disturbance: null disturbance table");
  GUARD(h);
  if (const int rc = reserve_disturbance(h, B, "mpcqp_set_disturbance")) return rc;
  hipLaunchKernelGGL(mpcqp_disturb_rows_kernel, blocks(B), dim3(256), 0, (hipStream_t)stream, rows, h->dist_mem, B);
  const int rc = launched(h, "disturbance table kernel launch");
  h->dist_B = rc == MPCQP_OK ? B : 0;
  return rc;
}

int mpcqp_clear_disturbance(mpcqp_handle h) {
  if (!h) return MPCQP_EINVAL;
  if (h->dist_B == 0) return MPCQP_OK;
  GUARD(h);
  // No stream argument: the solves enqueued so far (on whatever stream) finish with the table, every later one runs without it.
  const hipError_t he = hipDeviceSynchronize();
  if (he != hipSuccess) return fail(h, MPCQP_EHIP, "mpcqp_clear_disturbance", he);
  h->dist_B = 0;
  return MPCQP_OK;
}

int mpcqp_disturbance_shift(mpcqp_handle h, int64_t B, const void* x0, const void* xdes, void* out, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_disturbance_shift: batch size out of range");
  if (h->dist_B == 0) return fail(h, MPCQP_EINVAL, "mpcqp_disturbance_shift: no disturbance table is set");
  if (B > 0 && (!x0 || !xdes || !out)) return fail(h, MPCQP_EINVAL, "mpcqp_disturbance_shift: null buffer");
  if (const int rc = solve_tables_match(h, B, "mpcqp_disturbance_shift")) return rc;
  if (B == 0) return MPCQP_OK;
  return on_device(h, "disturbance shift kernel launch", [&](auto tag) {
    using T = decltype(tag);
    launch_disturb_shift<T>(h, B, (const T*)x0, (const T*)xdes, (T*)out, (hipStream_t)stream);
  });
}

int mpcqp_default_wrench_observer(MpcQpWrenchObserver* par) {
  if (!par) return MPCQP_EINVAL;
  memset(par, 0, sizeof(*par));
  par->size = (uint32_t)sizeof(*par);
  par->gravity = -9.81;
  par->kappa = 0.2;
  par->f_lim = INFINITY;
  par->t_lim = INFINITY;
  return MPCQP_OK;
}

int mpcqp_disturbance_track(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet, const void* body,
                            const MpcQpWrenchObserver* par, double* state, void* dist, void* resid, void* stream) {
  const char* who = "mpcqp_disturbance_track";
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || B * (int64_t)T > 0x1fffffff) return bad(h, who, "size out of range");
  if (!dist && !resid) return bad(h, who, "no output buffer (dist and resid are both null)");
  if (B > 0 && T > 0 && (!actual || !forces || !feet)) return bad(h, who, "null buffer (actual, forces, feet)");
  DistPar e;
  if (const int rc = observer_row(h, who, par, e)) return rc;
  if (B == 0 || T == 0) return MPCQP_OK;
  return on_device(h, "disturbance track kernel launch", [&](auto tag) {
    using TIO = decltype(tag);
    hipLaunchKernelGGL((mpcqp_disturb_track_kernel<TIO>), blocks(B), dim3(256), 0, (hipStream_t)stream, (const TIO*)actual, (const TIO*)forces,
                       (const TIO*)feet, (const TIO*)body, plant_model(h), e, state, (TIO*)dist, (TIO*)resid, B, (int)T);
  });
}

// include/mpcqp_actuators.h.  The table is a kernel argument of the ACT instantiations, so only the host side of the handle knows it.
int mpcqp_set_actuators(mpcqp_handle h, int64_t B, const double* act, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B <= 0 || B > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_set_actuators: batch size out of range");
  if (!act) return fail(h, MPCQP_EINVAL, "mpcqp_set_actuators: null actuator table");
  GUARD(h);
  if (!table_reserve(actuators(h), B, ACT_ROW)) return fail(h, MPCQP_ENOMEM, "mpcqp_set_actuators: table allocation failed");
  hipLaunchKernelGGL(mpcqp_actuator_rows_kernel, blocks(B), dim3(256), 0, (hipStream_t)stream, act, h->act_mem, B);
  const int rc = launched(h, "actuator table kernel launch");
  h->act_B = rc == MPCQP_OK ? B : 0;
  return rc;
}

int mpcqp_clear_actuators(mpcqp_handle h) {
  if (!h) return MPCQP_EINVAL;
  if (h->act_B == 0) return MPCQP_OK;
  GUARD(h);
  // No stream argument: the calls enqueued so far (on whatever stream) finish with the table, every later one runs without it.
  const hipError_t he = hipDeviceSynchronize();
  if (he != hipSuccess) return fail(h, MPCQP_EHIP, "mpcqp_clear_actuators", he);
  h->act_B = 0;
  return MPCQP_OK;
}

int mpcqp_plant_step(mpcqp_handle h, int64_t B, const void* x, const void* f, const void* feet, const uint8_t* contact,
                     const void* body, const void* wrench, int32_t substeps, void* x_out, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_plant_step: batch size out of range");
  const int n = plant_substeps(substeps);
  if (n < 0) return fail(h, MPCQP_EINVAL, "mpcqp_plant_step: substeps out of range [0, 1000]");
  if (B > 0 && (!x || !f || !feet || !contact || !x_out)) return fail(h, MPCQP_EINVAL, "mpcqp_plant_step: null buffer");
  if (B == 0) return MPCQP_OK;
  return on_device(h, "plant kernel launch", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((mpcqp_plant_step_kernel<T>), blocks(B), dim3(256), 0, (hipStream_t)stream, (const T*)x, (const T*)f, (const T*)feet,
                       contact, (const T*)body, (const T*)wrench, plant_model(h), n, h->cfg.delta / n, B, (T*)x_out);
  });
}

int mpcqp_plan_footsteps(mpcqp_handle h, int64_t B, int32_t S, const void* feet0, const void* cmd, const int32_t* gait, void* plan_pos,
                         uint8_t* plan_feet_id, int32_t* plan_meta, void* plan_ang, void* plan_hip, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || S < 1 || B * (int64_t)S > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_plan_footsteps: size out of range");
  if (B > 0 && (!feet0 || !cmd || !gait || !plan_pos || !plan_feet_id || !plan_meta))
    return fail(h, MPCQP_EINVAL, "mpcqp_plan_footsteps: null buffer");
  if (B == 0) return MPCQP_OK;
  GUARD(h);
  const int64_t rows = B * S;
  if (h->plan_cap < rows) {   // once per size; later calls at this size or smaller allocate nothing
    if (!grow(h->plan_ws, (size_t)rows * PLAN_WS * sizeof(double)))
      return fail(h, MPCQP_ENOMEM, "mpcqp_plan_footsteps: workspace allocation failed");
    h->plan_cap = rows;
  }
  hipStream_t st = (hipStream_t)stream;
  with_io(h, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((mpcqp_plan_unicycle_kernel<T>), blocks(B, 64), dim3(64), 0, st, (const T*)feet0, (const T*)cmd, gait, h->cfg.delta, (int)S,
                       B, h->plan_ws);
    hipLaunchKernelGGL((mpcqp_plan_tables_kernel<T>), blocks(rows, PLAN_BLOCK), dim3(PLAN_BLOCK), 0, st, (const T*)feet0, (const T*)cmd, gait,
                       (const double*)h->plan_ws, (int)S, B, (T*)plan_pos, plan_feet_id, plan_meta, (T*)plan_ang, (T*)plan_hip);
  });
  return launched(h, "footstep planner kernel launch");
}

int mpcqp_swing_trajectories(mpcqp_handle h, int64_t B, int32_t K, int32_t S, const void* plan_pos, const uint8_t* plan_feet_id,
                             const int32_t* plan_meta, const void* plan_ang, const int32_t* tick, const void* step_height, void* traj,
                             void* feet_des, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || K < 0 || S < 1 || B * (int64_t)K > 0x7fffffff)
    return fail(h, MPCQP_EINVAL, "mpcqp_swing_trajectories: size out of range");
  if (B > 0 && K > 0 && (!plan_pos || !plan_feet_id || !plan_meta || !plan_ang || !tick || !step_height || !traj))
    return fail(h, MPCQP_EINVAL, "mpcqp_swing_trajectories: null buffer");
  if (B == 0 || K == 0) return MPCQP_OK;
  return on_device(h, "swing trajectory kernel launch", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((mpcqp_swing_kernel<T>), blocks(B * K * 4, PLAN_BLOCK), dim3(PLAN_BLOCK), 0, (hipStream_t)stream, (const T*)plan_pos,
                       plan_feet_id, plan_meta, (const T*)plan_ang, tick, (const T*)step_height, h->cfg.delta, (int)K, (int)S, B, (T*)traj,
                       (T*)feet_des);
  });
}

int mpcqp_phase_swing(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* desired, const void* feet_log, const int32_t* gait,
                      const int32_t* tick0, const void* stand, const void* gain, const void* step_height, void* swing, void* feet_des,
                      void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || B * (int64_t)T > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_phase_swing: size out of range");
  if (B > 0 && T > 0 && (!actual || !desired || !feet_log || !gait || !tick0 || !stand || !step_height || !swing))
    return fail(h, MPCQP_EINVAL, "mpcqp_phase_swing: null buffer");
  if (B == 0 || T == 0) return MPCQP_OK;
  return on_device(h, "phase swing kernel launch", [&](auto tag) {
    using TIO = decltype(tag);
    hipLaunchKernelGGL((mpcqp_phase_swing_kernel<TIO>), leg_grid(B * T), dim3(256), 0, (hipStream_t)stream, (const TIO*)actual, (const TIO*)desired,
                       (const TIO*)feet_log, gait, tick0, (const TIO*)stand, (const TIO*)gain, (const TIO*)step_height, h->cfg.delta, (int)T, B,
                       (TIO*)swing, (TIO*)feet_des);
  });
}

int mpcqp_torque_map(mpcqp_handle h, int64_t B, const void* u, const void* jac, void* tau, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_torque_map: batch size out of range");
  if (B > 0 && (!u || !jac || !tau)) return fail(h, MPCQP_EINVAL, "mpcqp_torque_map: null buffer");
  if (B == 0) return MPCQP_OK;
  return on_device(h, "torque kernel launch", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((mpcqp_torque_kernel<T>), leg_grid(B), dim3(256), 0, (hipStream_t)stream, (const T*)u, (const T*)jac, (T*)tau, B, h->cfg.N);
  });
}

int mpcqp_default_leg_geometry(MpcQpLegGeometry* g) {   // lite3_urdf/urdf/Lite3.urdf:44-124 (joint origins and axes; data)
  if (!g) return MPCQP_EINVAL;
  memset(g, 0, sizeof(*g));
  g->size = (uint32_t)sizeof(*g);
  for (int l = 0; l < 4; ++l) {
    g->hip_x[l][0] = l < 2 ? 0.1745 : -0.1745;
    g->hip_x[l][1] = (l % 2 == 0) ? 0.062 : -0.062;
    g->hip_y[l][1] = (l % 2 == 0) ? 0.0985 : -0.0985;
  }
  g->knee[2] = -0.20;
  g->foot[2] = -0.21;
  g->axis_x[0] = -1.0;
  g->axis_y[1] = -1.0;
  return MPCQP_OK;
}

int mpcqp_leg_jacobians(mpcqp_handle h, int64_t B, const void* q, const void* rot, const MpcQpLegGeometry* geo, void* jac, void* foot,
                        void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_leg_jacobians: batch size out of range");
  if (B > 0 && (!q || !jac)) return fail(h, MPCQP_EINVAL, "mpcqp_leg_jacobians: null buffer");
  LegGeoDev g;
  if (const int rc = leg_geometry(h, "mpcqp_leg_jacobians", geo, false, g)) return rc;
  if (B == 0) return MPCQP_OK;
  return on_device(h, "leg Jacobian kernel launch", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((mpcqp_leg_jacobian_kernel<T>), leg_grid(B), dim3(256), 0, (hipStream_t)stream, (const T*)q, (const T*)rot, g, (T*)jac,
                       (T*)foot, B);
  });
}

int mpcqp_leg_ik(mpcqp_handle h, int64_t B, const void* foot, const void* rot, const void* origin, const MpcQpLegGeometry* geo, void* q,
                 uint8_t* reach, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_leg_ik: batch size out of range");
  if (B > 0 && !foot) return fail(h, MPCQP_EINVAL, "mpcqp_leg_ik: null foot buffer");
  if (B > 0 && !q) return fail(h, MPCQP_EINVAL, "mpcqp_leg_ik: null q buffer");
  LegGeoDev g;
  if (const int rc = leg_geometry(h, "mpcqp_leg_ik", geo, true, g)) return rc;
  if (B == 0) return MPCQP_OK;
  return on_device(h, "leg inverse kinematics kernel launch", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((mpcqp_leg_ik_kernel<T>), leg_grid(B), dim3(256), 0, (hipStream_t)stream, (const T*)foot, (const T*)rot, (const T*)origin,
                       g, (T*)q, reach, B);
  });
}

int mpcqp_joint_log(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet,
                    const MpcQpLegGeometry* geo, void* q, void* tau, uint8_t* reach, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || B * (int64_t)T > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_joint_log: size out of range");
  if (!q && !tau && !reach) return fail(h, MPCQP_EINVAL, "mpcqp_joint_log: no output buffer (q, tau and reach are all null)");
  if (B > 0 && T > 0 && (!actual || !forces || !feet)) return fail(h, MPCQP_EINVAL, "mpcqp_joint_log: null buffer");
  LegGeoDev g;
  if (const int rc = leg_geometry(h, "mpcqp_joint_log", geo, true, g)) return rc;
  if (B == 0 || T == 0) return MPCQP_OK;
  const int64_t rows = B * T;
  return on_device(h, "joint log kernel launch", [&](auto tag) {
    using TIO = decltype(tag);
    hipLaunchKernelGGL((mpcqp_joint_log_kernel<TIO>), leg_grid(rows), dim3(256), 0, (hipStream_t)stream, (const TIO*)actual, (const TIO*)forces,
                       (const TIO*)feet, g, (TIO*)q, (TIO*)tau, reach, rows);
  });
}

int mpcqp_joint_rates(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet, const void* foot_vel,
                      const MpcQpLegGeometry* geo, void* q, void* qd, void* tau, void* power, uint8_t* reach, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || B * (int64_t)T > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_joint_rates: size out of range");
  if (!q && !qd && !tau && !power && !reach)
    return fail(h, MPCQP_EINVAL, "mpcqp_joint_rates: no output buffer (q, qd, tau, power and reach are all null)");
  if (B > 0 && T > 0 && (!actual || !forces || !feet)) return fail(h, MPCQP_EINVAL, "mpcqp_joint_rates: null buffer");
  LegGeoDev g;
  if (const int rc = leg_geometry(h, "mpcqp_joint_rates", geo, true, g)) return rc;
  if (B == 0 || T == 0) return MPCQP_OK;
  const int64_t rows = B * T;
  return on_device(h, "joint rates kernel launch", [&](auto tag) {
    using TIO = decltype(tag);
    hipLaunchKernelGGL((mpcqp_joint_rates_kernel<TIO>), leg_grid(rows), dim3(256), 0, (hipStream_t)stream, (const TIO*)actual, (const TIO*)forces,
                       (const TIO*)feet, (const TIO*)foot_vel, g, (TIO*)q, (TIO*)qd, (TIO*)tau, (TIO*)power, reach, rows);
  });
}

int mpcqp_default_leg_inertia(MpcQpLegInertia* r) {   // lite3_urdf/urdf/Lite3.urdf: <inertial> of the HIP / THIGH / SHANK / FOOT links, joint <limit> rows (data)
  if (!r) return MPCQP_EINVAL;
  memset(r, 0, sizeof(*r));
  r->size = (uint32_t)sizeof(*r);
  // HIP: mirrored left / right in y and front / hind in x, to the description's own digits (its rows differ in the last ones)
  static const double hip_com[4][3] = {{-0.0047, -0.0091, -0.0018}, {-0.0047, 0.0091, -0.0018}, {0.0047, -0.0091, -0.0018}, {0.0047, 0.0091, -0.0018}};
  static const double hip_prod[4][3] = {{8.1579e-07, -1.264e-05, 1.3443e-06}, {-8.1551e-07, -1.2639e-05, -1.3441e-06},
                                        {-8.1585e-07, 1.2639e-05, 1.3444e-06}, {8.1545e-07, 1.2639e-05, -1.344e-06}};
  const double foot_m = 0.01, foot_i = 1e-2, foot_c[3] = {0.0, 0.0, -0.21};   // the FOOT link, on the fixed Ankle joint
  for (int l = 0; l < 4; ++l) {
    const double sy = (l % 2 == 0) ? 1.0 : -1.0;   // left : right
    r->mass[l][0] = 0.428;
    for (int a = 0; a < 3; ++a) { r->com[l][0][a] = hip_com[l][a]; r->inertia[l][0][3 + a] = hip_prod[l][a]; }
    r->inertia[l][0][0] = 0.00014538; r->inertia[l][0][1] = 0.00024024; r->inertia[l][0][2] = 0.00013038;
    // THIGH: mirrored left / right only (the hind thighs are the front ones)
    r->mass[l][1] = 0.61;
    r->com[l][1][0] = -0.00523; r->com[l][1][1] = -0.0216 * sy; r->com[l][1][2] = -0.0273;
    r->inertia[l][1][0] = 0.001; r->inertia[l][1][1] = 0.00116; r->inertia[l][1][2] = 2.68e-04;
    r->inertia[l][1][3] = -2.5e-06 * sy; r->inertia[l][1][4] = -1.12e-04; r->inertia[l][1][5] = 3.75e-07 * sy;
    // SHANK (the same row on all four legs) with the FOOT folded in by the parallel-axis theorem
    const double sm = 0.115, sc[3] = {0.00585, -8.732e-07, -0.12};
    const double si[6] = {6.68e-04, 6.86e-04, 3.155e-05, -1.24e-08, 6.91e-06, 5.65e-09};
    const double m = sm + foot_m;
    double c[3], I[6];
    for (int a = 0; a < 3; ++a) c[a] = (sm * sc[a] + foot_m * foot_c[a]) / m;
    for (int a = 0; a < 6; ++a) I[a] = si[a] + (a < 3 ? foot_i : 0.0);
    for (int k = 0; k < 2; ++k) {
      const double mk = k ? foot_m : sm;
      const double* ck = k ? foot_c : sc;
      const double dx = ck[0] - c[0], dy = ck[1] - c[1], dz = ck[2] - c[2];
      I[0] = I[0] + mk * (dy * dy + dz * dz); I[1] = I[1] + mk * (dx * dx + dz * dz); I[2] = I[2] + mk * (dx * dx + dy * dy);
      I[3] = I[3] - mk * (dx * dy); I[4] = I[4] - mk * (dx * dz); I[5] = I[5] - mk * (dy * dz);
    }
    r->mass[l][2] = m;
    for (int a = 0; a < 3; ++a) r->com[l][2][a] = c[a];
    for (int a = 0; a < 6; ++a) r->inertia[l][2][a] = I[a];
  }
  const double lim[4][3] = {{-0.42, -2.67, 0.6}, {0.42, 0.314, 2.72}, {26.0, 26.0, 17.0}, {24.0, 24.0, 36.0}};
  for (int j = 0; j < 3; ++j) { r->q_min[j] = lim[0][j]; r->q_max[j] = lim[1][j]; r->qd_max[j] = lim[2][j]; r->tau_max[j] = lim[3][j]; }
  r->gravity = -9.81;
  return MPCQP_OK;
}

int mpcqp_leg_dynamics(mpcqp_handle h, int64_t B, const void* q, const void* qd, const void* qdd, const void* rot, const void* base,
                       const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, void* tau, void* mass, void* bias, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_leg_dynamics: batch size out of range");
  if (!tau && !mass && !bias) return fail(h, MPCQP_EINVAL, "mpcqp_leg_dynamics: no output buffer (tau, mass and bias are all null)");
  if (B > 0 && !q) return fail(h, MPCQP_EINVAL, "mpcqp_leg_dynamics: null q buffer");
  LegGeoDev g;
  LegInrDev r;
  if (const int rc = leg_rows(h, "mpcqp_leg_dynamics", geo, inr, false, g, r)) return rc;
  if (B == 0) return MPCQP_OK;
  return on_device(h, "leg dynamics kernel launch", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((mpcqp_leg_dynamics_kernel<T>), leg_grid(B), dim3(256), 0, (hipStream_t)stream, (const T*)q, (const T*)qd, (const T*)qdd,
                       (const T*)rot, (const T*)base, g, r.k0, r.k1, r.k2, r.lim, (T*)tau, (T*)mass, (T*)bias, B);
  });
}

int mpcqp_leg_effort(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet, const void* foot_vel,
                     const void* foot_acc, const void* base_acc, const void* body, const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr,
                     void* qdd, void* tau_dyn, void* tau, void* power, uint8_t* limit, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || B * (int64_t)T > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_leg_effort: size out of range");
  if (!qdd && !tau_dyn && !tau && !power && !limit)
    return fail(h, MPCQP_EINVAL, "mpcqp_leg_effort: no output buffer (qdd, tau_dyn, tau, power and limit are all null)");
  if (B > 0 && T > 0 && (!actual || !forces || !feet)) return fail(h, MPCQP_EINVAL, "mpcqp_leg_effort: null buffer");
  LegGeoDev g;
  LegInrDev r;
  if (const int rc = leg_rows(h, "mpcqp_leg_effort", geo, inr, true, g, r)) return rc;
  if (B == 0 || T == 0) return MPCQP_OK;
  if (const int rc = actuators_match(h, B, "mpcqp_leg_effort")) return rc;
  const int64_t rows = B * T;
  return on_device(h, "leg effort kernel launch", [&](auto tag) {
    using TIO = decltype(tag);
    launch_act(h, leg_grid(rows), (hipStream_t)stream, mpcqp_leg_effort_kernel<TIO>, mpcqp_leg_effort_kernel<TIO, double>,
               (const TIO*)actual, (const TIO*)forces, (const TIO*)feet, (const TIO*)foot_vel, (const TIO*)foot_acc, (const TIO*)base_acc,
               (const TIO*)body, plant_model(h), g, r.k0, r.k1, r.k2, r.lim, (TIO*)qdd, (TIO*)tau_dyn, (TIO*)tau, (TIO*)power, limit, rows,
               (int64_t)T);
  });
}

int mpcqp_leg_accel(mpcqp_handle h, int64_t B, const void* q, const void* qd, const void* tau, const void* rot, const void* base,
                    const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, void* qdd, void* det, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_leg_accel: batch size out of range");
  if (B > 0 && !q) return fail(h, MPCQP_EINVAL, "mpcqp_leg_accel: null q buffer");
  if (B > 0 && !tau) return fail(h, MPCQP_EINVAL, "mpcqp_leg_accel: null tau buffer");
  if (B > 0 && !qdd) return fail(h, MPCQP_EINVAL, "mpcqp_leg_accel: null qdd buffer");
  LegGeoDev g;
  LegInrDev r;
  if (const int rc = leg_rows(h, "mpcqp_leg_accel", geo, inr, false, g, r)) return rc;
  if (B == 0) return MPCQP_OK;
  return on_device(h, "leg acceleration kernel launch", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((mpcqp_leg_accel_kernel<T>), leg_grid(B), dim3(256), 0, (hipStream_t)stream, (const T*)q, (const T*)qd, (const T*)tau,
                       (const T*)rot, (const T*)base, g, r.k0, r.k1, r.k2, r.lim, (T*)qdd, (T*)det, B);
  });
}

int mpcqp_swing_track(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet_log,
                      const uint8_t* contact_log, const void* swing, const void* base_acc, const void* body, const void* gains, void* state,
                      int32_t substeps, const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, void* q, void* qd, void* tau, void* foot,
                      void* err, uint8_t* flag, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || B * (int64_t)T > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_swing_track: size out of range");
  if (substeps < 0 || substeps > SWING_MAX_SUBSTEPS) return fail(h, MPCQP_EINVAL, "mpcqp_swing_track: substeps out of range [0, 1000]");
  if (!q && !qd && !tau && !foot && !err && !flag)
    return fail(h, MPCQP_EINVAL, "mpcqp_swing_track: no output buffer (q, qd, tau, foot, err and flag are all null)");
  if (B > 0 && T > 0 && (!actual || !forces || !feet_log || !contact_log || !swing)) return fail(h, MPCQP_EINVAL, "mpcqp_swing_track: null buffer");
  LegGeoDev g;
  LegInrDev r;
  if (const int rc = leg_rows(h, "mpcqp_swing_track", geo, inr, true, g, r)) return rc;
  if (B == 0 || T == 0) return MPCQP_OK;
  if (const int rc = actuators_match(h, B, "mpcqp_swing_track")) return rc;
  const int n = swing_substeps(h->cfg.delta, substeps);
  return on_device(h, "swing track kernel launch", [&](auto tag) {
    using TIO = decltype(tag);
    const SwingIn<TIO> in = {(const TIO*)actual, (const TIO*)forces, (const TIO*)feet_log, contact_log, (const TIO*)swing,
                             (const TIO*)base_acc, (const TIO*)body, (const TIO*)gains};
    const SwingOut<TIO> out = {(TIO*)q, (TIO*)qd, (TIO*)tau, (TIO*)foot, (TIO*)err, flag};
    launch_act(h, leg_grid(B), (hipStream_t)stream, mpcqp_swing_track_kernel<TIO>, mpcqp_swing_track_kernel<TIO, double>, in, (TIO*)state,
               plant_model(h), g, r.k0, r.k1, r.k2, r.lim, out, B, (int)T, n, h->cfg.delta / n);
  });
}

int mpcqp_rollout_legs(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                       const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                       const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains, int32_t leg_substeps,
                       const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, void* actual, void* desired, void* forces,
                       void* feet_log, uint8_t* contact_log, int32_t* solved, void* swing_log, void* q_log, void* qd_log, void* tau_log,
                       void* foot_log, void* err_log, uint8_t* flag_log, void* miss_log, void* stream) {
  return rollout_legs_run(h, "mpcqp_rollout_legs", B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps,
                          step_height, gains, leg_substeps, geo, inr, land, actual, desired, forces, feet_log, contact_log, solved, swing_log,
                          q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, stream, nullptr);
}

int mpcqp_rollout_drive(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                        const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                        const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains, int32_t leg_substeps,
                        const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, int32_t drive, const void* ground,
                        void* actual, void* desired, void* forces, void* feet_log, uint8_t* contact_log, int32_t* solved, void* swing_log,
                        void* q_log, void* qd_log, void* tau_log, void* foot_log, void* err_log, uint8_t* flag_log, void* miss_log,
                        void* cmd_log, void* stream) {
  const RolloutDriveArgs dr = {drive, ground, cmd_log};
  return rollout_legs_run(h, "mpcqp_rollout_drive", B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps,
                          step_height, gains, leg_substeps, geo, inr, land, actual, desired, forces, feet_log, contact_log, solved, swing_log,
                          q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, stream, &dr);
}

int mpcqp_stance_drive(mpcqp_handle h, int64_t B, const void* x, const void* f, const void* feet, const uint8_t* contact, const void* ground,
                       const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, void* f_out, void* tau, uint8_t* flag, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_stance_drive: batch size out of range");
  if (B > 0 && (!x || !f || !feet || !contact || !f_out)) return fail(h, MPCQP_EINVAL, "mpcqp_stance_drive: null buffer");
  LegGeoDev g;
  LegInrDev r;
  if (const int rc = leg_rows(h, "mpcqp_stance_drive", geo, inr, true, g, r)) return rc;
  if (B == 0) return MPCQP_OK;
  if (const int rc = actuators_match(h, B, "mpcqp_stance_drive")) return rc;
  return on_device(h, "stance drive kernel launch", [&](auto tag) {
    using TIO = decltype(tag);
    launch_act(h, leg_grid(B), (hipStream_t)stream, mpcqp_stance_drive_kernel<TIO>, mpcqp_stance_drive_kernel<TIO, double>,
               (const TIO*)x, (const TIO*)f, (int64_t)12, (const TIO*)feet, contact, (const int32_t*)nullptr, (const int32_t*)nullptr,
               (const TIO*)ground, g, r.lim, (int)DRIVE_LIMITED, (TIO*)f_out, (TIO*)tau, flag, (TIO*)nullptr, (int64_t)0, B);
  });
}

int mpcqp_rollout_slip(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                       const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                       const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains, int32_t leg_substeps,
                       const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, int32_t drive, const void* ground,
                       const void* foot_mass, double* slip, void* actual, void* desired, void* forces, void* feet_log, uint8_t* contact_log,
                       int32_t* solved, void* swing_log, void* q_log, void* qd_log, void* tau_log, void* foot_log, void* err_log,
                       uint8_t* flag_log, void* miss_log, void* cmd_log, double* slip_log, void* disp_log, void* stream) {
  const RolloutDriveArgs dr = {drive, ground, cmd_log};
  const RolloutSlipArgs sl = {foot_mass, slip, slip_log, disp_log};
  return rollout_legs_run(h, "mpcqp_rollout_slip", B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps,
                          step_height, gains, leg_substeps, geo, inr, land, actual, desired, forces, feet_log, contact_log, solved, swing_log,
                          q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, stream, &dr, &sl);
}

int mpcqp_stance_slip(mpcqp_handle h, int64_t B, const void* x, const void* f, const void* feet, const uint8_t* contact, const void* ground,
                      const void* foot_mass, const double* slip_in, int32_t substeps, const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr,
                      void* f_out, void* tau, uint8_t* flag, double* slip_out, void* disp, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_stance_slip: batch size out of range");
  const int n = plant_substeps(substeps);
  if (n < 0) return fail(h, MPCQP_EINVAL, "mpcqp_stance_slip: substeps out of range [0, 1000]");
  if (B > 0 && (!x || !f || !feet || !contact || !ground || !foot_mass || !slip_in || !f_out))
    return fail(h, MPCQP_EINVAL, "mpcqp_stance_slip: null buffer");
  LegGeoDev g;
  LegInrDev r;
  if (const int rc = leg_rows(h, "mpcqp_stance_slip", geo, inr, true, g, r)) return rc;
  if (B == 0) return MPCQP_OK;
  if (const int rc = actuators_match(h, B, "mpcqp_stance_slip")) return rc;
  const double d = h->cfg.delta;
  return on_device(h, "stance slip kernel launch", [&](auto tag) {
    using TIO = decltype(tag);
    launch_act(h, leg_grid(B), (hipStream_t)stream, mpcqp_stance_slip_kernel<TIO>, mpcqp_stance_slip_kernel<TIO, double>,
               (const TIO*)x, (const TIO*)f, (int64_t)12, (const TIO*)feet, contact, (const int32_t*)nullptr, (const int32_t*)nullptr,
               (const TIO*)ground, (const TIO*)foot_mass, slip_in, g, r.lim, (int)DRIVE_LIMITED, n, d / n, d, (TIO*)f_out, (TIO*)tau, flag,
               (TIO*)nullptr, (int64_t)0, slip_out, (TIO*)disp, (double*)nullptr, (int64_t)0, B);
  });
}

int mpcqp_rollout_observe(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                          const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                          const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains, int32_t leg_substeps,
                          const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, int32_t drive, const void* ground,
                          const void* foot_mass, double* slip, void* actual, void* desired, void* forces, void* feet_log, uint8_t* contact_log,
                          int32_t* solved, void* swing_log, void* q_log, void* qd_log, void* tau_log, void* foot_log, void* err_log,
                          uint8_t* flag_log, void* miss_log, void* cmd_log, double* slip_log, void* disp_log, int32_t feed, double* est_state,
                          const void* est_init, const void* height, const void* bias, const void* noise, const void* enc_noise,
                          const MpcQpEstimator* par, void* imu_log, void* q_enc_log, void* qd_enc_log, void* est_log, void* feet_est_log,
                          void* sigma_log, void* nis_log, void* stream) {
  const RolloutSlipCall c = {B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height, gains,
                             leg_substeps, geo, inr, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log, contact_log,
                             solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log};
  return rollout_observe_run(h, "mpcqp_rollout_observe", c, feed, est_state, est_init, height, bias, noise, enc_noise, par, imu_log, q_enc_log,
                             qd_enc_log, est_log, feet_est_log, sigma_log, nis_log, false, nullptr, nullptr, stream);
}

int mpcqp_rollout_observe_aided(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                                const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                                const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains,
                                int32_t leg_substeps, const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, int32_t drive,
                                const void* ground, const void* foot_mass, double* slip, void* actual, void* desired, void* forces,
                                void* feet_log, uint8_t* contact_log, int32_t* solved, void* swing_log, void* q_log, void* qd_log,
                                void* tau_log, void* foot_log, void* err_log, uint8_t* flag_log, void* miss_log, void* cmd_log,
                                double* slip_log, void* disp_log, int32_t feed, double* est_state, const void* est_init, const void* height,
                                const void* bias, const void* noise, const void* enc_noise, const MpcQpEstimator* par, void* imu_log,
                                void* q_enc_log, void* qd_enc_log, void* est_log, void* feet_est_log, void* sigma_log, void* nis_log,
                                const MpcQpTrustGate* gate, void* trust_log, int32_t flags, const MpcQpAttitude* att, double* att_state,
                                void* bias_log, void* stream) {
  const RolloutSlipCall c = {B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height, gains,
                             leg_substeps, geo, inr, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log, contact_log,
                             solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log};
  const EstimateAidedArgs ad = {flags, att, att_state, bias_log};
  return rollout_observe_run(h, "mpcqp_rollout_observe_aided", c, feed, est_state, est_init, height, bias, noise, enc_noise, par, imu_log,
                             q_enc_log, qd_enc_log, est_log, feet_est_log, sigma_log, nis_log, false, gate, trust_log, stream, &ad);
}

int mpcqp_default_compensate(MpcQpCompensate* comp) {
  if (!comp) return MPCQP_EINVAL;
  memset(comp, 0, sizeof(*comp));
  comp->size = (uint32_t)sizeof(*comp);
  comp->source = MPCQP_WRENCH_TRUTH;
  comp->hold = 1;
  return mpcqp_default_wrench_observer(&comp->observer);
}

int mpcqp_rollout_observe_compensated(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                                      const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                                      const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains,
                                      int32_t leg_substeps, const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, int32_t drive,
                                      const void* ground, const void* foot_mass, double* slip, void* actual, void* desired, void* forces,
                                      void* feet_log, uint8_t* contact_log, int32_t* solved, void* swing_log, void* q_log, void* qd_log,
                                      void* tau_log, void* foot_log, void* err_log, uint8_t* flag_log, void* miss_log, void* cmd_log,
                                      double* slip_log, void* disp_log, int32_t feed, double* est_state, const void* est_init, const void* height,
                                      const void* bias, const void* noise, const void* enc_noise, const MpcQpEstimator* par, void* imu_log,
                                      void* q_enc_log, void* qd_enc_log, void* est_log, void* feet_est_log, void* sigma_log, void* nis_log,
                                      const MpcQpTrustGate* gate, void* trust_log, int32_t flags, const MpcQpAttitude* att, double* att_state,
                                      void* bias_log, const MpcQpCompensate* comp, const void* obs_body, double* dist_state, void* dist_log,
                                      void* resid_log, void* stream) {
  const char* who = "mpcqp_rollout_observe_compensated";
  if (!h) return MPCQP_EINVAL;
  MpcQpCompensate dflt;
  if (!comp) { (void)mpcqp_default_compensate(&dflt); comp = &dflt; }
  if (comp->size != sizeof(MpcQpCompensate)) return bad(h, who, "compensate struct size mismatch");
  if (comp->flags & ~(uint32_t)(MPCQP_COMP_GATED | MPCQP_COMP_AIDED)) return bad(h, who, "compensate: flags has a bit other than MPCQP_COMP_GATED and MPCQP_COMP_AIDED");
  if (comp->source != MPCQP_WRENCH_TRUTH && comp->source != MPCQP_WRENCH_SENSED)
    return bad(h, who, "compensate: source is neither MPCQP_WRENCH_TRUTH nor MPCQP_WRENCH_SENSED");
  if (comp->hold < 1) return bad(h, who, "compensate: hold must be at least 1");
  RolloutCompensateArgs cp = {comp->source, comp->hold, {}, obs_body, dist_state, dist_log, resid_log};
  if (const int rc = observer_row(h, who, &comp->observer, cp.par)) return rc;
  const RolloutSlipCall c = {B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height, gains,
                             leg_substeps, geo, inr, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log, contact_log,
                             solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log};
  const bool gated = (comp->flags & MPCQP_COMP_GATED) != 0;
  if (comp->flags & MPCQP_COMP_AIDED) {
    const EstimateAidedArgs ad = {gated ? (flags | MPCQP_AIDED_GATE) : flags, att, att_state, bias_log};
    return rollout_observe_run(h, who, c, feed, est_state, est_init, height, bias, noise, enc_noise, par, imu_log, q_enc_log, qd_enc_log, est_log,
                               feet_est_log, sigma_log, nis_log, true, gate, trust_log, stream, &ad, &cp);
  }
  return rollout_observe_run(h, who, c, feed, est_state, est_init, height, bias, noise, enc_noise, par, imu_log, q_enc_log, qd_enc_log, est_log,
                             feet_est_log, sigma_log, nis_log, gated, gate, gated ? trust_log : nullptr, stream, nullptr, &cp);
}

int mpcqp_rollout_observe_gated(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                                const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                                const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains,
                                int32_t leg_substeps, const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, int32_t drive,
                                const void* ground, const void* foot_mass, double* slip, void* actual, void* desired, void* forces,
                                void* feet_log, uint8_t* contact_log, int32_t* solved, void* swing_log, void* q_log, void* qd_log,
                                void* tau_log, void* foot_log, void* err_log, uint8_t* flag_log, void* miss_log, void* cmd_log,
                                double* slip_log, void* disp_log, int32_t feed, double* est_state, const void* est_init, const void* height,
                                const void* bias, const void* noise, const void* enc_noise, const MpcQpEstimator* par, void* imu_log,
                                void* q_enc_log, void* qd_enc_log, void* est_log, void* feet_est_log, void* sigma_log, void* nis_log,
                                const MpcQpTrustGate* gate, void* trust_log, void* stream) {
  const RolloutSlipCall c = {B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height, gains,
                             leg_substeps, geo, inr, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log, contact_log,
                             solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log};
  return rollout_observe_run(h, "mpcqp_rollout_observe_gated", c, feed, est_state, est_init, height, bias, noise, enc_noise, par, imu_log,
                             q_enc_log, qd_enc_log, est_log, feet_est_log, sigma_log, nis_log, true, gate, trust_log, stream);
}

int mpcqp_rollout_score(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* desired, const void* forces,
                        const uint8_t* contact_log, const void* tau, const void* qd, const uint8_t* flag, const void* miss,
                        const MpcQpScoreRule* rule, int32_t accumulate, double* score, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || B * (int64_t)T > 0x7fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_rollout_score: size out of range");
  if ((tau || qd || flag) && !(tau && qd && flag))
    return fail(h, MPCQP_EINVAL, "mpcqp_rollout_score: the leg group is tau, qd and flag: all three or none");
  if (B > 0 && (!score || (T > 0 && (!actual || !desired || !forces || !contact_log)))) return fail(h, MPCQP_EINVAL, "mpcqp_rollout_score: null buffer");
  const MpcQpScoreRule dflt = {(uint32_t)sizeof(MpcQpScoreRule), MPCQP_SCORE_RULE_Z_FRAC, MPCQP_SCORE_RULE_TILT_MAX};
  if (!rule) rule = &dflt;
  if (rule->size != sizeof(MpcQpScoreRule)) return fail(h, MPCQP_EINVAL, "mpcqp_rollout_score: rule struct size mismatch");
  if (!std::isfinite(rule->z_frac) || !std::isfinite(rule->tilt_max) || !(rule->z_frac > 0) || !(rule->tilt_max > 0))
    return fail(h, MPCQP_EINVAL, "mpcqp_rollout_score: z_frac and tilt_max must be finite and positive");
  // the rows are read as 16-byte vectors and dwords
  for (const void* p : {actual, desired, forces, tau, qd, miss})
    if ((uintptr_t)p % 16) return fail(h, MPCQP_EINVAL, "mpcqp_rollout_score: a log buffer is not 16-byte aligned");
  if ((uintptr_t)contact_log % 4 || (uintptr_t)flag % 4 || (uintptr_t)score % 8)
    return fail(h, MPCQP_EINVAL, "mpcqp_rollout_score: contact_log / flag not 4-byte or score not 8-byte aligned");
  if (B == 0 || (T == 0 && accumulate)) return MPCQP_OK;
  return on_device(h, "score kernel launch", [&](auto tag) {
    using TIO = decltype(tag);
    const ScoreIn<TIO> in = {(const TIO*)actual, (const TIO*)desired, (const TIO*)forces, contact_log, (const TIO*)tau, (const TIO*)qd, flag,
                             (const TIO*)miss};
    // one wave per robot
    hipLaunchKernelGGL((mpcqp_score_kernel<TIO>), blocks(B, 4), dim3(256), 0, (hipStream_t)stream, in, rule->z_frac, rule->tilt_max,
                       (int)(accumulate != 0), score, (int)B, (int)T);
  });
}

int mpcqp_default_estimator(MpcQpEstimator* par) {
  if (!par) return MPCQP_EINVAL;
  memset(par, 0, sizeof(*par));
  par->size = (uint32_t)sizeof(*par);
  par->gravity = -9.81;
  par->kappa = 2.0;
  par->q_p = 0.02; par->q_v = 0.02; par->q_f = 0.002;
  par->r_p = 0.001; par->r_v = 0.1; par->r_z = 0.001;
  par->k_swing = 100.0;
  par->p0_p = 0.01; par->p0_v = 1.0; par->p0_f = 0.01;
  return MPCQP_OK;
}

int mpcqp_imu_log(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet, const void* base_acc,
                  const void* body, const void* bias, const void* noise, const MpcQpEstimator* par, void* imu, void* stream) {
  if (!h) return MPCQP_EINVAL;
  if (B < 0 || B > 0x7fffffff || T < 0 || B * (int64_t)T > 0x1fffffff) return fail(h, MPCQP_EINVAL, "mpcqp_imu_log: size out of range");
  if (B > 0 && T > 0 && (!actual || !forces || !feet)) return fail(h, MPCQP_EINVAL, "mpcqp_imu_log: null buffer (actual, forces, feet)");
  if (B > 0 && T > 0 && !imu) return fail(h, MPCQP_EINVAL, "mpcqp_imu_log: null imu buffer");
  EstPar e;
  if (const int rc = estimator_row(h, "mpcqp_imu_log", par, e)) return rc;
  if (B == 0 || T == 0) return MPCQP_OK;
  const int64_t rows = B * T;
  return on_device(h, "imu log kernel launch", [&](auto tag) {
    using TIO = decltype(tag);
    hipLaunchKernelGGL((mpcqp_imu_log_kernel<TIO>), blocks(rows), dim3(256), 0, (hipStream_t)stream, (const TIO*)actual, (const TIO*)forces,
                       (const TIO*)base_acc, (const TIO*)body, (const TIO*)bias, (const TIO*)noise, plant_model(h), e.g, (TIO*)imu, rows,
                       (int64_t)T);
  });
}

int mpcqp_estimate_track(mpcqp_handle h, int64_t B, int32_t T, const void* imu, const void* q, const void* qd, const uint8_t* contact_log,
                         const void* trust, const void* height, const void* init, const MpcQpEstimator* par, const MpcQpLegGeometry* geo,
                         double* state, void* est, void* feet_est, void* sigma, void* nis, void* stream) {
  return estimate_track_run(h, "mpcqp_estimate_track", B, T, imu, q, qd, contact_log, trust, height, init, par, geo, state, est, feet_est,
                            sigma, nis, false, nullptr, nullptr, stream);
}

int mpcqp_default_trust_gate(MpcQpTrustGate* gate) {
  if (!gate) return MPCQP_EINVAL;
  memset(gate, 0, sizeof(*gate));
  gate->size = (uint32_t)sizeof(*gate);
  gate->d_lo = 1.0;
  gate->d_hi = 4.0;
  return MPCQP_OK;
}

int mpcqp_default_attitude(MpcQpAttitude* att) {
  if (!att) return MPCQP_EINVAL;
  memset(att, 0, sizeof(*att));
  att->size = (uint32_t)sizeof(*att);
  att->k_s = 0.0;
  att->k_v = 2.0;
  att->k_b = 5.0;
  att->b_max = 0.1;
  return MPCQP_OK;
}

int mpcqp_estimate_track_aided(mpcqp_handle h, int64_t B, int32_t T, const void* imu, const void* q, const void* qd,
                               const uint8_t* contact_log, const void* trust, const void* height, const void* init,
                               const MpcQpEstimator* par, const MpcQpLegGeometry* geo, double* state, void* est, void* feet_est, void* sigma,
                               void* nis, const MpcQpTrustGate* gate, void* trust_out, int32_t flags, const MpcQpAttitude* att,
                               double* att_state, void* bias_log, void* stream) {
  const EstimateAidedArgs ad = {flags, att, att_state, bias_log};
  return estimate_track_run(h, "mpcqp_estimate_track_aided", B, T, imu, q, qd, contact_log, trust, height, init, par, geo, state, est,
                            feet_est, sigma, nis, false, gate, trust_out, stream, &ad);
}

int mpcqp_estimate_track_gated(mpcqp_handle h, int64_t B, int32_t T, const void* imu, const void* q, const void* qd,
                               const uint8_t* contact_log, const void* trust, const void* height, const void* init,
                               const MpcQpEstimator* par, const MpcQpLegGeometry* geo, double* state, void* est, void* feet_est, void* sigma,
                               void* nis, const MpcQpTrustGate* gate, void* trust_out, void* stream) {
  return estimate_track_run(h, "mpcqp_estimate_track_gated", B, T, imu, q, qd, contact_log, trust, height, init, par, geo, state, est,
                            feet_est, sigma, nis, true, gate, trust_out, stream);
}

int mpcqp_last_kernel_ms(mpcqp_handle h, float* ms) {
  if (!h || !ms) return MPCQP_EINVAL;
  if (h->cfg.flags & MPCQP_FLAG_NO_TIMING) return fail(h, MPCQP_EINVAL, "mpcqp_last_kernel_ms: the handle was created with MPCQP_FLAG_NO_TIMING");
  if (!h->timed) return fail(h, MPCQP_EINVAL, "mpcqp_last_kernel_ms: no solve recorded");
  DeviceGuard guard(h->cfg.device);
  hipError_t he = hipEventSynchronize(h->ev1);
  if (he == hipSuccess) he = hipEventElapsedTime(ms, h->ev0, h->ev1);
  if (he != hipSuccess) return fail(h, MPCQP_EHIP, "hipEventElapsedTime", he);
  return MPCQP_OK;
}

#if defined(MPCQP_STAMPS) || defined(MPCQP_TIMELINE)
extern "C" int mpcqp_debug_read_timeline(unsigned long long* out, int64_t B) {
  if (B > 65536) return MPCQP_EINVAL;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_timeline), (size_t)B * 3 * sizeof(unsigned long long)) == hipSuccess ? MPCQP_OK : MPCQP_EHIP;
}
#endif
#if defined(MPCQP_STAMPS) || defined(MPCQP_WDBG)
int mpcqp_debug_read_wdbg(double* out2048) {
  if (hipDeviceSynchronize() != hipSuccess) return MPCQP_EHIP;
  return hipMemcpyFromSymbol(out2048, HIP_SYMBOL(g_wdbg), 2048 * sizeof(double)) == hipSuccess ? MPCQP_OK : MPCQP_EHIP;
}
#endif
#ifdef MPCQP_STAMPS
// diagnostic build only: read and reset the phase counters
int mpcqp_debug_read_stamps(unsigned long long* out32) {
  unsigned long long z[32] = {0};
  if (hipDeviceSynchronize() != hipSuccess) return MPCQP_EHIP;
  if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_stamps), sizeof(z)) != hipSuccess) return MPCQP_EHIP;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z)) != hipSuccess) return MPCQP_EHIP;
  return MPCQP_OK;
}
#endif

}  // extern "C"
