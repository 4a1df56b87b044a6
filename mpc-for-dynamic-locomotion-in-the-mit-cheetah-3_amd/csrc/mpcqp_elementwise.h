// mpcqp_elementwise.h -- the element-wise kernels around the solve that are neither plan (mpcqp_plan.h) nor plant (mpcqp_plant.h):
// torque map, leg kinematics, gait-descriptor expansion and the closed-loop roll-out's expand / advance.  All HBM- or launch-bound,
// one thread per output element or per robot; their entry points are in mpcqp_kernels.hip (C-ABI include/mpcqp.h, mpcqp_sim.h).
#pragma once
#include "mpcqp_common.h"
#include "mpcqp_plan.h"
#include "mpcqp_plant.h"
#include "mpcqp_gaits.h"

namespace {

// tau[b][l] = J[b][l]^T (-f[b][l]) for the four legs of stage 0 (src/main.py:212-214).  Element-wise, HBM-bound:
// one thread per (robot, leg), 9 + 3 loads and 3 stores; consecutive threads touch consecutive 48 / 12-byte records.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_torque_kernel(const TIO* __restrict__ u, const TIO* __restrict__ jac, TIO* __restrict__ tau, const int64_t B, const int N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // i = 4 b + leg
  if (i >= 4 * B) return;
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  const TIO* f = u + b * N * 12 + 3 * l;       // stage-0 force of this leg
  const TIO* J = jac + i * 9;                  // 3x3, row-major, world-frame linear Jacobian block of the leg
  const TIO fx = -f[0], fy = -f[1], fz = -f[2];
#pragma unroll
  for (int q = 0; q < 3; ++q) tau[i * 3 + q] = J[0 * 3 + q] * fx + J[1 * 3 + q] * fy + J[2 * 3 + q] * fz;
}

// Leg kinematics (src/main.py:205-210 asks DART for these): foot position and d foot / d q of one leg from its three joint angles,
// by composing the joint rotations (Rodrigues' formula about the geometry's axes) along the chain torso -> HipX -> HipY -> Knee -> foot.
// One thread per (robot, leg): 3 (+9) loads, 9 (+3) stores, three sincos; fp64 arithmetic for either buffer type (the kernel is
// launch- and HBM-latency sized: 48 B in, 108 B out per thread).
struct LegGeoDev { double hx[4][3], hy[4][3], kn[3], ft[3], ax[3], ay[3]; };

__device__ __forceinline__ void rodrigues(const double (&a)[3], const double ang, double (&R)[9]) {
  double s, c;
  sincos(ang, &s, &c);
  const double t = 1.0 - c;
  R[0] = c + t * a[0] * a[0];        R[1] = t * a[0] * a[1] - s * a[2]; R[2] = t * a[0] * a[2] + s * a[1];
  R[3] = t * a[1] * a[0] + s * a[2]; R[4] = c + t * a[1] * a[1];        R[5] = t * a[1] * a[2] - s * a[0];
  R[6] = t * a[2] * a[0] - s * a[1]; R[7] = t * a[2] * a[1] + s * a[0]; R[8] = c + t * a[2] * a[2];
}
__device__ __forceinline__ void mat3_mul(const double (&A)[9], const double (&Bm)[9], double (&C)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * Bm[j] + A[3 * i + 1] * Bm[3 + j] + A[3 * i + 2] * Bm[6 + j];
}
__device__ __forceinline__ void mat3_vec(const double (&A)[9], const double (&v)[3], double (&o)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}
__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// The forward map of leg l in the torso frame: foot position pf relative to the torso origin and J = d pf / d q, row-major
// (row = axis, column = joint).  Shared by mpcqp_leg_jacobian_kernel and the joint-space log (mpcqp_joints.h).
__device__ __forceinline__ void leg_fk_jac(const LegGeoDev& geo, const int l, const double (&q)[3], double (&pf)[3], double (&J)[9]) {
  double R1[9], Ry[9], R2[9], R3[9];
  rodrigues(geo.ax, q[0], R1);
  rodrigues(geo.ay, q[1], Ry);
  mat3_mul(R1, Ry, R2);
  rodrigues(geo.ay, q[2], Ry);
  mat3_mul(R2, Ry, R3);
  double hx[3], hy[3], p2[3], p3[3], t[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { hx[a] = geo.hx[l][a]; hy[a] = geo.hy[l][a]; }   // (leg-indexed: a scalar-indexed copy per lane)
  mat3_vec(R1, hy, t);
#pragma unroll
  for (int a = 0; a < 3; ++a) p2[a] = hx[a] + t[a];
  mat3_vec(R2, geo.kn, t);
#pragma unroll
  for (int a = 0; a < 3; ++a) p3[a] = p2[a] + t[a];
  mat3_vec(R3, geo.ft, t);
#pragma unroll
  for (int a = 0; a < 3; ++a) pf[a] = p3[a] + t[a];
  double w[3], dlt[3], col[3];   // column j = (joint axis in the torso frame) x (foot - joint origin)
  mat3_vec(R1, geo.ax, w);
#pragma unroll
  for (int a = 0; a < 3; ++a) dlt[a] = pf[a] - hx[a];
  cross3(w, dlt, col);
#pragma unroll
  for (int a = 0; a < 3; ++a) J[3 * a] = col[a];
  mat3_vec(R2, geo.ay, w);
#pragma unroll
  for (int a = 0; a < 3; ++a) dlt[a] = pf[a] - p2[a];
  cross3(w, dlt, col);
#pragma unroll
  for (int a = 0; a < 3; ++a) J[3 * a + 1] = col[a];
  mat3_vec(R3, geo.ay, w);
#pragma unroll
  for (int a = 0; a < 3; ++a) dlt[a] = pf[a] - p3[a];
  cross3(w, dlt, col);
#pragma unroll
  for (int a = 0; a < 3; ++a) J[3 * a + 2] = col[a];
}

template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_leg_jacobian_kernel(const TIO* __restrict__ q, const TIO* __restrict__ rot, const LegGeoDev geo, TIO* __restrict__ jac,
                          TIO* __restrict__ foot, const int64_t B) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // i = 4 b + leg
  if (i >= 4 * B) return;
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  const double ql[3] = {(double)q[3 * i], (double)q[3 * i + 1], (double)q[3 * i + 2]};
  double pf[3], J[9];
  leg_fk_jac(geo, l, ql, pf, J);
  if (rot) {   // world <- torso
    double Rb[9], Jw[9], pw[3];
#pragma unroll
    for (int a = 0; a < 9; ++a) Rb[a] = (double)rot[9 * b + a];
    mat3_mul(Rb, J, Jw);
    mat3_vec(Rb, pf, pw);
#pragma unroll
    for (int a = 0; a < 9; ++a) J[a] = Jw[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) pf[a] = pw[a];
  }
#pragma unroll
  for (int a = 0; a < 9; ++a) jac[9 * i + a] = (TIO)J[a];
  if (foot) {
#pragma unroll
    for (int a = 0; a < 3; ++a) foot[3 * i + a] = (TIO)pf[a];
  }
}

// ------------------------------------------------------------------------------------------- expansion into an operator tuple
// What MPC.solve computes on the host every tick (src/mpc.py:178-254) from the planner queries (src/footstep_planner.py:226-246),
// for B robots at once, into the engine's own tuple workspace:
//   x_des[k]   = [roll0, pitch0, yaw_start + k d w, com_start + k d v, 0, 0, w, v, g]             (src/mpc.py:202-214)
//   contact[k] = feet_id[step(k)] during that step's first ss ticks, else all stance          (footstep_planner.py:239-246)
//   r[0]       = measured foot - measured com;  r[k>=1] = planned foothold of step(k) - x_des com(k)   (src/mpc.py:218-239)
// with step(k) from the plan clock (mpcqp_plan.h).  Both expand kernels are element-wise and HBM-bound (about 100 B in, 1.1 KB out
// per QP at N = 10, which the solve kernel then reads from L2): one thread per output element, consecutive threads write
// consecutive addresses.  They share the element arithmetic of mpcqp_common.h (xdes_elem, lever_elem) with the expansion of a per-leg
// gait (mpcqp_gaits.h) and differ in where the rows and the clock come from.

// Leg l of the step row `fid` carries force at a tick: the step's own pattern during single support, every foot after it.
__device__ __forceinline__ bool in_stance(const PlanClock<int>& c, const uint8_t* fid, const int l) { return c.swing ? fid[l] != 0 : true; }

// Gait entry point (mpcqp_solve_batch_gait): the clock is the descriptor gait[b] = t_in_step, ss, ds over the S described steps of the
// call (past the last one: that step with its time running on, all feet in stance -- the planner's clamp,
// src/footstep_planner.py:226-237); the stage-0 feet are the measured ones.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_gait_expand_kernel(const FastIn<TIO> in, const double d, const int N, const int S, const int64_t B, TIO* __restrict__ r,
                         uint8_t* __restrict__ contact, TIO* __restrict__ xdes) {
  const int nx = (N + 1) * 13, nr = N * 12, per = nx + nr;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * per) return;
  const int64_t b = t / per;
  const int e = (int)(t - b * per);
  const TIO* ref = in.ref + b * 10;
  const TIO* x0 = in.x0 + b * 13;
  if (e < nx) {
    xdes[b * nx + e] = (TIO)xdes_elem(ref, x0[12], e / 13, e % 13, d, 1.0);
  } else {
    const int i = e - nx, k = i / 12, l = (i % 12) / 3, a = i % 3;
    const int32_t* g = in.gait + b * 4;
    const PlanClock<int> c = plan_clock(S, g[1], g[2], S, max(g[0], 0) + k);
    const TIO foot = k == 0 ? in.feet0[b * 12 + l * 3 + a] : in.footholds[((b * S + c.step) * 4 + l) * 3 + a];
    r[b * nr + i] = (TIO)lever_elem(foot, ref, x0, k, a, d, 1.0);
    if (a == 0) contact[b * (N * 4) + k * 4 + l] = in_stance(c, in.feet_id + (b * S + c.step) * 4, l) ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------- closed-loop roll-out
// mpcqp_rollout: B robots advance T control ticks on the device.  Per tick, per robot -- what
// Lite3Controller.customPreStep / MPC.solve do on the host (src/main.py:130-188, src/mpc.py:176-271):
//   expand   x_des from the rolled-forward reference (src/mpc.py:202-214, velocities zeroed on the last plan step, :178-183),
//            contact masks and planned footholds from the robot's plan table (src/footstep_planner.py:226-246), lever arms
//            (src/mpc.py:218-239; stance feet stand on the plan, swing feet carry no force)
//   solve    the batched QP, warm-started from the previous tick when the engine was created with the warm-start flags
//   advance  the world step (below), com_start += v d, yaw_start += w d (src/mpc.py:261-262), tick += 1,
//            log the tick's actual / desired state and stage-0 forces (the log's TRACKING PERFORMANCE / FORCES, src/logger.py:22-46)
// pos [B,S,4,3], feet_id [B,S,4], meta [B,4] = S, ss, ds, reserved
template <typename TIO>
struct RolloutPlan { const TIO* pos; const uint8_t* feet_id; const int32_t* meta; };

template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_rollout_expand_kernel(const TIO* __restrict__ x, const TIO* __restrict__ ref, const RolloutPlan<TIO> plan,
                            const int32_t* __restrict__ tick, const double d, const int N, const int Smax, const int64_t B,
                            TIO* __restrict__ r, uint8_t* __restrict__ contact, TIO* __restrict__ xdes) {
  const int nx = (N + 1) * 13, nr = N * 12, per = nx + nr;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * per) return;
  const int64_t b = t / per;
  const int e = (int)(t - b * per);
  const TIO* rf = ref + b * 10;
  const TIO* xb = x + b * 13;
  const int t0 = max(tick[b], 0);
  const double gate = plan_clock(plan.meta + b * 4, Smax, t0).gate;   // src/mpc.py:181-183: references zeroed on the last plan step
  if (e < nx) {
    xdes[b * nx + e] = (TIO)xdes_elem(rf, xb[12], e / 13, e % 13, d, gate);
  } else {
    const int i = e - nx, k = i / 12, l = (i % 12) / 3, a = i % 3;
    const PlanClock<int> c = plan_clock(plan.meta + b * 4, Smax, t0 + k);   // past the plan: the last step, all stance
    const TIO* pos = plan.pos + ((b * Smax + c.step) * 4 + l) * 3;
    r[b * nr + i] = (TIO)lever_elem(pos[a], rf, xb, k, a, d, gate);
    if (a == 0) contact[b * (N * 4) + k * 4 + l] = in_stance(c, plan.feet_id + (b * Smax + c.step) * 4, l) ? 1 : 0;
  }
}

// The world step of the advance: what turns the tick's solve into the next measured state.
//   ModelWorld  x <- X[:,1], the model's own prediction (mpcqp_rollout; the kinematic stand-in of the plumbing tests)
//   PlantIn     one tick of the rigid-body plant (mpcqp_plant.h) under the stage-0 forces, with the expand kernel's stage-0 stance
//               feet and contact and the robot's push inside its tick window (mpcqp_rollout_plant)
template <typename TIO>
struct ModelWorld { const TIO* X; };

template <typename TIO>
__device__ __forceinline__ void world_step(const ModelWorld<TIO>& w, TIO* x, const TIO* u0, const RolloutPlan<TIO>& plan,
                                           const PlanClock<int>& c, const int64_t b, const int N, const int Smax, const int tk) {
  for (int i = 0; i < 12; ++i) x[i] = w.X[((size_t)b * (N + 1) + 1) * 13 + i];
}

// One plant tick of robot b at its tick tk: stage-0 forces u0, feet pos [4,3] and stance mask st of the tick, the robot's body row and
// its push inside the window.
template <typename TIO>
__device__ __forceinline__ void plant_world_step(const PlantIn<TIO>& pin, TIO* x, const TIO* u0, const TIO* pos, const bool (&st)[4],
                                                 const int64_t b, const int tk) {
  double xs[13], fs[12], ft[12], bd[7], wr[6], out[13];
#pragma unroll
  for (int i = 0; i < 13; ++i) xs[i] = (double)x[i];
#pragma unroll
  for (int i = 0; i < 12; ++i) { fs[i] = (double)u0[i]; ft[i] = (double)pos[i]; }
  plant_body_row(pin.body, pin.model, b, bd);
  const bool pushed = pin.push && pin.push_ticks[2 * b] <= tk && tk < pin.push_ticks[2 * b + 1];
#pragma unroll
  for (int i = 0; i < 6; ++i) wr[i] = pushed ? (double)pin.push[b * 6 + i] : 0.0;
  plant_tick(xs, fs, ft, st, bd, wr, pin.n, pin.h, out);
#pragma unroll
  for (int i = 0; i < 13; ++i) x[i] = (TIO)out[i];
}

template <typename TIO>
__device__ __forceinline__ void world_step(const PlantIn<TIO>& pin, TIO* x, const TIO* u0, const RolloutPlan<TIO>& plan,
                                           const PlanClock<int>& c, const int64_t b, const int N, const int Smax, const int tk) {
  bool st[4];
  const uint8_t* fid = plan.feet_id + (b * Smax + c.step) * 4;
#pragma unroll
  for (int l = 0; l < 4; ++l) st[l] = in_stance(c, fid, l);
  plant_world_step(pin, x, u0, plan.pos + (b * Smax + c.step) * 12, st, b, tk);
}

// What every advance kernel does around its world step.  advance_log: the tick's log rows and the `solved` count, before the state
// moves; advance_ref: the reference roll-forward after it.
template <typename TIO>
__device__ __forceinline__ void advance_log(const TIO* xb, const TIO* rf, const TIO* u0, const int st, const double gate, const size_t row,
                                            const int it, const int64_t b, TIO* __restrict__ actual, TIO* __restrict__ desired,
                                            TIO* __restrict__ forces, int32_t* __restrict__ solved) {
  if (actual) for (int i = 0; i < 12; ++i) actual[row + i] = xb[i];                               // logger.log_tracking_data (src/mpc.py:295)
  if (desired) {
    const TIO des[12] = {rf[0], rf[1], rf[2], rf[3], rf[4], rf[5], (TIO)0, (TIO)0, (TIO)(gate * (double)rf[9]),
                         (TIO)(gate * (double)rf[6]), (TIO)(gate * (double)rf[7]), (TIO)(gate * (double)rf[8])};
    for (int i = 0; i < 12; ++i) desired[row + i] = des[i];
  }
  if (forces) for (int i = 0; i < 12; ++i) forces[row + i] = u0[i];                               // src/main.py:216-218
  if (solved) solved[b] = (it == 0 ? 0 : solved[b]) + ((st == MPCQP_STATUS_SOLVED_POLISHED || st == MPCQP_STATUS_SOLVED_ADMM) ? 1 : 0);
}

template <typename TIO>
__device__ __forceinline__ void advance_ref(TIO* rf, const double gate, const double d) {
  for (int a = 0; a < 3; ++a) rf[3 + a] = (TIO)((double)rf[3 + a] + gate * (double)rf[6 + a] * d);   // src/mpc.py:261
  rf[2] = (TIO)((double)rf[2] + gate * (double)rf[9] * d);                                      // src/mpc.py:262
}

// The roll-out's third launch per tick, one thread per robot: log rows, `solved` count, world step, reference roll-forward, tick.
template <typename TIO, typename World>
__global__ void __launch_bounds__(256)
mpcqp_rollout_advance_kernel(TIO* __restrict__ x, TIO* __restrict__ ref, const RolloutPlan<TIO> plan, int32_t* __restrict__ tick,
                             const World world, const TIO* __restrict__ u, const int32_t* __restrict__ status, const double d, const int N,
                             const int64_t B, const int T, const int it, const int Smax, TIO* __restrict__ actual,
                             TIO* __restrict__ desired, TIO* __restrict__ forces, int32_t* __restrict__ solved) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  TIO* rf = ref + b * 10;
  TIO* xb = x + b * 13;
  const TIO* u0 = u + (size_t)b * N * 12;
  const int tk = tick[b];
  const PlanClock<int> c = plan_clock(plan.meta + b * 4, Smax, max(tk, 0));
  const double gate = c.gate;
  advance_log(xb, rf, u0, status[b], gate, ((size_t)b * T + it) * 12, it, b, actual, desired, forces, solved);
  world_step(world, xb, u0, plan, c, b, N, Smax, tk);
  advance_ref(rf, gate, d);
  tick[b] = tk + 1;
}

// The advance of mpcqp_rollout_phase: the gait clock (mpcqp_gaits.h) in place of the plan table, the robot's feet as state.  After the
// plant tick every leg that touches down at the new tick gets its foothold from the measured state -- the state as stored, so that the
// log replays: CoM, velocity, yaw = atan2(R10, R00) of the plant's own rotation-vector conversion.  Every other foot is not written.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_phase_advance_kernel(TIO* __restrict__ x, TIO* __restrict__ ref, TIO* feet, const PhaseRows<TIO> ph, int32_t* __restrict__ tick,
                           const PlantIn<TIO> pin, const TIO* __restrict__ u, const int32_t* __restrict__ status, const double d, const int N,
                           const int64_t B, const int T, const int it, TIO* __restrict__ actual, TIO* __restrict__ desired,
                           TIO* __restrict__ forces, TIO* __restrict__ feet_log, uint8_t* __restrict__ contact_log,
                           int32_t* __restrict__ solved) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  TIO* rf = ref + b * 10;
  TIO* xb = x + b * 13;
  TIO* ft = feet + b * 12;
  const TIO* u0 = u + (size_t)b * N * 12;
  const int tk = tick[b];
  const GaitLeg c[4] = {gait_leg(ph.gait + b * GAIT_ROW, 0), gait_leg(ph.gait + b * GAIT_ROW, 1), gait_leg(ph.gait + b * GAIT_ROW, 2),
                        gait_leg(ph.gait + b * GAIT_ROW, 3)};
  advance_log(xb, rf, u0, status[b], 1.0, ((size_t)b * T + it) * 12, it, b, actual, desired, forces, solved);
  bool st[4];
#pragma unroll
  for (int l = 0; l < 4; ++l) st[l] = gait_phase(c[l], (uint32_t)max(tk, 0)) < c[l].st;
  if (feet_log) for (int i = 0; i < 12; ++i) feet_log[((size_t)b * T + it) * 12 + i] = ft[i];
  if (contact_log) for (int l = 0; l < 4; ++l) contact_log[((size_t)b * T + it) * 4 + l] = st[l] ? 1 : 0;
  plant_world_step(pin, xb, u0, ft, st, b, tk);
  advance_ref(rf, 1.0, d);
  tick[b] = tk + 1;
  const uint32_t tn = tk < 0 ? 0u : (uint32_t)tk + 1u;
  bool td[4], any = false;
#pragma unroll
  for (int l = 0; l < 4; ++l) { td[l] = gait_steps(c[l]) && gait_phase(c[l], tn) == 0; any = any || td[l]; }
  if (!any) return;
  double q[4], sn, cs;
  plant_rotvec_to_quat((double)xb[0], (double)xb[1], (double)xb[2], q);
  {
#pragma clang fp contract(off)
    sincos(atan2(2.0 * (q[1] * q[2] + q[0] * q[3]), 1.0 - 2.0 * (q[2] * q[2] + q[3] * q[3])), &sn, &cs);
  }
  const double gain = ph.gain ? (double)ph.gain[b] : 0.0;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    if (!td[l]) continue;
    const TIO* s = ph.stand + b * 12 + l * 3;
    for (int a = 0; a < 2; ++a)
      ft[3 * l + a] = (TIO)gait_foothold_xy(a, (double)xb[3 + a], cs, sn, (double)s[0], (double)s[1], (double)xb[9 + a], (double)rf[6 + a],
                                            gait_half_stance(c[l], d), gain);
    ft[3 * l + 2] = s[2];
  }
}

}  // namespace
