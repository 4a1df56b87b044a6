// mpcqp_drive.h -- what a stance leg delivers: the commanded foot force through the actuators' torque limits and the ground (the
// C-ABI is mpcqp_stance_drive and mpcqp_rollout_drive in include/mpcqp_sim.h, which has the rule; the entry points live in
// mpcqp_kernels.hip).  Two kernels:
//   mpcqp_stance_drive_kernel  the rule for one (robot, leg).  mpcqp_stance_drive runs it on the caller's rows; mpcqp_rollout_drive runs
//                              the SAME instantiation per tick on the live buffers, between the solve and the legs step: the commanded
//                              force is stage 0 of the solve's [B,N,12] buffer (stride fstride), the stance mask the gait clock's at
//                              max(tick, 0) (contact = null), and the applied force goes to a [B,12] side buffer of the roll-out's
//                              reserve.  The legs step and the advance then read that side buffer as a force buffer of horizon 1, so they
//                              keep their source and their assembly, and the solver's own buffer -- its next warm start -- is not altered.
//   mpcqp_drive_log_kernel     after the legs step of a tick: on stance rows tau_log becomes the rule's torque and flag_log gains the
//                              rule's bits 2 / 16 / 32 (0xff for a poisoned leg).
// One kernel for both entry points is what makes the roll-out's logs replay bit for bit through mpcqp_stance_drive.
//
// The rule is written once, here, for a held foot and for a sliding one (mpcqp_slip.h): the stance mask (stance_mask), steps 2 and 3
// (drive_force), step 5 (drive_torque), the common stores (drive_store) and the log step (drive_log_step).  A kernel reads: row,
// drive_force, its own step 4 -- drive_cone here, slip_slide there --, drive_torque, its poison test, stores.  The row and the poison
// test are lines of the two kernels, not functions: the kernels say why.
//
// Layout as mpcqp_legdyn.h states it: one thread per (robot, leg), a robot's four legs in one quad, fp64 arithmetic, no LDS, geometry
// and limits by value.  q and tau_cmd = (R J)^T (-f) are leg_joints<true>'s, the device function of mpcqp_joint_log, with R formed as
// that kernel forms it; J is leg_fk_jac's at that q; the 3x3 solve is adj_solve (cofactors and determinant in the order the rates
// solve J) on J^T.  The rule's own arithmetic runs without contraction.  Masks are selects: a poisoned leg computes on and is selected
// away at the store; no lane returns early and nothing is exchanged between lanes.
#pragma once
#include "mpcqp_gaits.h"
#include "mpcqp_joints.h"
#include "mpcqp_legsim.h"

namespace {

constexpr int DRIVE_IDEAL = 0, DRIVE_LIMITED = 1;   // MPCQP_DRIVE_IDEAL, MPCQP_DRIVE_LIMITED (include/mpcqp_sim.h)
constexpr unsigned DRIVE_BITS = 2u | 16u | 32u;     // what the rule adds to a stance row's flag

// Is leg l of robot b (i = 4 b + l) in stance: contact u8 [B,4], or null: the gait clock of `gait` [B,9] at max(tick[b], 0).
__device__ __forceinline__ bool stance_mask(const uint8_t* __restrict__ contact, const int32_t* __restrict__ gait,
                                            const int32_t* __restrict__ tick, const int64_t i, const int64_t b, const int l) {
  if (contact) return contact[i] != 0;
  const GaitLeg gc = gait_leg(gait + b * GAIT_ROW, l);
  return gait_phase(gc, (uint32_t)max(tick[b], 0)) < gc.st;
}

// Steps 2 and 3 of the rule: the applied torque ta, the force f1 it delivers; returns the bits 2 / 16.
// ACT: step 2 is the envelope of the actuator row `ar` at the joint rates qr, not the box of lim.taumax.
template <bool ACT>
__device__ __forceinline__ unsigned drive_force(const double (&R)[9], const double (&J)[9], const bool reach, const V3 f, const V3 tc,
                                                const LegLimDev& lim, const bool limited, V3& ta, V3& f1,
                                                const double* __restrict__ ar, const V3 qr) {
#pragma clang fp contract(off)
  // 2. the actuators
  if constexpr (ACT)
    ta = {limited ? act_clamp(ar, 0, tc.x, qr.x) : tc.x, limited ? act_clamp(ar, 1, tc.y, qr.y) : tc.y,
          limited ? act_clamp(ar, 2, tc.z, qr.z) : tc.z};
  else
    ta = {limited ? clamp_sym(tc.x, lim.taumax[0]) : tc.x, limited ? clamp_sym(tc.y, lim.taumax[1]) : tc.y,
          limited ? clamp_sym(tc.z, lim.taumax[2]) : tc.z};
  const bool clamped = ta.x != tc.x || ta.y != tc.y || ta.z != tc.z;
  // 3. f1 = -A^-1 tau_app, A = (R J)^T = J^T R^T: g = J^-T tau_app, f1 = -(R g)
  const M3 Jt = {{J[0], J[3], J[6]}, {J[1], J[4], J[7]}, {J[2], J[5], J[8]}};
  double det;
  const V3 g = adj_solve(Jt, ta, det);
  const V3 fc = {-((R[0] * g.x + R[1] * g.y) + R[2] * g.z), -((R[3] * g.x + R[4] * g.y) + R[5] * g.z), -((R[6] * g.x + R[7] * g.y) + R[8] * g.z)};
  const bool solve = reach && det != 0.0;
  f1 = sel3(clamped && solve, fc, f);
  return (clamped ? 2u : 0u) | ((clamped && !solve) ? 16u : 0u);
}

// Step 4 for a held foot, the ground: no pull, and the tangential part on the circular cone (cone_on; mu the ground's friction) with
// its direction kept.  Returns f2 by value: the caller selects it where it differs from f1.
__device__ __forceinline__ V3 drive_cone(const V3 f1, const bool cone_on, const double mu) {
#pragma clang fp contract(off)
  const bool pull = f1.z <= 0.0;
  const double ft = sqrt(f1.x * f1.x + f1.y * f1.y), cap = mu * f1.z;
  const bool cone = cone_on && ft > cap;
  const double s = cap / ft;
  return {pull ? 0.0 : (cone ? f1.x * s : f1.x), pull ? 0.0 : (cone ? f1.y * s : f1.y), pull ? 0.0 : f1.z};
}

// Step 5, the torque that goes with f2: (R J)^T (-f2) where the ground changed the force (`changed`), the applied torque ta where it
// did not.
__device__ __forceinline__ V3 drive_torque(const double (&R)[9], const double (&J)[9], const V3 f2, const bool changed, const V3 ta) {
#pragma clang fp contract(off)
  const double h0 = -((R[0] * f2.x + R[3] * f2.y) + R[6] * f2.z), h1 = -((R[1] * f2.x + R[4] * f2.y) + R[7] * f2.z),
               h2 = -((R[2] * f2.x + R[5] * f2.y) + R[8] * f2.z);   // R^T (-f2)
  const V3 tg = {(J[0] * h0 + J[3] * h1) + J[6] * h2, (J[1] * h0 + J[4] * h1) + J[7] * h2, (J[2] * h0 + J[5] * h1) + J[8] * h2};
  return sel3(changed, tg, ta);
}

// The stores of leg i = 4 b + l: the commanded force as read to cmd (or null), then f_out, tau (or null) and flag (or null).  A swing
// leg keeps its commanded force as read, with no torque and no bits; a leg that is not `good` gets NaN and 0xff.
template <typename TIO>
__device__ __forceinline__ void drive_store(const int64_t i, const int64_t b, const int l, const TIO (&fr)[3], const bool good,
                                            const bool stance, const V3 fo, const V3 to, const unsigned bits, TIO* f_out,
                                            TIO* __restrict__ tau, uint8_t* __restrict__ flag, TIO* __restrict__ cmd, const int64_t cstride) {
  const double nan = __builtin_nan("");
  const V3 zero = {0.0, 0.0, 0.0};
  TIO* fw = f_out + 12 * b + 3 * l;
  if (cmd) {
    TIO* cw = cmd + b * cstride + 3 * l;
    cw[0] = fr[0]; cw[1] = fr[1]; cw[2] = fr[2];
  }
  fw[0] = good ? (stance ? (TIO)fo.x : fr[0]) : (TIO)nan;
  fw[1] = good ? (stance ? (TIO)fo.y : fr[1]) : (TIO)nan;
  fw[2] = good ? (stance ? (TIO)fo.z : fr[2]) : (TIO)nan;
  if (tau) store3(tau + 3 * i, good, sel3(stance, to, zero));
  if (flag) flag[i] = good ? (uint8_t)(stance ? bits : 0u) : (uint8_t)0xff;
}

// i = 4 b + leg.  x [B,13]; f the commanded forces, robot b's at f + b fstride; feet [B,4,3]; contact u8 [B,4], or null: the gait
// clock of `gait` [B,9] at max(tick[b], 0); ground [B] or null.  f_out [B,12] (may be f when fstride = 12: a lane reads its own three
// values before it writes them), tau [B,4,3] or null, flag u8 [B,4] or null, cmd or null: robot b's commanded forces as read, to
// cmd + b cstride.
// ACTROW (act_rows, mpcqp_actuators.h) is empty, or double: mpcqp_stance_drive_kernel<TIO, double> is the kernel with an actuator
// table set (include/mpcqp_actuators.h) and takes it, act [B,9], as one more argument; lim.taumax is then not read, and the joint
// rates with the foot at rest in the world, J^-1 R^T (-v - omega x (foot - c)) from x[6..11] by leg_joints<true, true> (0 out of
// reach or where det J = 0), enter the envelope of row b of the table.
template <typename TIO, typename... ACTROW>
__global__ void __launch_bounds__(256)
mpcqp_stance_drive_kernel(const TIO* __restrict__ x, const TIO* f, const int64_t fstride, const TIO* __restrict__ feet,
                          const uint8_t* __restrict__ contact, const int32_t* __restrict__ gait, const int32_t* __restrict__ tick,
                          const TIO* __restrict__ ground, const LegGeoDev geo, const LegLimDev lim, const int drive, TIO* f_out,
                          TIO* __restrict__ tau, uint8_t* __restrict__ flag, TIO* __restrict__ cmd, const int64_t cstride, const int64_t B,
                          const ACTROW* __restrict__... actp) {
  constexpr bool ACT = sizeof...(ACTROW) != 0;
  const double* const act = act_rows(actp...);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  const TIO* xb = x + 13 * b;   // rotation vector, CoM, ...
  const TIO* fb = f + b * fstride + 3 * l;
  const TIO fr[3] = {fb[0], fb[1], fb[2]};
  const bool stance = stance_mask(contact, gait, tick, i, b, l);
  // mpcqp_joint_log's row: R from the rotation vector, the foot seen from the CoM, q and tau_cmd (in the kernel, as in the slip kernel: in a
  // function of their own these lines, which run with contraction, are fused differently and the results move in the last place)
  double qt[4], pw[3], fl[3], ql[3], tl[3];
  plant_rotvec_to_quat((double)xb[0], (double)xb[1], (double)xb[2], qt);
  const double qw = qt[0], qx = qt[1], qy = qt[2], qz = qt[3];
  const double R[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                       2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                       2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    pw[a] = (double)feet[3 * i + a] - (double)xb[3 + a];
    fl[a] = (double)fr[a];
  }
  bool reach;
  V3 rate = {0.0, 0.0, 0.0};
  if constexpr (ACT) {
    const double om[3] = {(double)xb[6], (double)xb[7], (double)xb[8]};
    double wxr[3], vr[3], qr[4];
    cross3(om, pw, wxr);
#pragma unroll
    for (int a = 0; a < 3; ++a) vr[a] = (0.0 - (double)xb[9 + a]) - wxr[a];
    reach = leg_joints<true, true>(geo, l, R, pw, fl, ql, tl, vr, qr);
    rate = {qr[0], qr[1], qr[2]};
  } else {
    reach = leg_joints<true>(geo, l, R, pw, fl, ql, tl);
  }
  double pf[3], J[9];
  leg_fk_jac(geo, l, ql, pf, J);
  const V3 fv = {fl[0], fl[1], fl[2]}, tc = {tl[0], tl[1], tl[2]}, q = {ql[0], ql[1], ql[2]}, zero = {0.0, 0.0, 0.0};
  const double mu = ground ? (double)ground[b] : 0.0;
  V3 ta, f1;
  unsigned bits = drive_force<ACT>(R, J, reach, fv, tc, lim, drive == DRIVE_LIMITED, ta, f1, ACT ? act + ACT_ROW * b : nullptr, rate);
  const V3 f2 = drive_cone(f1, ground != nullptr, mu);
  const bool changed = f2.x != f1.x || f2.y != f1.y || f2.z != f1.z;   // the ground changed the force
  const V3 fo = sel3(changed, f2, f1);   // (a select: an untouched force keeps its bits, a -0 included)
  const V3 to = drive_torque(R, J, f2, changed, ta);
  bits |= (changed ? 32u : 0u) | swing_limits(lim, q, zero);   // 4: q outside its limits
  // the robot's x and ground row poison its four legs, a leg's own operands that leg (in the kernel, not in a function shared with the
  // slip kernel: there the twelve x values stay in registers to the end, and three of the eight stance kernels lose a wave per SIMD)
  bool robot = isfinite(mu) && mu >= 0.0;
#pragma unroll
  for (int a = 0; a < 12; ++a) robot = robot && isfinite((double)xb[a]);
  const bool good = robot && (!stance || (fin3(fv) && isfinite(pw[0]) && isfinite(pw[1]) && isfinite(pw[2]) && fin3(fo) && fin3(to)));
  drive_store(i, b, l, fr, good, stance, fo, to, bits, f_out, tau, flag, cmd, cstride);
}

// The log step of stance leg i = 4 b + l, whose row of the logs is il: rtau [B,4,3] and rflag [B,4] are what the stance kernel left
// for this tick.  A row the legs step poisoned (tau NaN, flag 0xff) keeps what it logged; with only_changed so does a row without a
// bit of `mask` in rflag (0xff has the bits); any other gets the rule's torque and its bits of `mask`, or 0xff for a poisoned leg.
template <typename TIO>
__device__ __forceinline__ void drive_log_step(const int64_t i, const int64_t il, const TIO* __restrict__ rtau,
                                               const uint8_t* __restrict__ rflag, const unsigned mask, const bool only_changed,
                                               TIO* __restrict__ tau_log, uint8_t* __restrict__ flag_log) {
  const bool was_bad = (flag_log && flag_log[il] == 0xff) || (tau_log && isnan((double)tau_log[3 * il]));
  if (was_bad) return;
  const unsigned rb = rflag[i];
  if (only_changed && (rb & mask) == 0u) return;
  if (tau_log) {   // (a poisoned leg's rtau is NaN already)
    tau_log[3 * il] = rtau[3 * i]; tau_log[3 * il + 1] = rtau[3 * i + 1]; tau_log[3 * il + 2] = rtau[3 * i + 2];
  }
  if (flag_log) flag_log[il] = rb == 0xffu ? (uint8_t)0xff : (uint8_t)(flag_log[il] | (rb & mask));
}

// After the legs step of tick `it`, before the advance (tick is still the row's): i = 4 b + leg.  rtau [B,4,3] and rflag [B,4] are what
// mpcqp_stance_drive_kernel left for this tick.  A swing row keeps what the legs step logged; a stance row takes drive_log_step.
// only_changed (MPCQP_DRIVE_IDEAL without a ground row): a stance row the rule left alone keeps the legs step's torque too.  That
// torque and the rule's are both (R J)^T (-f) at the same operands, but the legs step's differs from mpcqp_joint_log's -- which the
// rule's is, bit for bit -- in the last place in fp64 (its inlined copy of leg_joints is fused differently), and in that mode every
// log has to be mpcqp_rollout_legs' bit for bit.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_drive_log_kernel(const int32_t* __restrict__ gait, const int32_t* __restrict__ tick, const TIO* __restrict__ rtau,
                       const uint8_t* __restrict__ rflag, const int only_changed, const int64_t B, const int T, const int it,
                       TIO* __restrict__ tau_log, uint8_t* __restrict__ flag_log) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  if (!stance_mask(nullptr, gait, tick, i, b, l)) return;
  drive_log_step(i, 4 * (b * T + it) + l, rtau, rflag, DRIVE_BITS, only_changed != 0, tau_log, flag_log);
}

}  // namespace
