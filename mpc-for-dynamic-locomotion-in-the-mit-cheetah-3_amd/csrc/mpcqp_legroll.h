// mpcqp_legroll.h -- the swing legs inside the roll-out on a gait clock (the C-ABI is mpcqp_rollout_legs in include/mpcqp_sim.h, which
// has the rules; the entry point lives in mpcqp_kernels.hip).  Two kernels around the unchanged mpcqp_phase_advance_kernel:
//   mpcqp_legs_step_kernel   before the advance: the row mpcqp_phase_swing and mpcqp_swing_track would read at this tick, formed from
//                            the live buffers (x, ref, feet, tick, the solve's stage-0 forces), and one row of mpcqp_swing_track on it,
//                            the leg state carried in `legs` (fp64 whatever the I/O type)
//   mpcqp_legs_land_kernel   after the advance: the landing miss of every leg that touches down at the new tick and, with
//                            MPCQP_LAND_ACTUAL, the foot the leg delivered in place of the rule's xy
// The landing is a launch of its own: the advance stands at 186-192 VGPRs without scratch and four forward kinematics do not fit in
// what is left, and as a second launch the advance keeps its source and its assembly.
//
// The row body is a SECOND COPY of mpcqp_phase_swing_kernel's rule (mpcqp_gaits.h) and of mpcqp_swing_track_kernel's row
// (mpcqp_legsim.h), not a shared function: those two kernels keep their source and with it their assembly.  What differs from the copy's
// origin is where the operands come from, the fp64 state, and the torso's acceleration, which here includes the robot's push where its
// window is open.  A change to either rule has to be made in both places; tests/test_gpu_rollout_legs.py holds the two together (the
// logs of this kernel against mpcqp_phase_swing and mpcqp_swing_track on the roll-out's logs).
//
// Layout as mpcqp_legdyn.h states it: one thread per (robot, leg), a robot's four legs in one quad, fp64 arithmetic, no LDS, geometry
// and inertia by value with one argument per link.  Every lane exchange (quad_sum) comes before anything diverges; the control periods
// of a swing row run under a branch that holds none.  A poisoned leg computes on and is selected away where the row is written.
#pragma once
#include "mpcqp_gaits.h"
#include "mpcqp_joints.h"
#include "mpcqp_legsim.h"

namespace {

constexpr int LAND_RULE = 0, LAND_ACTUAL = 1;   // MPCQP_LAND_RULE, MPCQP_LAND_ACTUAL (include/mpcqp_sim.h)

// The logs of the legs step, each may be null: swing [B,T,4,4,3], q / qd / tau / foot [B,T,4,3], err [B,T,4], flag u8 [B,T,4].
template <typename TIO>
struct LegRollOut { TIO *swing, *q, *qd, *tau, *foot, *err; uint8_t* flag; };

// mpcqp_phase_swing_kernel's rule for one (robot, leg) at the live tick: xa = x[0..11], the reference row rf (desired[8] = rf[9],
// desired[9..11] = rf[6..8]), the held foot p0, the leg's clock c at phase phi -> o = (pos, vel, acc, target), NaN where an operand is
// not finite.  Without contraction, as there.
template <typename TIO>
__device__ __forceinline__ void legroll_swing_row(const TIO* __restrict__ xa, const TIO* __restrict__ rf, const TIO* __restrict__ p0t,
                                                  const TIO* __restrict__ sl, const GaitLeg& c, const int phi, bool fin, const double hh,
                                                  const double g, const double d, double (&o)[12]) {
#pragma clang fp contract(off)
  const bool up = gait_steps(c) && phi >= c.st;
  const int n = up ? c.P - c.st : 1;   // (a leg that is down never divides by its own count)
  const double s = (double)(up ? phi - c.st : 0) / (double)n;
  const double ahead = (double)(c.P - phi) * d, tsw = (double)n * d;
  fin = fin && isfinite(hh) && isfinite((double)rf[9]) && isfinite((double)rf[6]) && isfinite((double)rf[7]);
#pragma unroll
  for (int a = 0; a < 12; ++a) fin = fin && isfinite((double)xa[a]);
  double p0[3], p1[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { p0[a] = (double)p0t[a]; fin = fin && isfinite(p0[a]); }
  double q[4], sn, cs;
  plant_rotvec_to_quat((double)xa[0], (double)xa[1], (double)xa[2], q);
  const double yaw = atan2(2.0 * (q[1] * q[2] + q[0] * q[3]), 1.0 - 2.0 * (q[2] * q[2] + q[3] * q[3]));
  sincos(yaw + ahead * (double)rf[9], &sn, &cs);
#pragma unroll
  for (int a = 0; a < 2; ++a)
    p1[a] = gait_foothold_xy(a, (double)xa[3 + a] + ahead * (double)xa[9 + a], cs, sn, (double)sl[0], (double)sl[1], (double)xa[9 + a],
                             (double)rf[6 + a], gait_half_stance(c, d), g);
  p1[2] = (double)sl[2];
  const double s2 = s * s, u = s * (1.0 - s);
  const double b0 = s2 * (3.0 - 2.0 * s), b1 = 6.0 * u, b2 = 6.0 - 12.0 * s;
  const double z0 = (16.0 * hh) * (u * u), z1 = (32.0 * hh) * (u * (1.0 - 2.0 * s)), z2 = (32.0 * hh) * ((1.0 - 6.0 * s) + 6.0 * s2);
  const double nan = __builtin_nan("");
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double dp = p1[a] - p0[a];
    const double pos = a == 2 ? (p0[a] + b0 * dp) + z0 : p0[a] + b0 * dp;
    const double vel = (a == 2 ? b1 * dp + z1 : b1 * dp) / tsw;
    const double acc = (a == 2 ? b2 * dp + z2 : b2 * dp) / (tsw * tsw);
    o[a] = !fin ? nan : (up ? pos : p0[a]);
    o[3 + a] = !fin ? nan : (up ? vel : 0.0);
    o[6 + a] = !fin ? nan : (up ? acc : 0.0);
    o[9 + a] = !fin ? nan : (up ? p1[a] : p0[a]);
  }
}

// The legs step of tick `it`: i = 4 b + leg.  u is the solve's force buffer [B,N,12]; n control periods of h each on a swing row.
// The kernel's text is mpcqp_legroll_row.inl, included once in this kernel and once in its ACT twin below: a device function shared by
// the two changes this kernel's assembly (tried with by-reference and by-value rows), a second copy of the text would drift.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_legs_step_kernel(const TIO* __restrict__ x, const TIO* __restrict__ ref, const PhaseRows<TIO> ph, const int32_t* __restrict__ tick,
                       const TIO* __restrict__ u, const TIO* __restrict__ step_height, const TIO* __restrict__ gains,
                       double* __restrict__ legs, const PlantIn<TIO> pin, const LegGeoDev geo, const LegLinkInr i0, const LegLinkInr i1,
                       const LegLinkInr i2, const LegLimDev lim, const LegRollOut<TIO> out, const double d, const int N, const int64_t B,
                       const int T, const int it, const int n, const double h) {
  constexpr bool ACT = false;
  const double* const act = nullptr;
#include "mpcqp_legroll_row.inl"
}

// ... with an actuator table set (include/mpcqp_actuators.h): act [B,9], lim.taumax is not read.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_legs_step_act_kernel(const TIO* __restrict__ x, const TIO* __restrict__ ref, const PhaseRows<TIO> ph, const int32_t* __restrict__ tick,
                           const TIO* __restrict__ u, const TIO* __restrict__ step_height, const TIO* __restrict__ gains,
                           double* __restrict__ legs, const PlantIn<TIO> pin, const LegGeoDev geo, const LegLinkInr i0, const LegLinkInr i1,
                           const LegLinkInr i2, const LegLimDev lim, const LegRollOut<TIO> out, const double d, const int N, const int64_t B,
                           const int T, const int it, const int n, const double h, const double* __restrict__ act) {
  constexpr bool ACT = true;
#include "mpcqp_legroll_row.inl"
}

// After the advance of tick `it`: i = 4 b + leg.  x and tick are the post-step values, feet[b][l] of a leg that touches down at the new
// tick is the rule's foothold, which the advance has just written.  The miss is |c + R p_foot(q) - rule foothold| with q from `legs`;
// with LAND_ACTUAL the foot's xy becomes the leg's, z stays the rule's stand_z.  A non-finite q gives a NaN miss and a NaN foot.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_legs_land_kernel(const TIO* __restrict__ x, TIO* __restrict__ feet, const int32_t* __restrict__ gait, const int32_t* __restrict__ tick,
                       const double* __restrict__ legs, const LegGeoDev geo, const int land, const int64_t B, const int T, const int it,
                       TIO* __restrict__ miss_log) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  // the clock the advance landed on: tick + 1 of a tick >= 0 (2^31 after the last one), 0 otherwise
  const int32_t tn = tick[b];
  const uint32_t tc = (tn > 0 || tn == INT32_MIN) ? (uint32_t)tn : 0u;
  const GaitLeg gc = gait_leg(gait + b * GAIT_ROW, l);
  const bool td = gait_steps(gc) && gait_phase(gc, tc) == 0;
  double miss = 0.0;
  if (td) {
    const TIO* xb = x + 13 * b;
    double qt[4];
    plant_rotvec_to_quat((double)xb[0], (double)xb[1], (double)xb[2], qt);
    const M3 Rw = quat_rot(qt);
    const V3 q = {legs[7 * i], legs[7 * i + 1], legs[7 * i + 2]};
    LegChain ch;
    leg_chain(geo, l, q, ch);
    const V3 p = load3(xb + 3) + mv(Rw, ch.p3);
    TIO* ft = feet + 3 * i;
    miss = norm3(p - load3(ft));
    if (land == LAND_ACTUAL) { ft[0] = (TIO)p.x; ft[1] = (TIO)p.y; }
  }
  if (miss_log) miss_log[4 * ((int64_t)b * T + it) + l] = (TIO)miss;
}

}  // namespace
