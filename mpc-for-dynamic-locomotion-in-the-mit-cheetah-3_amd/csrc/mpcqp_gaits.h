// mpcqp_gaits.h -- per-leg periodic gaits with reactive footholds (the C-ABI is mpcqp_phase_expand / mpcqp_solve_batch_phase in
// include/mpcqp_plan.h and mpcqp_rollout_phase in include/mpcqp_sim.h; the entry points live in mpcqp_kernels.hip, the roll-out's
// advance kernel for this clock in mpcqp_elementwise.h).
//
//   clock     gait[b] = (P, offset[4], stance[4]) in ticks: leg l is in stance at tick t when (t + offset_l) mod P < stance_l, and
//             touches down when that phase is 0 and 0 < stance_l < P.  The row is device memory: clamped, never trusted.
//   foothold  p_xy = c_xy + Rz(psi) stand_xy + (Ts / 2) v_ref_xy + gain (v_xy - v_ref_xy), p_z = stand_z, Ts = stance_l delta: the
//             nominal foot under the hip, half a stance of travel ahead of it, moved by the velocity error.
//   expand    one thread per output element of the operator tuple, like the two expand kernels of mpcqp_elementwise.h, whose element
//             arithmetic (xdes_elem, lever_elem, mpcqp_common.h) it shares.
// fp64 arithmetic with T-typed I/O, in the operation order of the host counterpart (gaits.py), the rule without contraction into
// fused multiply-adds.
#pragma once
#include "mpcqp_common.h"
#include "mpcqp_plant.h"

namespace {

constexpr int GAIT_ROW = 9;                // int32 per robot: P, offset FL FR HL HR, stance FL FR HL HR
constexpr int GAIT_MAX_PERIOD = 65535;

struct GaitLeg { int P, off, st; };   // the clock of one leg

// Leg l of a gait row: P into [1, 65535], the offset reduced into [0, P) (a negative one to its non-negative residue), stance into [0, P].
__device__ __forceinline__ GaitLeg gait_leg(const int32_t* g, const int l) {
  GaitLeg c;
  c.P = min(max(g[0], 1), GAIT_MAX_PERIOD);
  int o = g[1 + l];
  if (o < 0 || o >= c.P) {   // (an offset already in range, the usual row, costs no division)
    o %= c.P;
    if (o < 0) o += c.P;
  }
  c.off = o;
  c.st = min(max(g[5 + l], 0), c.P);
  return c;
}

// Phase of the leg at tick t (a clamped tick plus at most a horizon: t + offset passes 2^31 but stays below 2^32, so the sum is formed
// unsigned; a 64-bit remainder costs several times a 32-bit one).  Stance: phase < st.
__device__ __forceinline__ int gait_phase(const GaitLeg& c, const uint32_t t) { return (int)((t + (uint32_t)c.off) % (uint32_t)c.P); }

// A leg that never lifts (stance = P) or never lands (stance = 0) has no touchdown: it keeps the foot it holds.
__device__ __forceinline__ bool gait_steps(const GaitLeg& c) { return c.st > 0 && c.st < c.P; }

// Per-robot rows of the phase calls: feet [B,4,3] (the roll-out's state, which only its advance kernel writes, through a pointer of its
// own), gait i32 [B,9], stand [B,4,3] (x, y relative to the CoM in the yaw frame; z the world height of the ground under the foot),
// gain [B] or null (0).
template <typename TIO>
struct PhaseRows { const TIO* feet; const int32_t* gait; const TIO* stand; const TIO* gain; };

// Component a < 2 of the foothold rule.  c the CoM component, (cs, sn) of the yaw, s the leg's stand row, v / vr the measured and
// reference velocity component, half_ts = stance delta / 2.
__device__ __forceinline__ double gait_foothold_xy(const int a, const double c, const double cs, const double sn, const double sx,
                                                   const double sy, const double v, const double vr, const double half_ts,
                                                   const double gain) {
#pragma clang fp contract(off)
  const double rot = a == 0 ? cs * sx - sn * sy : sn * sx + cs * sy;
  return ((c + rot) + half_ts * vr) + gain * (v - vr);
}

__device__ __forceinline__ double gait_half_stance(const GaitLeg& c, const double d) {
#pragma clang fp contract(off)
  return 0.5 * ((double)c.st * d);
}

// A non-finite stand or gain row poisons the robot's stage-0 lever arms, which never read the rule: the tuple is then non-finite
// whatever the clock, and the solve reports MPCQP_STATUS_NONFINITE for that robot alone.  Only the 12 stage-0 threads read the rows.
template <typename TIO>
__device__ __forceinline__ bool phase_rows_finite(const PhaseRows<TIO>& ph, const int64_t b) {
  bool ok = ph.gain ? isfinite((double)ph.gain[b]) : true;
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && isfinite((double)ph.stand[b * 12 + i]);
  return ok;
}

// mpcqp_phase_expand.  x_des with gate 1; contact from the clock at tick + k; the foothold of (k, l) from its last touchdown at stage
// j = k - phase: inside the horizon (j >= 1) the rule at the reference pose of stage j with the measured velocity, else the held foot.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_phase_expand_kernel(const TIO* __restrict__ x, const TIO* __restrict__ ref, const PhaseRows<TIO> ph, const int32_t* __restrict__ tick,
                          const double d, const int N, const int64_t B, TIO* __restrict__ r, uint8_t* __restrict__ contact,
                          TIO* __restrict__ xdes) {
  const int nx = (N + 1) * 13, nr = N * 12, per = nx + nr;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * per) return;
  const int64_t b = t / per;
  const int e = (int)(t - b * per);
  const TIO* rf = ref + b * 10;
  const TIO* xb = x + b * 13;
  if (e < nx) {
    xdes[b * nx + e] = (TIO)xdes_elem(rf, xb[12], e / 13, e % 13, d, 1.0);
  } else {
    const int i = e - nx, k = i / 12, l = (i % 12) / 3, a = i % 3;
    const GaitLeg c = gait_leg(ph.gait + b * GAIT_ROW, l);
    const int phi = gait_phase(c, (uint32_t)max(tick[b], 0) + (uint32_t)k);
    const int j = k - phi;
    double foot;
    if (gait_steps(c) && j >= 1) {
      const TIO* s = ph.stand + b * 12 + l * 3;
      if (a == 2) {
        foot = (double)s[2];
      } else {
        double sn, cs;
        sincos(xdes_elem(rf, xb[12], j, 2, d, 1.0), &sn, &cs);
        foot = gait_foothold_xy(a, xdes_elem(rf, xb[12], j, 3 + a, d, 1.0), cs, sn, (double)s[0], (double)s[1], (double)xb[9 + a],
                                (double)rf[6 + a], gait_half_stance(c, d), ph.gain ? (double)ph.gain[b] : 0.0);
      }
    } else {
      foot = (double)ph.feet[b * 12 + l * 3 + a];
    }
    const double lever = lever_elem(foot, rf, xb, k, a, d, 1.0);
    r[b * nr + i] = (k > 0 || phase_rows_finite(ph, b)) ? (TIO)lever : (TIO)NAN;
    if (a == 0) contact[b * (N * 4) + k * 4 + l] = phi < c.st ? 1 : 0;
  }
}

// mpcqp_phase_swing: the swing-foot trajectory of the roll-out on a gait clock, from its logs alone.  One thread per (robot, log row,
// leg), i = 4 (b T + t) + l; a pure function of that row.  A leg in swing (gait_steps and phase >= stance) moves from its lift-off
// foot p0 = feet_log[b,t,l] to the target p1, the foothold rule at the touchdown predicted from the row's measured state (CoM and yaw
// carried rem delta ahead at the measured velocity and the reference yaw rate), along
//   pos = p0 + b(s) (p1 - p0) + z_b(s) e_z,   b(s) = 3 s^2 - 2 s^3,   z_b(s) = 16 H s^2 (1 - s)^2,   s = (phase - stance) / (P - stance)
// with the target held frozen in vel = d pos / dt and acc = d^2 pos / dt^2 (t = s T_sw, T_sw = (P - stance) delta).  With rem = 0 the
// target is, term for term, what mpcqp_phase_advance_kernel writes at the landing.  Every other leg: pos = target = p0, vel = acc = 0.
// Out [row, leg, (pos, vel, acc, target), 3]; every lane runs the same instructions, the cases are selects on the outputs.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_phase_swing_kernel(const TIO* __restrict__ actual, const TIO* __restrict__ desired, const TIO* __restrict__ feet_log,
                         const int32_t* __restrict__ gait, const int32_t* __restrict__ tick0, const TIO* __restrict__ stand,
                         const TIO* __restrict__ gain, const TIO* __restrict__ step_height, const double d, const int T, const int64_t B,
                         TIO* __restrict__ swing, TIO* __restrict__ feet_des) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B * T) return;
  const int l = (int)(i & 3);
  const int64_t row = i >> 2, b = row / T;
  const int t = (int)(row - b * T);
  const TIO* xa = actual + row * 12;
  const TIO* xd = desired + row * 12;
  const PhaseRows<TIO> ph = {feet_log, gait, stand, gain};
  // the tick of the row: tick0 + t as the advance kernel's clock sees it (a negative one is 0; the sum saturates at 2^31 - 1)
  const int64_t tk = min(max((int64_t)tick0[b] + t, (int64_t)0), (int64_t)0x7fffffff);
  const GaitLeg c = gait_leg(gait + b * GAIT_ROW, l);
  const int phi = gait_phase(c, (uint32_t)tk);
  const bool up = gait_steps(c) && phi >= c.st;
  const int n = up ? c.P - c.st : 1;   // (a leg that is down never divides by its own count)
  const double s = (double)(up ? phi - c.st : 0) / (double)n;
  const double ahead = (double)(c.P - phi) * d, tsw = (double)n * d;
  const double hh = (double)step_height[b], g = gain ? (double)gain[b] : 0.0;
  bool fin = phase_rows_finite(ph, b) && isfinite(hh) && isfinite((double)xd[8]) && isfinite((double)xd[9]) && isfinite((double)xd[10]);
#pragma unroll
  for (int a = 0; a < 12; ++a) fin = fin && isfinite((double)xa[a]);
  double p0[3], p1[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { p0[a] = (double)feet_log[3 * i + a]; fin = fin && isfinite(p0[a]); }
  // the yaw exactly as mpcqp_phase_advance_kernel reads it, then carried to the touchdown
  double q[4], sn, cs;
  plant_rotvec_to_quat((double)xa[0], (double)xa[1], (double)xa[2], q);
  const double yaw = atan2(2.0 * (q[1] * q[2] + q[0] * q[3]), 1.0 - 2.0 * (q[2] * q[2] + q[3] * q[3]));
  sincos(yaw + ahead * (double)xd[8], &sn, &cs);
  const TIO* sl = stand + b * 12 + l * 3;
#pragma unroll
  for (int a = 0; a < 2; ++a)
    p1[a] = gait_foothold_xy(a, (double)xa[3 + a] + ahead * (double)xa[9 + a], cs, sn, (double)sl[0], (double)sl[1], (double)xa[9 + a],
                             (double)xd[9 + a], gait_half_stance(c, d), g);
  p1[2] = (double)sl[2];
  const double s2 = s * s, u = s * (1.0 - s);
  const double b0 = s2 * (3.0 - 2.0 * s), b1 = 6.0 * u, b2 = 6.0 - 12.0 * s;
  const double z0 = (16.0 * hh) * (u * u), z1 = (32.0 * hh) * (u * (1.0 - 2.0 * s)), z2 = (32.0 * hh) * ((1.0 - 6.0 * s) + 6.0 * s2);
  const double nan = __builtin_nan("");
  double o[12];
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
#pragma unroll
  for (int e = 0; e < 12; ++e) swing[12 * i + e] = (TIO)o[e];
  if (feet_des) {
#pragma unroll
    for (int a = 0; a < 3; ++a) feet_des[3 * i + a] = (TIO)o[a];
  }
}

}  // namespace
