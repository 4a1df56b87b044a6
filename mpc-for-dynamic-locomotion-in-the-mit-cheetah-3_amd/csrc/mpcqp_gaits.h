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

}  // namespace
