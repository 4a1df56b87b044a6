// mpcqp_plan.h -- footstep plans and swing-foot trajectories on the device (the C-ABI is include/mpcqp_plan.h; its entry points
// live in mpcqp_kernels.hip), and the plan clock that every reader of a plan table decodes its meta row with (the swing kernel here,
// the expand / advance kernels of mpcqp_elementwise.h).  The kernels here are fp64 arithmetic with T-typed I/O, in the host ports'
// operation order and without contraction into fused multiply-adds (footstep_planner.py, foot_trajectory_generator.py).
//
//   planner   two launches.  (1) one lane per robot runs the sequential unicycle recurrence (theta += w dt, centre += R(theta) v dt,
//             ss + ds ticks per step) and leaves theta, centre x / y, cos / sin theta of every step in an engine-owned [B,S,5] fp64
//             workspace.  (2) one thread per (robot, step) row builds pos / feet_id / ang / hip: a foot that stays down at step s
//             keeps row s - 1, which is its fresh placement of step s - 1 because the keep pattern alternates, so no thread depends
//             on another.  Rows are staged in LDS and written back as contiguous runs (coalesced stores).
//   swing     one thread per (robot, tick, leg) output group, closed form (no search, no transcendental), staged the same way.
#pragma once
#include "mpcqp_device.h"
#include "../../include/mpcqp_plan.h"

namespace {

constexpr int PLAN_WS = 5;                  // workspace doubles per (robot, step): theta, centre x, centre y, cos theta, sin theta
constexpr int PLAN_STANDING_STEPS = 100;    // total_steps == 0: 100 identical all-stance steps (src/footstep_planner.py:53-71)
constexpr int PLAN_MAX_TICKS = 65535;       // ss / ds clamp: the recurrence runs (ss + ds) ticks per step in one lane
constexpr int PLAN_BLOCK = 256;             // rows (planner) / output groups (swing) per workgroup

struct PlanGait { int rows, ss, ds; bool standing; };

// The gait row [total_steps, ss, ds, first_swing mask] is device memory the host cannot inspect: clamped, never trusted.
__device__ __forceinline__ PlanGait plan_gait(const int32_t* g, const int S) {
  PlanGait p;
  p.standing = g[0] <= 0;
  p.rows = min(p.standing ? PLAN_STANDING_STEPS : g[0], S);
  p.ss = min(max(g[1], 0), PLAN_MAX_TICKS);
  p.ds = min(max(g[2], 0), PLAN_MAX_TICKS);
  return p;
}

// The plan clock: where tick tau falls in a plan whose meta row is [S, ss, ds, reserved].  The plan table lives in device memory the
// host cannot inspect: malformed rows are clamped, never indexed with -- 1 <= S_b <= Smax, ss >= 0, ss + ds >= 1; callers clamp
// tick >= 0 (include/mpcqp.h).  Past the plan: the last step with its time running on.  I is the caller's tick arithmetic: int
// where tau stays within the horizon of a tick, int64_t in the swing kernel, whose tau = tick + K - 1 may pass 2^31.
template <typename I>
struct PlanClock {
  int S;         // steps of the robot's plan
  I ss, period;  // single-support ticks of a step, and all its ticks
  int step;      // the step tau falls in
  I tin;         // ... and the ticks into it
  bool swing;    // ... which are single support: the step's own stance pattern holds (else every foot is down)
  double gate;   // 0 on the last plan step, where the references are zeroed (src/mpc.py:181-183), else 1
};

template <typename I>
__device__ __forceinline__ PlanClock<I> plan_clock(const int S, const int ss, const int ds, const int Smax, const I tau) {
  PlanClock<I> c;
  c.S = min(max(S, 1), Smax);
  c.ss = max(ss, 0);
  c.period = max(c.ss + max(ds, 0), (I)1);
  c.step = (int)min(tau / c.period, (I)(c.S - 1));
  c.tin = tau - c.step * c.period;
  c.swing = c.tin < c.ss;
  c.gate = c.step == c.S - 1 ? 0.0 : 1.0;
  return c;
}
template <typename I>
__device__ __forceinline__ PlanClock<I> plan_clock(const int32_t* meta, const int Smax, const I tau) {
  return plan_clock(meta[0], meta[1], meta[2], Smax, tau);
}

template <typename TIO>
__global__ void __launch_bounds__(64)
mpcqp_plan_unicycle_kernel(const TIO* __restrict__ feet0, const TIO* __restrict__ cmd, const int32_t* __restrict__ gait, const double dt,
                           const int S, const int64_t B, double* __restrict__ ws) {
#pragma clang fp contract(off)
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const PlanGait p = plan_gait(gait + b * 4, S);
  if (p.standing) return;                                  // the standing plan is read from the inputs alone
  const TIO* f = feet0 + b * 12;
  const TIO* c = cmd + b * 5;
  const double vx = (double)c[1], vy = (double)c[2], w = (double)c[3];
  double theta = (double)c[0];
  // the unicycle starts under the feet centroid (feet0.mean(axis=0): ((f0 + f1) + f2) + f3, then / 4)
  double cx = ((((double)f[0] + (double)f[3]) + (double)f[6]) + (double)f[9]) / 4.0;
  double cy = ((((double)f[1] + (double)f[4]) + (double)f[7]) + (double)f[10]) / 4.0;
  double sn, cs;
  sincos(theta, &sn, &cs);
  double* o = ws + b * S * PLAN_WS;
  const int ticks = p.ss + p.ds;
  for (int j = 0; j < p.rows; ++j) {
    if (j >= 1) {                                          // the unicycle only moves from the second step on
      // The lane is alone on its SIMD at B = 65536 and each sincos is a long dependent chain: four ticks at a time give it four
      // independent ones.  Same operations in the same order (theta chain, then the centre sums tick by tick).
      int k = 0;
      for (; k + 4 <= ticks; k += 4) {
        double th[4], s4[4], c4[4];
        th[0] = theta + w * dt;
        for (int q = 1; q < 4; ++q) th[q] = th[q - 1] + w * dt;
        for (int q = 0; q < 4; ++q) sincos(th[q], &s4[q], &c4[q]);
        for (int q = 0; q < 4; ++q) {
          cx += (c4[q] * vx + (-s4[q]) * vy) * dt;
          cy += (s4[q] * vx + c4[q] * vy) * dt;
        }
        theta = th[3]; sn = s4[3]; cs = c4[3];
      }
      for (; k < ticks; ++k) {
        theta += w * dt;
        sincos(theta, &sn, &cs);
        cx += (cs * vx + (-sn) * vy) * dt;                 // centre[:2] += R @ v[:2] * dt
        cy += (sn * vx + cs * vy) * dt;
      }
    }
    o[j * PLAN_WS + 0] = theta; o[j * PLAN_WS + 1] = cx; o[j * PLAN_WS + 2] = cy;
    o[j * PLAN_WS + 3] = cs;    o[j * PLAN_WS + 4] = sn;
  }
}

// Fresh placement of leg l at the step whose workspace row is w: centre +- torso / 2 +- half_width, z at the centroid height.
template <typename TIO>
__device__ __forceinline__ void plan_fresh(const double* w, const TIO* f, const int l, double* out) {
#pragma clang fp contract(off)
  const double cs = w[3], sn = w[4];
  const double dx = (double)f[0] - (double)f[6], dy = (double)f[1] - (double)f[7];      // FL - HL
  const double hx = (double)f[9] - (double)f[6], hy = (double)f[10] - (double)f[7];     // HR - HL
  const double tx = cs * dx + (-sn) * dy, ty = sn * dx + cs * dy;
  const double wx = (cs * hx + (-sn) * hy) / 2.0, wy = (sn * hx + cs * hy) / 2.0;
  const double s0 = l < 2 ? 1.0 : -1.0, s1 = (l & 1) ? 1.0 : -1.0;                      // FL (+,-) FR (+,+) HL (-,-) HR (-,+)
  out[0] = (w[1] + s0 * tx / 2.0) + s1 * wx;
  out[1] = (w[2] + s0 * ty / 2.0) + s1 * wy;
  out[2] = ((((double)f[2] + (double)f[5]) + (double)f[8]) + (double)f[11]) / 4.0;
}

template <typename TIO>
__global__ void __launch_bounds__(PLAN_BLOCK)
mpcqp_plan_tables_kernel(const TIO* __restrict__ feet0, const TIO* __restrict__ cmd, const int32_t* __restrict__ gait,
                         const double* __restrict__ ws, const int S, const int64_t B, TIO* __restrict__ pos, uint8_t* __restrict__ fid,
                         int32_t* __restrict__ meta, TIO* __restrict__ ang, TIO* __restrict__ hip) {
#pragma clang fp contract(off)
  __shared__ TIO t_pos[PLAN_BLOCK * 12];
  __shared__ TIO t_hip[PLAN_BLOCK * 3];
  __shared__ uint8_t t_fid[PLAN_BLOCK * 4];
  const int64_t R = B * S, r0 = (int64_t)blockIdx.x * PLAN_BLOCK, r = r0 + threadIdx.x;
  const int n = (int)min((int64_t)PLAN_BLOCK, R - r0);
  if (r < R) {
    const int64_t b = r / S;
    const int s = (int)(r - b * S);
    const int32_t* g = gait + b * 4;
    const PlanGait p = plan_gait(g, S);
    const TIO* f = feet0 + b * 12;
    const double h = (double)cmd[b * 5 + 4];
    const int se = min(s, p.rows - 1);                     // rows past the plan repeat its last row
    double th, hx, hy;
    int stance;                                            // bit l: leg l in stance at this step
    if (p.standing) {
      for (int e = 0; e < 12; ++e) t_pos[threadIdx.x * 12 + e] = f[e];
      th = (double)cmd[b * 5 + 0];
      hx = hy = __builtin_nan("");
      stance = 15;
    } else {
      const double* w = ws + (b * S + se) * PLAN_WS;
      const int fs = g[3] & 15;
      const int keep = se == 0 ? 0 : (((se - 1) & 1) ? (~fs & 15) : fs);   // first_swing, then its complement, alternating
      for (int l = 0; l < 4; ++l) {
        double q[3];
        plan_fresh(((keep >> l) & 1) ? w - PLAN_WS : w, f, l, q);           // a kept foot stays on its fresh row of step se - 1
        for (int a = 0; a < 3; ++a) t_pos[threadIdx.x * 12 + l * 3 + a] = (TIO)q[a];
      }
      th = w[0];
      const double dx = (double)f[0] - (double)f[6], dy = (double)f[1] - (double)f[7];
      hx = w[1] - (w[3] * dx + (-w[4]) * dy) / 2.0;       // centre - torso / 2
      hy = w[2] - (w[4] * dx + w[3] * dy) / 2.0;
      stance = se == 0 ? 15 : keep;
    }
    for (int l = 0; l < 4; ++l) t_fid[threadIdx.x * 4 + l] = (uint8_t)((stance >> l) & 1);
    t_hip[threadIdx.x * 3 + 0] = (TIO)hx; t_hip[threadIdx.x * 3 + 1] = (TIO)hy; t_hip[threadIdx.x * 3 + 2] = (TIO)h;
    if (ang) ang[r] = (TIO)th;
    if (s == 0) { meta[b * 4 + 0] = p.rows; meta[b * 4 + 1] = p.ss; meta[b * 4 + 2] = p.ds; meta[b * 4 + 3] = 0; }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < n * 12; q += PLAN_BLOCK) pos[r0 * 12 + q] = t_pos[q];
  for (int q = threadIdx.x; q < n * 4; q += PLAN_BLOCK) fid[r0 * 4 + q] = t_fid[q];
  if (hip)
    for (int q = threadIdx.x; q < n * 3; q += PLAN_BLOCK) hip[r0 * 3 + q] = t_hip[q];
}

// One output group = (robot b, tick tick[b] + j, leg l): the pos / vel / acc 6-vectors of the trajectory and the logged desired
// foot position.  Step index and time in step are closed form (plan_clock).
template <typename TIO>
__global__ void __launch_bounds__(PLAN_BLOCK)
mpcqp_swing_kernel(const TIO* __restrict__ pos, const uint8_t* __restrict__ fid, const int32_t* __restrict__ meta, const TIO* __restrict__ ang,
                   const int32_t* __restrict__ tick, const TIO* __restrict__ step_height, const double dt, const int K, const int Smax,
                   const int64_t B, TIO* __restrict__ traj, TIO* __restrict__ des) {
#pragma clang fp contract(off)
  __shared__ TIO t_traj[PLAN_BLOCK * 18];
  __shared__ TIO t_des[PLAN_BLOCK * 3];
  const int64_t G = B * K * 4, g0 = (int64_t)blockIdx.x * PLAN_BLOCK, gi = g0 + threadIdx.x;
  const int n = (int)min((int64_t)PLAN_BLOCK, G - g0);
  if (gi < G) {
    const int l = (int)(gi & 3);
    const int64_t bj = gi >> 2, b = bj / K;
    const int j = (int)(bj - b * K);
    const PlanClock<int64_t> c = plan_clock(meta + b * 4, Smax, (int64_t)max(tick[b], 0) + j);
    const int s = c.step, nx = min(s + 1, c.S - 1);        // past the plan: target = start
    const int64_t ss = c.ss, t = c.tin;
    const TIO* p0 = pos + ((b * Smax + s) * 4 + l) * 3;
    const TIO* p1 = pos + ((b * Smax + nx) * 4 + l) * 3;
    const double a0 = (double)ang[b * Smax + s], a1 = (double)ang[b * Smax + nx];
    double o[18];                                          // pos | vel | acc, each (angle xyz, position xyz)
    for (int e = 0; e < 18; ++e) o[e] = 0.0;
    const double tsw = 0.80 * (double)ss;                  // land before the end of single support
    if (s == 0) {                                          // standing phase
      o[2] = a0;
      for (int a = 0; a < 3; ++a) o[3 + a] = (double)p0[a];
    } else if ((double)t >= tsw) {                         // landed (t >= tsw, which includes double support t >= ss)
      o[2] = a1;
      for (int a = 0; a < 3; ++a) o[3 + a] = (double)p1[a];
    } else {
      const double tt = (double)t, t2 = tt * tt, t3 = t2 * tt, t4 = t3 * tt;
      const double w2 = tsw * tsw, w3 = w2 * tsw, w4 = w3 * tsw, dt2 = dt * dt;
      const double c3 = -2.0 / w3, c2 = 3.0 / w2;         // cubic 3 (t/Ts)^2 - 2 (t/Ts)^3 in the plane and for the angle
      const double s0 = c3 * t3 + c2 * t2;
      const double s1 = (3.0 * c3 * t2 + 2.0 * c2 * tt) / dt;
      const double s2 = (6.0 * c3 * tt + 2.0 * c2) / dt2;
      for (int a = 0; a < 2; ++a) {
        const double st = (double)p0[a], dp = (double)p1[a] - st;
        o[3 + a] = st + dp * s0; o[9 + a] = dp * s1; o[15 + a] = dp * s2;
      }
      const double da = a1 - a0;
      o[2] = a0 + da * s0; o[8] = da * s1; o[14] = da * s2;
      const double hh = (double)step_height[b];            // quartic bump of height step_height, zero at both ends
      const double q4 = 16.0 * hh / w4, q3 = -32.0 * hh / w3, q2 = 16.0 * hh / w2;
      o[5] = q4 * t4 + q3 * t3 + q2 * t2 + (double)p0[2];
      o[11] = (4.0 * q4 * t3 + 3.0 * q3 * t2 + 2.0 * q2 * tt) / dt;
      o[17] = (12.0 * q4 * t2 + 6.0 * q3 * tt + 2.0 * q2) / dt2;
    }
    for (int e = 0; e < 18; ++e) t_traj[threadIdx.x * 18 + e] = (TIO)o[e];
    // the host generator's side effect (src/foot_trajectory_generator.py:53-54) as a pure rule, include/mpcqp_plan.h: a swing leg
    // follows the trajectory (whose position is the target from 0.8 ss on, so also on the first double-support tick t == ss) until
    // the step has been marked all-stance, i.e. after its first double-support tick; step 0 never reaches the side effect
    const bool planted = fid[(b * Smax + s) * 4 + l] != 0 || (s > 0 && t > ss);
    double d[3];
    for (int a = 0; a < 3; ++a) d[a] = planted ? (double)p0[a] : o[3 + a];
    if (!planted && d[2] < 0.0) d[2] = 0.0;
    for (int a = 0; a < 3; ++a) t_des[threadIdx.x * 3 + a] = (TIO)d[a];
  }
  __syncthreads();
  for (int q = threadIdx.x; q < n * 18; q += PLAN_BLOCK) traj[g0 * 18 + q] = t_traj[q];
  if (des)
    for (int q = threadIdx.x; q < n * 3; q += PLAN_BLOCK) des[g0 * 3 + q] = t_des[q];
}

}  // namespace
