// mpcqp_legsim.h -- the three-link leg as a plant: forward dynamics and the swing legs of a roll-out under their tracking controller
// (the C-ABI is include/mpcqp_joints.h, which has the rules; the entry points live in mpcqp_kernels.hip): mpcqp_leg_accel (joint
// accelerations of B rows of joint states under applied torques) and mpcqp_swing_track (a leg state per (robot, leg) carried through
// the T rows of a roll-out's log: computed torque plus Cartesian PD, clamped at the actuator's limit, semi-implicit Euler).
//
// Everything the legs need is mpcqp_legdyn.h's: leg_chain, leg_rnea<VEL>, quad_sum and the limits row; the on-trajectory state of a row
// is mpcqp_joints.h's leg_joints<true, true>.  M(q) comes column by column from leg_rnea<false> at unit accelerations, the bias and
// the foot point's acceleration from one leg_rnea<true> at qdd = 0, and both 3x3 systems (J for the desired, M for the actual joint
// acceleration) are solved by cofactors and determinant as the rates solve J.  One thread per (row, leg) / (robot, leg), fp64
// arithmetic with T-typed I/O, geometry and inertia by value with one argument per link (for the reason mpcqp_legdyn.h gives), no LDS.
//
// mpcqp_swing_track is serial over the rows of its robot.  The four legs of a robot are the four lanes of a quad and every lane forms
// the row's quad sums (the plant's right-hand side) before anything diverges; the control periods of a swing row run under a branch
// that holds no lane exchange.  A poisoned leg computes on and is selected away where the row is written: no lane returns early.
#pragma once
#include "mpcqp_actuators.h"
#include "mpcqp_legdyn.h"

namespace {

constexpr double SWING_KP = 250.0, SWING_KD = 15.0;   // gains = NULL (src/main.py:48-49)
constexpr double SWING_H0 = 2e-3;                     // substeps = 0: the default control period (include/mpcqp_joints.h)
constexpr int SWING_MAX_SUBSTEPS = 1000;

// x = A^-1 h by cofactors and determinant (A by rows), in the order the rates solve J; det goes out, the caller selects on it.
__device__ __forceinline__ V3 adj_solve(const M3& A, const V3 h, double& det) {
  const double a0 = A.r0.x, a1 = A.r0.y, a2 = A.r0.z, a3 = A.r1.x, a4 = A.r1.y, a5 = A.r1.z, a6 = A.r2.x, a7 = A.r2.y, a8 = A.r2.z;
  const double c00 = a4 * a8 - a5 * a7, c01 = a5 * a6 - a3 * a8, c02 = a3 * a7 - a4 * a6;
  const double c10 = a2 * a7 - a1 * a8, c11 = a0 * a8 - a2 * a6, c12 = a1 * a6 - a0 * a7;
  const double c20 = a1 * a5 - a2 * a4, c21 = a2 * a3 - a0 * a5, c22 = a0 * a4 - a1 * a3;
  det = a0 * c00 + a1 * c01 + a2 * c02;
  return {(c00 * h.x + c10 * h.y + c20 * h.z) / det, (c01 * h.x + c11 * h.y + c21 * h.z) / det, (c02 * h.x + c12 * h.y + c22 * h.z) / det};
}

// M(q) by rows: column j is the recursion at a unit qdd_j without velocity, torso and gravity terms.
__device__ __forceinline__ M3 leg_mass(const LegLinkInr& i0, const LegLinkInr& i1, const LegLinkInr& i2, const int l, const LegChain& ch) {
  const V3 zero = {0.0, 0.0, 0.0};
  V3 c0, c1, c2, af;
  leg_rnea<false>(i0, i1, i2, l, ch, zero, zero, zero, zero, zero, V3{1.0, 0.0, 0.0}, c0, af);
  leg_rnea<false>(i0, i1, i2, l, ch, zero, zero, zero, zero, zero, V3{0.0, 1.0, 0.0}, c1, af);
  leg_rnea<false>(i0, i1, i2, l, ch, zero, zero, zero, zero, zero, V3{0.0, 0.0, 1.0}, c2, af);
  return {{c0.x, c1.x, c2.x}, {c0.y, c1.y, c2.y}, {c0.z, c1.z, c2.z}};
}

__device__ __forceinline__ bool fin3(const V3 u) { return isfinite(u.x) && isfinite(u.y) && isfinite(u.z); }
__device__ __forceinline__ V3 sel3(const bool c, const V3 a, const V3 b) { return {c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z}; }
__device__ __forceinline__ double norm3(const V3 d) { return sqrt((d.x * d.x + d.y * d.y) + d.z * d.z); }
__device__ __forceinline__ M3 quat_rot(const double (&qt)[4]) {
  const double qw = qt[0], qx = qt[1], qy = qt[2], qz = qt[3];
  return {{1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)},
          {2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)},
          {2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)}};
}
template <typename TIO>
__device__ __forceinline__ V3 load3(const TIO* __restrict__ p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
template <typename TIO>
__device__ __forceinline__ void store3(TIO* __restrict__ p, const bool ok, const V3 v) {
  const double nan = __builtin_nan("");
  p[0] = (TIO)(ok ? v.x : nan); p[1] = (TIO)(ok ? v.y : nan); p[2] = (TIO)(ok ? v.z : nan);
}
// 4: a joint angle outside [q_min, q_max], 8: a joint rate beyond qd_max
__device__ __forceinline__ unsigned swing_limits(const LegLimDev& lim, const V3 q, const V3 qd) {
  unsigned bits = (q.x < lim.qmin[0] || q.x > lim.qmax[0] || q.y < lim.qmin[1] || q.y > lim.qmax[1] || q.z < lim.qmin[2] || q.z > lim.qmax[2]) ? 4u : 0u;
  bits |= (fabs(qd.x) > lim.qdmax[0] || fabs(qd.y) > lim.qdmax[1] || fabs(qd.z) > lim.qdmax[2]) ? 8u : 0u;
  return bits;
}
__device__ __forceinline__ double clamp_sym(const double v, const double m) { return v > m ? m : (v < -m ? -m : v); }   // (a NaN stays)

// mpcqp_leg_accel: i = 4 b + leg.  qd / rot / base and det may be null.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_leg_accel_kernel(const TIO* __restrict__ q, const TIO* __restrict__ qd, const TIO* __restrict__ tau, const TIO* __restrict__ rot,
                       const TIO* __restrict__ base, const LegGeoDev geo, const LegLinkInr i0, const LegLinkInr i1, const LegLinkInr i2,
                       const LegLimDev lim, TIO* __restrict__ qdd, TIO* __restrict__ det, const int64_t B) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  M3 R = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  if (rot) {
    const TIO* r = rot + 9 * b;
    R = {load3(r), load3(r + 3), load3(r + 6)};
  }
  V3 bw = {0.0, 0.0, 0.0}, ba = {0.0, 0.0, 0.0}, bl = {0.0, 0.0, 0.0};   // the torso's omega, alpha and linear acceleration, world axes
  if (base) {
    const TIO* s = base + 9 * b;
    bw = load3(s); ba = load3(s + 3); bl = load3(s + 6);
  }
  const V3 zero = {0.0, 0.0, 0.0};
  const V3 ql = load3(q + 3 * i), tl = load3(tau + 3 * i);
  const V3 v = qd ? load3(qd + 3 * i) : zero;
  const V3 w0 = mtv(R, bw), al0 = mtv(R, ba), a0 = mtv(R, bl), gb = lim.g * R.r2;   // R^T: world -> torso axes
  LegChain ch;
  leg_chain(geo, l, ql, ch);
  V3 bias, af;
  leg_rnea<true>(i0, i1, i2, l, ch, w0, al0, a0, gb, v, zero, bias, af);
  const M3 M = leg_mass(i0, i1, i2, l, ch);
  double dm;
  const V3 x = adj_solve(M, tl - bias, dm);
  const V3 a = sel3(dm != 0.0, x, zero);   // massless legs: no acceleration
  const bool fin = fin3(ql) && fin3(v) && fin3(tl) && fin3(R.r0) && fin3(R.r1) && fin3(R.r2) && fin3(bw) && fin3(ba) && fin3(bl) && fin3(a);
  store3(qdd + 3 * i, fin, a);
  if (det) det[i] = (TIO)dm;
}

// The operands of mpcqp_swing_track_kernel that are read per row, and its outputs (each may be null).
template <typename TIO>
struct SwingIn { const TIO *actual, *forces, *feet_log; const uint8_t* contact; const TIO *swing, *base_acc, *body, *gains; };
template <typename TIO>
struct SwingOut { TIO *q, *qd, *tau, *foot, *err; uint8_t* flag; };

// mpcqp_swing_track: i = 4 b + leg, serial over the T rows of robot b.  n control periods of h each per swing row.
// The kernel's text is mpcqp_legsim_rows.inl, included once in this kernel and once in its ACT twin below: a device function shared by
// the two changes this kernel's assembly (tried with by-reference and by-value rows), a second copy of the text would drift.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_swing_track_kernel(const SwingIn<TIO> in, TIO* __restrict__ state, const PlantModel model, const LegGeoDev geo, const LegLinkInr i0,
                         const LegLinkInr i1, const LegLinkInr i2, const LegLimDev lim, const SwingOut<TIO> out, const int64_t B, const int T,
                         const int n, const double h) {
  constexpr bool ACT = false;
  const double* const act = nullptr;
#include "mpcqp_legsim_rows.inl"
}

// ... with an actuator table set (include/mpcqp_actuators.h): act [B,9], lim.taumax is not read.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_swing_track_act_kernel(const SwingIn<TIO> in, TIO* __restrict__ state, const PlantModel model, const LegGeoDev geo, const LegLinkInr i0,
                             const LegLinkInr i1, const LegLinkInr i2, const LegLimDev lim, const SwingOut<TIO> out, const int64_t B,
                             const int T, const int n, const double h, const double* __restrict__ act) {
  constexpr bool ACT = true;
#include "mpcqp_legsim_rows.inl"
}

}  // namespace
