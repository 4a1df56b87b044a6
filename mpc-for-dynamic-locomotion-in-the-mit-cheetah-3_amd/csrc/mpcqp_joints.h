// mpcqp_joints.h -- closed-form leg inverse kinematics and the joint-space log of a roll-out (the C-ABI is include/mpcqp_joints.h,
// which has the formulas, the branch and the reach rule; its entry points live in mpcqp_kernels.hip).
//
// The leg is a HipX joint followed by a planar 2R chain, so the inverse is three atan2 / acos and two square roots: no iteration, no
// seed.  One device function, leg_joints, does the inverse, and for the log the forward map of mpcqp_elementwise.h at the result
// and tau = (R J)^T (-f); two element-wise kernels call it, one thread per (row, leg), fp64 arithmetic with T-typed I/O, the
// geometry by value.  No LDS, no scratch.  Out-of-reach and non-finite legs are selects on the two clamped quantities and on the
// outputs, never a product with a 0 / 1 flag: every lane runs the same instructions and a NaN stays in its own leg.
// mpcqp_joint_rates adds the joint rates qd = J^-1 R^T (foot velocity relative to the torso point it rides on), by adjugate and
// determinant of the same J, and the joint power tau . qd.
//
// Per leg of mpcqp_joint_log: 18 (actual, shared by the four legs of a row) + 3 + 3 values in, 3 + 3 values and a byte out; about
// 40 flops for the inverse plus four atan2 / acos / sqrt, three sincos and about 250 flops for the forward map and the torque.
#pragma once
#include "mpcqp_elementwise.h"
#include "../../include/mpcqp_joints.h"

namespace {

// The geometry's structure is checked on the host (leg_geometry in mpcqp_kernels.hip): ax = (s_x, 0, 0), ay = (0, s_y, 0),
// hy[l] = (0, d_l, 0), kn = (0, 0, -l1), ft = (0, 0, -l2).
//
// One leg: R world <- torso (row-major), pw = foot - torso origin in world orientation, f the leg's force (world).  Writes q (HipX,
// HipY, Knee: clamped when out of reach, NaN when an input is not finite) and, with TORQUE, tau = (R J(q))^T (-f); returns reach.
// With RATES also qd[0..2] = J(q)^-1 R^T vrel, vrel = foot velocity - v - omega x pw (world), and qd[3] = tau . qd: 0 out of reach or
// where det J = 0, NaN when an input (vrel included) is not finite.
template <bool TORQUE, bool RATES = false>
__device__ __forceinline__ bool leg_joints(const LegGeoDev& geo, const int l, const double (&R)[9], const double (&pw)[3],
                                           const double (&f)[3], double (&q)[3], double (&tau)[3], const double* vrel = nullptr,
                                           double* qd = nullptr) {
  static_assert(TORQUE || !RATES, "the rates share the torque's Jacobian");
  bool fin = true;
#pragma unroll
  for (int a = 0; a < 9; ++a) fin = fin && isfinite(R[a]);
#pragma unroll
  for (int a = 0; a < 3; ++a) fin = fin && isfinite(pw[a]);
  const double sx = geo.ax[0], sy = geo.ay[1], l1 = -geo.kn[2], l2 = -geo.ft[2], d = geo.hy[l][1];
  // p = R^T pw - hip_x
  const double px = (R[0] * pw[0] + R[3] * pw[1] + R[6] * pw[2]) - geo.hx[l][0];
  const double py = (R[1] * pw[0] + R[4] * pw[1] + R[7] * pw[2]) - geo.hx[l][1];
  const double pz = (R[2] * pw[0] + R[5] * pw[1] + R[8] * pw[2]) - geo.hx[l][2];
  const double w = py * py + pz * pz - d * d;
  bool ok = w >= 0.0;
  const double zs = -sqrt(ok ? w : 0.0);
  const double a0 = atan2(d * pz - zs * py, d * py + zs * pz);
  const double r2 = px * px + zs * zs, r = sqrt(r2);
  ok = ok && r >= fabs(l1 - l2) && r <= l1 + l2;
  const double c0 = (r2 - l1 * l1 - l2 * l2) / (2.0 * l1 * l2);
  const double c = c0 > 1.0 ? 1.0 : (c0 < -1.0 ? -1.0 : c0);
  const double k = acos(c), s = sqrt((1.0 - c) * (1.0 + c));
  const double u = l1 + l2 * c, v = sy * (l2 * s);   // the foot seen from the HipY joint, along and across the thigh
  const double a1 = atan2(zs * v - px * u, -(zs * u + px * v));
  const double qc[3] = {sx * a0, sy * a1, k};
  const double nan = __builtin_nan("");
#pragma unroll
  for (int a = 0; a < 3; ++a) q[a] = fin ? qc[a] : nan;
  if constexpr (TORQUE) {
    double pf[3], J[9];
    leg_fk_jac(geo, l, qc, pf, J);
    double g[3];   // R^T (-f)
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = -(R[a] * f[0] + R[3 + a] * f[1] + R[6 + a] * f[2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double t = J[j] * g[0] + J[3 + j] * g[1] + J[6 + j] * g[2];
      tau[j] = fin ? t : nan;
    }
    if constexpr (RATES) {
      double h[3];   // R^T vrel
#pragma unroll
      for (int a = 0; a < 3; ++a) h[a] = R[a] * vrel[0] + R[3 + a] * vrel[1] + R[6 + a] * vrel[2];
      // cofactors of J by row; J^-1 = adj / det, adj = cofactors transposed
      const double c00 = J[4] * J[8] - J[5] * J[7], c01 = J[5] * J[6] - J[3] * J[8], c02 = J[3] * J[7] - J[4] * J[6];
      const double c10 = J[2] * J[7] - J[1] * J[8], c11 = J[0] * J[8] - J[2] * J[6], c12 = J[1] * J[6] - J[0] * J[7];
      const double c20 = J[1] * J[5] - J[2] * J[4], c21 = J[2] * J[3] - J[0] * J[5], c22 = J[0] * J[4] - J[1] * J[3];
      const double det = J[0] * c00 + J[1] * c01 + J[2] * c02;
      const double r[3] = {(c00 * h[0] + c10 * h[1] + c20 * h[2]) / det, (c01 * h[0] + c11 * h[1] + c21 * h[2]) / det,
                           (c02 * h[0] + c12 * h[1] + c22 * h[2]) / det};
      const bool finv = fin && isfinite(vrel[0]) && isfinite(vrel[1]) && isfinite(vrel[2]), move = ok && det != 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) qd[j] = finv ? (move ? r[j] : 0.0) : nan;
      qd[3] = finv ? (move ? (tau[0] * r[0] + tau[1] * r[1]) + tau[2] * r[2] : 0.0) : nan;   // the leg's joint power
    }
  }
  return ok && fin;
}

// mpcqp_leg_ik: i = 4 b + leg.  rot / origin / reach may be null.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_leg_ik_kernel(const TIO* __restrict__ foot, const TIO* __restrict__ rot, const TIO* __restrict__ origin, const LegGeoDev geo,
                    TIO* __restrict__ q, uint8_t* __restrict__ reach, const int64_t B) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, pw[3], ql[3], unused[3];
  const double f0[3] = {0.0, 0.0, 0.0};
  if (rot) {
#pragma unroll
    for (int a = 0; a < 9; ++a) R[a] = (double)rot[9 * b + a];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) pw[a] = (double)foot[3 * i + a] - (origin ? (double)origin[3 * b + a] : 0.0);
  const bool ok = leg_joints<false>(geo, l, R, pw, f0, ql, unused);
#pragma unroll
  for (int a = 0; a < 3; ++a) q[3 * i + a] = (TIO)ql[a];
  if (reach) reach[i] = ok ? 1 : 0;
}

// mpcqp_joint_log: i = 4 (b T + t) + leg over rows [B T] of the roll-out's logs.  Each of q / tau / reach may be null.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_joint_log_kernel(const TIO* __restrict__ actual, const TIO* __restrict__ forces, const TIO* __restrict__ feet, const LegGeoDev geo,
                       TIO* __restrict__ q, TIO* __restrict__ tau, uint8_t* __restrict__ reach, const int64_t rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * rows) return;
  const int64_t row = i / 4;
  const int l = (int)(i % 4);
  const TIO* x = actual + 12 * row;   // rotation vector, CoM, ...
  double qt[4], pw[3], f[3], ql[3], tl[3];
  plant_rotvec_to_quat((double)x[0], (double)x[1], (double)x[2], qt);
  const double qw = qt[0], qx = qt[1], qy = qt[2], qz = qt[3];
  const double R[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                       2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                       2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    pw[a] = (double)feet[3 * i + a] - (double)x[3 + a];
    f[a] = (double)forces[3 * i + a];
  }
  const bool ok = leg_joints<true>(geo, l, R, pw, f, ql, tl);
  if (q) {
#pragma unroll
    for (int a = 0; a < 3; ++a) q[3 * i + a] = (TIO)ql[a];
  }
  if (tau) {
#pragma unroll
    for (int a = 0; a < 3; ++a) tau[3 * i + a] = (TIO)tl[a];
  }
  if (reach) reach[i] = ok ? 1 : 0;
}

// mpcqp_joint_rates: mpcqp_joint_log's rows plus foot_vel [rows,4,3] (null: feet at rest in the world) -> q, qd, tau, power, reach,
// each of which may be null.  The foot rides on the torso point pw: vrel = foot_vel - v - omega x pw.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_joint_rates_kernel(const TIO* __restrict__ actual, const TIO* __restrict__ forces, const TIO* __restrict__ feet,
                         const TIO* __restrict__ foot_vel, const LegGeoDev geo, TIO* __restrict__ q, TIO* __restrict__ qd,
                         TIO* __restrict__ tau, TIO* __restrict__ power, uint8_t* __restrict__ reach, const int64_t rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * rows) return;
  const int64_t row = i / 4;
  const int l = (int)(i % 4);
  const TIO* x = actual + 12 * row;   // rotation vector, CoM, omega, v
  double qt[4], pw[3], f[3], ql[3], tl[3], vr[3], qr[4];
  plant_rotvec_to_quat((double)x[0], (double)x[1], (double)x[2], qt);
  const double qw = qt[0], qx = qt[1], qy = qt[2], qz = qt[3];
  const double R[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                       2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                       2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    pw[a] = (double)feet[3 * i + a] - (double)x[3 + a];
    f[a] = (double)forces[3 * i + a];
  }
  const double om[3] = {(double)x[6], (double)x[7], (double)x[8]};
  double wxr[3];
  cross3(om, pw, wxr);
#pragma unroll
  for (int a = 0; a < 3; ++a) vr[a] = ((foot_vel ? (double)foot_vel[3 * i + a] : 0.0) - (double)x[9 + a]) - wxr[a];
  const bool ok = leg_joints<true, true>(geo, l, R, pw, f, ql, tl, vr, qr);
  if (q) {
#pragma unroll
    for (int a = 0; a < 3; ++a) q[3 * i + a] = (TIO)ql[a];
  }
  if (qd) {
#pragma unroll
    for (int a = 0; a < 3; ++a) qd[3 * i + a] = (TIO)qr[a];
  }
  if (tau) {
#pragma unroll
    for (int a = 0; a < 3; ++a) tau[3 * i + a] = (TIO)tl[a];
  }
  if (power) power[i] = (TIO)qr[3];
  if (reach) reach[i] = ok ? 1 : 0;
}

}  // namespace
