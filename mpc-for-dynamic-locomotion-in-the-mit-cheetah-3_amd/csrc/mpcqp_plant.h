// mpcqp_plant.h -- the rigid-body plant of the device roll-out (the C-ABI is include/mpcqp_sim.h; its entry points live in
// mpcqp_kernels.hip; the roll-out's advance kernel, which takes a plant tick as its world step, in mpcqp_elementwise.h).
//
// Single rigid body, massless legs, forces held over the tick; integrated in a unit quaternion with classical RK4 over `substeps`
// substeps, renormalised after each.  One thread per robot, fp64 arithmetic with T-typed I/O, in the host checker's operation order
// (plant.py) and without contraction into fused multiply-adds, so that the device agrees with the checker to rounding.
//
// Per robot-tick: about 150 flops per derivative, 4 derivatives per substep -> about 6 kflop at 10 substeps, on 52 B (fp32) /
// 104 B (fp64) of state in and out.  The lane is a dependent fp64 chain; the stance sums that do not depend on the state (the net
// foot force and sum foot_l x f_l) are formed once per tick, so the torque inside a derivative is M0 - p x F_feet.
#pragma once
#include "mpcqp_device.h"
#include "../../include/mpcqp_sim.h"

namespace {

constexpr int PLANT_DEFAULT_SUBSTEPS = 10;   // substeps = 0
constexpr int PLANT_MAX_SUBSTEPS = 1000;
constexpr double PLANT_SERIES_ANGLE = 1e-3;  // below this angle the rotation-vector <-> quaternion conversions use their series

struct PlantModel { double m, ixx, iyy, izz; };   // body = NULL: MpcQpConfig.m, diag(1 / Ibody_inv)

// The stance sums and the body of one robot-tick: constant over the tick's substeps.
struct PlantConst {
  double acc[3];   // (sum f_l + F_push) / m + g e_z
  double M0[3];    // sum foot_l x f_l + tau_push
  double Ff[3];    // sum f_l (stance feet only)
  double Ib[6];    // torso-frame inertia xx, yy, zz, xy, xz, yz
  double Ii[6];    // its inverse, same layout
};

// o = S v for a symmetric S stored as xx, yy, zz, xy, xz, yz
__host__ __device__ __forceinline__ void plant_symv(const double (&S)[6], const double (&v)[3], double (&o)[3]) {
#pragma clang fp contract(off)
  o[0] = (S[0] * v[0] + S[3] * v[1]) + S[4] * v[2];
  o[1] = (S[3] * v[0] + S[1] * v[1]) + S[5] * v[2];
  o[2] = (S[4] * v[0] + S[5] * v[1]) + S[2] * v[2];
}

__host__ __device__ __forceinline__ void plant_cross(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
#pragma clang fp contract(off)
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// Inverse of the torso-frame inertia by cofactors; false when a row is invalid (non-finite entry, m <= 0, not positive definite by
// Sylvester's criterion: xx > 0, xx yy - xy^2 > 0, det > 0).
__host__ __device__ __forceinline__ bool plant_inertia(const double m, const double (&I)[6], double (&Ii)[6]) {
#pragma clang fp contract(off)
  const double xx = I[0], yy = I[1], zz = I[2], xy = I[3], xz = I[4], yz = I[5];
  const double c00 = yy * zz - yz * yz, c01 = xz * yz - xy * zz, c02 = xy * yz - xz * yy;
  const double c11 = xx * zz - xz * xz, c12 = xy * xz - xx * yz, c22 = xx * yy - xy * xy;
  const double det = (xx * c00 + xy * c01) + xz * c02;
  bool ok = isfinite(m) && m > 0.0 && xx > 0.0 && c22 > 0.0 && det > 0.0 && isfinite(det);
#pragma unroll
  for (int i = 0; i < 6; ++i) ok = ok && isfinite(I[i]);
  Ii[0] = c00 / det; Ii[1] = c11 / det; Ii[2] = c22 / det; Ii[3] = c01 / det; Ii[4] = c02 / det; Ii[5] = c12 / det;
  return ok;
}

// theta -> (w, x, y, z); w = cos(|theta| / 2) >= 0 for |theta| <= pi
__host__ __device__ __forceinline__ void plant_rotvec_to_quat(const double t0, const double t1, const double t2, double* q) {
#pragma clang fp contract(off)
  const double a = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
  const double a2 = a * a;
  const double s = a <= PLANT_SERIES_ANGLE ? (0.5 - a2 / 48.0) + (a2 * a2) / 3840.0 : sin(0.5 * a) / a;   // sin(a / 2) / a
  q[0] = cos(0.5 * a); q[1] = s * t0; q[2] = s * t1; q[3] = s * t2;
}

// (w, x, y, z) -> theta with |theta| <= pi (the sign of q is chosen with w >= 0)
__host__ __device__ __forceinline__ void plant_quat_to_rotvec(const double* q, double* t) {
#pragma clang fp contract(off)
  const double sg = q[0] < 0.0 ? -1.0 : 1.0;
  const double w = sg * q[0], x = sg * q[1], y = sg * q[2], z = sg * q[3];
  const double nv = sqrt((x * x + y * y) + z * z);
  const double a = 2.0 * atan2(nv, w);
  const double a2 = a * a;
  const double sc = a <= PLANT_SERIES_ANGLE ? (2.0 + a2 / 12.0) + 7.0 * (a2 * a2) / 2880.0 : a / sin(0.5 * a);   // a / sin(a / 2)
  t[0] = sc * x; t[1] = sc * y; t[2] = sc * z;
}

// y = [q (4), p (3), omega (3), v (3)] -> dy/dt
__host__ __device__ __forceinline__ void plant_deriv(const PlantConst& c, const double (&y)[13], double (&d)[13]) {
#pragma clang fp contract(off)
  const double w = y[0], qx = y[1], qy = y[2], qz = y[3];
  const double R[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - w * qz), 2.0 * (qx * qz + w * qy),
                       2.0 * (qx * qy + w * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - w * qx),
                       2.0 * (qx * qz - w * qy), 2.0 * (qy * qz + w * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
  const double p[3] = {y[4], y[5], y[6]}, om[3] = {y[7], y[8], y[9]};
  double pf[3], tau[3], wb[3], tb[3], L[3], gy[3], r[3], e[3];
  plant_cross(p, c.Ff, pf);
#pragma unroll
  for (int i = 0; i < 3; ++i) tau[i] = c.M0[i] - pf[i];                              // sum (foot_l - p) x f_l + tau_push
#pragma unroll
  for (int i = 0; i < 3; ++i) {                                                      // torso frame: R^T omega, R^T tau
    wb[i] = (R[i] * om[0] + R[3 + i] * om[1]) + R[6 + i] * om[2];
    tb[i] = (R[i] * tau[0] + R[3 + i] * tau[1]) + R[6 + i] * tau[2];
  }
  plant_symv(c.Ib, wb, L);
  plant_cross(wb, L, gy);
#pragma unroll
  for (int i = 0; i < 3; ++i) r[i] = tb[i] - gy[i];                                  // I_b wb' = tb - wb x (I_b wb)
  plant_symv(c.Ii, r, e);
  d[0] = 0.5 * (-((om[0] * qx + om[1] * qy) + om[2] * qz));                         // q' = 1/2 (0, omega) (x) q
  d[1] = 0.5 * (w * om[0] + (om[1] * qz - om[2] * qy));
  d[2] = 0.5 * (w * om[1] + (om[2] * qx - om[0] * qz));
  d[3] = 0.5 * (w * om[2] + (om[0] * qy - om[1] * qx));
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    d[4 + i] = y[10 + i];                                                            // p' = v
    d[7 + i] = (R[3 * i] * e[0] + R[3 * i + 1] * e[1]) + R[3 * i + 2] * e[2];        // omega' = R wb'
    d[10 + i] = c.acc[i];                                                            // v' = F / m + g e_z
  }
}

// One tick of the plant.  x [13] state, f [12] foot forces, feet [12] foot positions, stance [4], body (m, Ixx, Iyy, Izz, Ixy, Ixz,
// Iyz), wrench (F, tau), n substeps of h each -> xo [13] (may alias x).
__host__ __device__ inline void plant_tick(const double (&x)[13], const double (&f)[12], const double (&feet)[12], const bool (&stance)[4],
                                           const double (&body)[7], const double (&wrench)[6], const int n, const double h, double (&xo)[13]) {
#pragma clang fp contract(off)
  PlantConst c;
#pragma unroll
  for (int i = 0; i < 6; ++i) c.Ib[i] = body[1 + i];
  const double m = body[0], g = x[12];
  if (!plant_inertia(m, c.Ib, c.Ii)) {
#pragma unroll
    for (int i = 0; i < 12; ++i) xo[i] = NAN;
    xo[12] = g;
    return;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) { c.Ff[a] = 0.0; c.M0[a] = 0.0; }
#pragma unroll
  for (int l = 0; l < 4; ++l) {   // a swing leg's force and foot are ignored (zeroed, whatever they hold)
    const double fl[3] = {stance[l] ? f[3 * l] : 0.0, stance[l] ? f[3 * l + 1] : 0.0, stance[l] ? f[3 * l + 2] : 0.0};
    const double rl[3] = {stance[l] ? feet[3 * l] : 0.0, stance[l] ? feet[3 * l + 1] : 0.0, stance[l] ? feet[3 * l + 2] : 0.0};
    double cr[3];
    plant_cross(rl, fl, cr);
#pragma unroll
    for (int a = 0; a < 3; ++a) { c.Ff[a] = c.Ff[a] + fl[a]; c.M0[a] = c.M0[a] + cr[a]; }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) { c.M0[a] = c.M0[a] + wrench[3 + a]; c.acc[a] = (c.Ff[a] + wrench[a]) / m; }
  c.acc[2] = c.acc[2] + g;
  double y[13], k[13], s[13], t[13];
  plant_rotvec_to_quat(x[0], x[1], x[2], y);
#pragma unroll
  for (int i = 0; i < 9; ++i) y[4 + i] = x[3 + i];
  const double hh = 0.5 * h, h6 = h / 6.0;
  for (int it = 0; it < n; ++it) {   // classical RK4: s = ((k1 + 2 k2) + 2 k3) + k4, y += h / 6 s
    plant_deriv(c, y, k);
#pragma unroll
    for (int i = 0; i < 13; ++i) { s[i] = k[i]; t[i] = y[i] + hh * k[i]; }
    plant_deriv(c, t, k);
#pragma unroll
    for (int i = 0; i < 13; ++i) { s[i] = s[i] + 2.0 * k[i]; t[i] = y[i] + hh * k[i]; }
    plant_deriv(c, t, k);
#pragma unroll
    for (int i = 0; i < 13; ++i) { s[i] = s[i] + 2.0 * k[i]; t[i] = y[i] + h * k[i]; }
    plant_deriv(c, t, k);
#pragma unroll
    for (int i = 0; i < 13; ++i) y[i] = y[i] + h6 * (s[i] + k[i]);
    const double nq = sqrt(((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]) + y[3] * y[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = y[i] / nq;
  }
  plant_quat_to_rotvec(y, xo);
#pragma unroll
  for (int i = 0; i < 9; ++i) xo[3 + i] = y[4 + i];
  xo[12] = g;
}

template <typename TIO>
__device__ __forceinline__ void plant_body_row(const TIO* __restrict__ body, const PlantModel& model, const int64_t b, double (&bd)[7]) {
  if (body) {
#pragma unroll
    for (int i = 0; i < 7; ++i) bd[i] = (double)body[b * 7 + i];
  } else {
    bd[0] = model.m; bd[1] = model.ixx; bd[2] = model.iyy; bd[3] = model.izz; bd[4] = 0.0; bd[5] = 0.0; bd[6] = 0.0;
  }
}

// mpcqp_plant_step: one thread per robot.  x and xo may be the same buffer (each lane reads its row before it writes it).
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_plant_step_kernel(const TIO* x, const TIO* __restrict__ f, const TIO* __restrict__ feet, const uint8_t* __restrict__ contact,
                        const TIO* __restrict__ body, const TIO* __restrict__ wrench, const PlantModel model, const int n, const double h,
                        const int64_t B, TIO* xo) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double xs[13], fs[12], ft[12], bd[7], wr[6], out[13];
  bool st[4];
#pragma unroll
  for (int i = 0; i < 13; ++i) xs[i] = (double)x[b * 13 + i];
#pragma unroll
  for (int i = 0; i < 12; ++i) { fs[i] = (double)f[b * 12 + i]; ft[i] = (double)feet[b * 12 + i]; }
#pragma unroll
  for (int l = 0; l < 4; ++l) st[l] = contact[b * 4 + l] != 0;
  plant_body_row(body, model, b, bd);
#pragma unroll
  for (int i = 0; i < 6; ++i) wr[i] = wrench ? (double)wrench[b * 6 + i] : 0.0;
  plant_tick(xs, fs, ft, st, bd, wr, n, h, out);
#pragma unroll
  for (int i = 0; i < 13; ++i) xo[b * 13 + i] = (TIO)out[i];
}

// The plant as the roll-out's world step (mpcqp_rollout_plant): per-robot body rows and pushes (either may be null), the push
// window [push_ticks[2 b], push_ticks[2 b + 1]) in ticks, n substeps of h each.
template <typename TIO>
struct PlantIn { const TIO* body; const TIO* push; const int32_t* push_ticks; PlantModel model; int n; double h; };

}  // namespace
