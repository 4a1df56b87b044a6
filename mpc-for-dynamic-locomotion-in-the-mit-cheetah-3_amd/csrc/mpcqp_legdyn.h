// mpcqp_legdyn.h -- rigid-body dynamics of the three-link leg on a moving torso (the C-ABI is include/mpcqp_joints.h, which has the
// formulas; the entry points live in mpcqp_kernels.hip): mpcqp_leg_dynamics (joint torques, joint-space inertia and bias of B rows of
// joint states) and mpcqp_leg_effort (joint accelerations, full joint torques, power and actuator-limit flags of a roll-out's log).
//
// Recursive Newton-Euler over HipX, HipY, Knee, written in the torso's axes: the forward pass carries each link's angular velocity,
// angular acceleration and the acceleration of its joint origin outwards, the backward pass the link forces and moments inwards;
// tau_j is the moment about joint j's origin along its axis.  The FOOT link is part of the SHANK row (the default row folds it in on
// the host).  Two element-wise kernels, one thread per (row, leg), fp64 arithmetic with T-typed I/O, geometry and inertia by value
// (the leg-indexed rows are read from the kernel arguments per lane), no LDS.  Non-finite and out-of-reach legs are selects on the
// results, never a product with a 0 / 1 flag.
//
// Vectors and matrices are small structs with named components (V3, M3), the three links are written out, and the inertial row
// reaches the kernels as one argument per link.  The last is on purpose.  mpcqp_leg_effort_kernel inlines the same leg_joints<true,
// true> as mpcqp_joint_rates_kernel, and its q, qd and (R J)^T (-f) have to be that kernel's bit for bit.  The compiler fuses the
// multiply-adds of leg_joints the same way in both only if the small arrays of that code are promoted to registers in the same,
// first round; that round gives up on the whole kernel at the first by-value struct larger than its budget (512 B here), and the row
// in one piece is 1064 B.  tests/test_gpu_leg_dynamics.py (massless legs) holds the two kernels to each other.
#pragma once
#include "mpcqp_actuators.h"
#include "mpcqp_joints.h"

namespace {

// MpcQpLegInertia as the kernels take it (checked on the host, leg_inertia_row in mpcqp_kernels.hip).
// One kernel argument per link and one for the limits (see above).
struct LegLinkInr { double m[4], c[4][3], I[4][6]; };   // one link (HIP, THIGH or SHANK) of the four legs
struct LegLimDev { double qmin[3], qmax[3], qdmax[3], taumax[3], g; };
struct LegInrDev { LegLinkInr k0, k1, k2; LegLimDev lim; };   // host side only: what leg_inertia_row fills

struct V3 { double x, y, z; };
struct M3 { V3 r0, r1, r2; };      // rows
struct S3 { double xx, yy, zz, xy, xz, yz; };

__device__ __forceinline__ V3 operator+(const V3 a, const V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(const V3 a, const V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(const double s, const V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(const V3 a, const V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(const V3 a, const V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 mv(const M3& A, const V3 v) { return {dot(A.r0, v), dot(A.r1, v), dot(A.r2, v)}; }
__device__ __forceinline__ V3 mtv(const M3& A, const V3 v) {   // A^T v
  return {(A.r0.x * v.x + A.r1.x * v.y) + A.r2.x * v.z, (A.r0.y * v.x + A.r1.y * v.y) + A.r2.y * v.z, (A.r0.z * v.x + A.r1.z * v.y) + A.r2.z * v.z};
}
__device__ __forceinline__ V3 mrow(const V3 a, const M3& B) { return (a.x * B.r0 + a.y * B.r1) + a.z * B.r2; }
__device__ __forceinline__ M3 mmul(const M3& A, const M3& B) { return {mrow(A.r0, B), mrow(A.r1, B), mrow(A.r2, B)}; }
__device__ __forceinline__ V3 symv(const S3& S, const V3 u) {
  return {(S.xx * u.x + S.xy * u.y) + S.xz * u.z, (S.xy * u.x + S.yy * u.y) + S.yz * u.z, (S.xz * u.x + S.yz * u.y) + S.zz * u.z};
}
__device__ __forceinline__ M3 rot3(const double (&a)[3], const double ang) {   // Rodrigues' formula about a unit axis
  double R[9];
  rodrigues(a, ang, R);
  return {{R[0], R[1], R[2]}, {R[3], R[4], R[5]}, {R[6], R[7], R[8]}};
}

// The chain of leg l at q in the torso frame, in leg_fk_jac's operation order: link orientations (torso <- HIP, THIGH, SHANK), joint
// axes, joint origins p0..p2 and the foot p3.
struct LegChain { M3 R0, R1, R2; V3 z0, z1, z2, p0, p1, p2, p3; };

__device__ __forceinline__ void leg_chain(const LegGeoDev& geo, const int l, const V3 q, LegChain& ch) {
  const V3 hx = {geo.hx[l][0], geo.hx[l][1], geo.hx[l][2]}, hy = {geo.hy[l][0], geo.hy[l][1], geo.hy[l][2]};
  const V3 kn = {geo.kn[0], geo.kn[1], geo.kn[2]}, ft = {geo.ft[0], geo.ft[1], geo.ft[2]};
  const V3 ax = {geo.ax[0], geo.ax[1], geo.ax[2]}, ay = {geo.ay[0], geo.ay[1], geo.ay[2]};
  ch.R0 = rot3(geo.ax, q.x);
  ch.R1 = mmul(ch.R0, rot3(geo.ay, q.y));
  ch.R2 = mmul(ch.R1, rot3(geo.ay, q.z));
  ch.p0 = hx;
  ch.p1 = hx + mv(ch.R0, hy);
  ch.p2 = ch.p1 + mv(ch.R1, kn);
  ch.p3 = ch.p2 + mv(ch.R2, ft);
  ch.z0 = mv(ch.R0, ax);
  ch.z1 = mv(ch.R1, ay);
  ch.z2 = mv(ch.R2, ay);
}

// What a link keeps between the outward and the inward pass: the force and moment its motion needs, its centre of mass and the next
// joint origin seen from its own joint origin.
struct LegLink { V3 F, N, rc, d; };

// Outward step over one link (inr its inertial rows): R its orientation, z its joint axis, p / pn its and the next joint origin.  w, al, ap (angular velocity,
// angular acceleration, acceleration of the joint origin) come in as the parent link's and go out as this link's / the next origin's.
template <bool VEL>
__device__ __forceinline__ void leg_link_out(const LegLinkInr& inr, const int l, const M3& R, const V3 z, const V3 p, const V3 pn, const V3 gb,
                                             const double qd, const double qdd, V3& w, V3& al, V3& ap, LegLink& L) {
  if constexpr (VEL) {
    const V3 t = cross(w, z);   // the axis turns with the link it hangs from
    al = (al + qdd * z) + qd * t;
    w = w + qd * z;
  } else {
    al = al + qdd * z;
  }
  const V3 cm = {inr.c[l][0], inr.c[l][1], inr.c[l][2]};
  const S3 S = {inr.I[l][0], inr.I[l][1], inr.I[l][2], inr.I[l][3], inr.I[l][4], inr.I[l][5]};
  const double mk = inr.m[l];
  L.rc = mv(R, cm);
  L.d = pn - p;
  V3 ac = ap + cross(al, L.rc), an = ap + cross(al, L.d);   // accelerations of the centre of mass and of the next joint origin
  L.N = mv(R, symv(S, mtv(R, al)));
  if constexpr (VEL) {
    ac = ac + cross(w, cross(w, L.rc));
    an = an + cross(w, cross(w, L.d));
    L.N = L.N + cross(w, mv(R, symv(S, mtv(R, w))));
    L.F = mk * (ac - gb);
  } else {
    L.F = mk * ac;
  }
  ap = an;
}

// Inward step: f, n the force and the moment (about the next joint origin) the outer links need; returns this joint's torque.
__device__ __forceinline__ double leg_link_in(const LegLink& L, const V3 z, V3& f, V3& n) {
  n = ((L.N + cross(L.rc, L.F)) + n) + cross(L.d, f);
  f = L.F + f;
  return dot(z, n);
}

// Inverse dynamics of leg l on the chain ch.  Everything is in the torso's axes: w0, al0, a0 the torso's angular velocity, angular
// acceleration and the acceleration of its origin, gb the gravity vector; qd, qdd the joint rates and accelerations.  tau = joint
// torques without a foot force, af = acceleration of the foot point.  VEL = false drops every velocity, base and gravity term: tau is
// then M(q) qdd, af = J(q) qdd.
template <bool VEL>
__device__ __forceinline__ void leg_rnea(const LegLinkInr& i0, const LegLinkInr& i1, const LegLinkInr& i2, const int l, const LegChain& ch, const V3 w0, const V3 al0, const V3 a0,
                                         const V3 gb, const V3 qd, const V3 qdd, V3& tau, V3& af) {
  V3 w = {0.0, 0.0, 0.0}, al = {0.0, 0.0, 0.0}, ap = {0.0, 0.0, 0.0};
  if constexpr (VEL) {   // the HipX joint's origin rides on the torso
    w = w0; al = al0;
    ap = (a0 + cross(al0, ch.p0)) + cross(w0, cross(w0, ch.p0));
  }
  LegLink L0, L1, L2;
  leg_link_out<VEL>(i0, l, ch.R0, ch.z0, ch.p0, ch.p1, gb, qd.x, qdd.x, w, al, ap, L0);
  leg_link_out<VEL>(i1, l, ch.R1, ch.z1, ch.p1, ch.p2, gb, qd.y, qdd.y, w, al, ap, L1);
  leg_link_out<VEL>(i2, l, ch.R2, ch.z2, ch.p2, ch.p3, gb, qd.z, qdd.z, w, al, ap, L2);
  af = ap;
  V3 f = {0.0, 0.0, 0.0}, n = {0.0, 0.0, 0.0};
  tau.z = leg_link_in(L2, ch.z2, f, n);
  tau.y = leg_link_in(L1, ch.z1, f, n);
  tau.x = leg_link_in(L0, ch.z0, f, n);
}

// Sum over the four lanes of a quad (DPP lane moves, no LDS), the same bits in all four: (v_l + v_{l^1}) + (v_{l^2} + v_{l^3}).
__device__ __forceinline__ double quad_sum(double v) {
  v = v + dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  return v + dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
}

// mpcqp_leg_dynamics: i = 4 b + leg.  qd / qdd / rot / base and each of tau / mass / bias may be null.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_leg_dynamics_kernel(const TIO* __restrict__ q, const TIO* __restrict__ qd, const TIO* __restrict__ qdd, const TIO* __restrict__ rot,
                          const TIO* __restrict__ base, const LegGeoDev geo, const LegLinkInr i0, const LegLinkInr i1, const LegLinkInr i2, const LegLimDev lim,
                          TIO* __restrict__ tau,
                          TIO* __restrict__ mass, TIO* __restrict__ bias, const int64_t B) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  M3 R = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  if (rot) {
    const TIO* r = rot + 9 * b;
    R = {{(double)r[0], (double)r[1], (double)r[2]}, {(double)r[3], (double)r[4], (double)r[5]}, {(double)r[6], (double)r[7], (double)r[8]}};
  }
  V3 bw = {0.0, 0.0, 0.0}, ba = {0.0, 0.0, 0.0}, bl = {0.0, 0.0, 0.0};   // the torso's omega, alpha and linear acceleration, world axes
  if (base) {
    const TIO* s = base + 9 * b;
    bw = {(double)s[0], (double)s[1], (double)s[2]};
    ba = {(double)s[3], (double)s[4], (double)s[5]};
    bl = {(double)s[6], (double)s[7], (double)s[8]};
  }
  const V3 zero = {0.0, 0.0, 0.0};
  const V3 ql = {(double)q[3 * i], (double)q[3 * i + 1], (double)q[3 * i + 2]};
  const V3 v = qd ? V3{(double)qd[3 * i], (double)qd[3 * i + 1], (double)qd[3 * i + 2]} : zero;
  const V3 a = qdd ? V3{(double)qdd[3 * i], (double)qdd[3 * i + 1], (double)qdd[3 * i + 2]} : zero;
  const V3 w0 = mtv(R, bw), al0 = mtv(R, ba), a0 = mtv(R, bl), gb = lim.g * R.r2;   // R^T: world -> torso axes
  LegChain ch;
  leg_chain(geo, l, ql, ch);
  V3 out, af;
  if (tau) {
    leg_rnea<true>(i0, i1, i2, l, ch, w0, al0, a0, gb, v, a, out, af);
    tau[3 * i] = (TIO)out.x; tau[3 * i + 1] = (TIO)out.y; tau[3 * i + 2] = (TIO)out.z;
  }
  if (bias) {
    leg_rnea<true>(i0, i1, i2, l, ch, w0, al0, a0, gb, v, zero, out, af);
    bias[3 * i] = (TIO)out.x; bias[3 * i + 1] = (TIO)out.y; bias[3 * i + 2] = (TIO)out.z;
  }
  if (mass) {   // column j of M(q): the torques of a unit acceleration of joint j
    leg_rnea<false>(i0, i1, i2, l, ch, zero, zero, zero, zero, zero, V3{1.0, 0.0, 0.0}, out, af);
    mass[9 * i] = (TIO)out.x; mass[9 * i + 3] = (TIO)out.y; mass[9 * i + 6] = (TIO)out.z;
    leg_rnea<false>(i0, i1, i2, l, ch, zero, zero, zero, zero, zero, V3{0.0, 1.0, 0.0}, out, af);
    mass[9 * i + 1] = (TIO)out.x; mass[9 * i + 4] = (TIO)out.y; mass[9 * i + 7] = (TIO)out.z;
    leg_rnea<false>(i0, i1, i2, l, ch, zero, zero, zero, zero, zero, V3{0.0, 0.0, 1.0}, out, af);
    mass[9 * i + 2] = (TIO)out.x; mass[9 * i + 5] = (TIO)out.y; mass[9 * i + 8] = (TIO)out.z;
  }
}

// mpcqp_leg_effort: mpcqp_joint_rates' rows plus foot_acc [rows,4,3], base_acc [rows,6] (either may be null) and, read only without
// base_acc, body [B,7] (null: model) -> qdd, tau_dyn, tau [rows,4,3], power [rows,4], limit u8 [rows,4], each of which may be null.
// Up to the call of leg_joints this is mpcqp_joint_rates_kernel's text.
// One (row, leg), i = 4 row + leg.  ACTROW (act_rows, mpcqp_actuators.h) is empty, or double: mpcqp_leg_effort_kernel<TIO, double> is
// the kernel with an actuator table set (include/mpcqp_actuators.h) and takes it, act [rows / T, 9], as one more argument; limit bit
// 4 is then the envelope of row (row / T) of the table at the row's qd, not lim.taumax, and an invalid row gives limit = 0xff.
template <typename TIO, typename... ACTROW>
__global__ void __launch_bounds__(256)
mpcqp_leg_effort_kernel(const TIO* __restrict__ actual, const TIO* __restrict__ forces, const TIO* __restrict__ feet,
                        const TIO* __restrict__ foot_vel, const TIO* __restrict__ foot_acc, const TIO* __restrict__ base_acc,
                        const TIO* __restrict__ body, const PlantModel model, const LegGeoDev geo, const LegLinkInr i0, const LegLinkInr i1,
                        const LegLinkInr i2, const LegLimDev lim,
                        TIO* __restrict__ qdd, TIO* __restrict__ tau_dyn, TIO* __restrict__ tau, TIO* __restrict__ power,
                        uint8_t* __restrict__ limit, const int64_t rows, const int64_t T, const ACTROW* __restrict__... actp) {
  constexpr bool ACT = sizeof...(ACTROW) != 0;
  const double* const act = act_rows(actp...);
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
  const M3 Rw = {{R[0], R[1], R[2]}, {R[3], R[4], R[5]}, {R[6], R[7], R[8]}};
  const V3 omv = {om[0], om[1], om[2]}, pv = {pw[0], pw[1], pw[2]}, fv = {f[0], f[1], f[2]};
  const V3 q = {ql[0], ql[1], ql[2]}, qv = {qr[0], qr[1], qr[2]}, tf = {tl[0], tl[1], tl[2]};   // (qv: 0 where the leg does not move)
  // the torso's angular acceleration and the CoM's acceleration, world axes
  V3 alw, aw;
  bool fin = true;
  if (base_acc) {
    const TIO* s = base_acc + 6 * row;
    alw = {(double)s[0], (double)s[1], (double)s[2]};
    aw = {(double)s[3], (double)s[4], (double)s[5]};
  } else {   // the unpushed plant's right-hand side at the row (plant_deriv's order)
    double bd[7];
    plant_body_row(body, model, row / T, bd);
    const double Ib[6] = {bd[1], bd[2], bd[3], bd[4], bd[5], bd[6]};
    double Ii[6];
    fin = plant_inertia(bd[0], Ib, Ii);
    // the four legs of a row are the four lanes of a quad: sum f_l and r_l x f_l across it, (l + l^1) + (l^2 + l^3)
    const V3 cr = cross(pv, fv);
    const V3 Fs = {quad_sum(fv.x), quad_sum(fv.y), quad_sum(fv.z)}, Ms = {quad_sum(cr.x), quad_sum(cr.y), quad_sum(cr.z)};
    const V3 wb = mtv(Rw, omv), tb = mtv(Rw, Ms);
    aw = {Fs.x / bd[0], Fs.y / bd[0], Fs.z / bd[0] + lim.g};
    const S3 SIb = {Ib[0], Ib[1], Ib[2], Ib[3], Ib[4], Ib[5]}, SIi = {Ii[0], Ii[1], Ii[2], Ii[3], Ii[4], Ii[5]};
    alw = mv(Rw, symv(SIi, tb - cross(wb, symv(SIb, wb))));
  }
  const V3 w0 = mtv(Rw, omv), al0 = mtv(Rw, alw), a0 = mtv(Rw, aw), gb = lim.g * Rw.r2;   // world -> torso axes
  const V3 fa = foot_acc ? V3{(double)foot_acc[3 * i], (double)foot_acc[3 * i + 1], (double)foot_acc[3 * i + 2]} : V3{0.0, 0.0, 0.0};
  const auto fin3 = [](const V3 u) { return isfinite(u.x) && isfinite(u.y) && isfinite(u.z); };
  fin = fin && fin3(alw) && fin3(aw) && fin3(fa) && fin3(fv) && fin3(qv) && fin3(q);
  const V3 zero = {0.0, 0.0, 0.0};
  LegChain ch;
  leg_chain(geo, l, q, ch);
  // J = d foot / d q from the chain (column j = z_j x (foot - p_j), leg_fk_jac's), its cofactors by row and its determinant, as the
  // rates form them: J^-1 = adj / det
  const V3 k0 = cross(ch.z0, ch.p3 - ch.p0), k1 = cross(ch.z1, ch.p3 - ch.p1), k2 = cross(ch.z2, ch.p3 - ch.p2);
  const double J0 = k0.x, J1 = k1.x, J2 = k2.x, J3 = k0.y, J4 = k1.y, J5 = k2.y, J6 = k0.z, J7 = k1.z, J8 = k2.z;
  const double c00 = J4 * J8 - J5 * J7, c01 = J5 * J6 - J3 * J8, c02 = J3 * J7 - J4 * J6;
  const double c10 = J2 * J7 - J1 * J8, c11 = J0 * J8 - J2 * J6, c12 = J1 * J6 - J0 * J7;
  const double c20 = J1 * J5 - J2 * J4, c21 = J2 * J3 - J0 * J5, c22 = J0 * J4 - J1 * J3;
  const double det = J0 * c00 + J1 * c01 + J2 * c02;
  const bool move = ok && det != 0.0;
  V3 t0, af, td;
  leg_rnea<true>(i0, i1, i2, l, ch, w0, al0, a0, gb, qv, zero, t0, af);   // af: the foot's acceleration when the joints do not accelerate
  const V3 h = mtv(Rw, fa) - af;
  const V3 qr3 = {(c00 * h.x + c10 * h.y + c20 * h.z) / det, (c01 * h.x + c11 * h.y + c21 * h.z) / det, (c02 * h.x + c12 * h.y + c22 * h.z) / det};
  const V3 qa = {move ? qr3.x : 0.0, move ? qr3.y : 0.0, move ? qr3.z : 0.0};
  leg_rnea<true>(i0, i1, i2, l, ch, w0, al0, a0, gb, qv, qa, td, af);
  const double nan = __builtin_nan("");
  const double pd = dot(td, qv);
  const V3 tt = tf + td;
  unsigned bits = ok ? 0u : 8u;
  bits |= (q.x < lim.qmin[0] || q.x > lim.qmax[0] || q.y < lim.qmin[1] || q.y > lim.qmax[1] || q.z < lim.qmin[2] || q.z > lim.qmax[2]) ? 1u : 0u;
  bits |= (fabs(qv.x) > lim.qdmax[0] || fabs(qv.y) > lim.qdmax[1] || fabs(qv.z) > lim.qdmax[2]) ? 2u : 0u;
  bool act_ok = true;
  if constexpr (ACT) {
    const double* ar = act + ACT_ROW * (row / T);
    bits |= (act_beyond(ar, 0, tt.x, qv.x) || act_beyond(ar, 1, tt.y, qv.y) || act_beyond(ar, 2, tt.z, qv.z)) ? 4u : 0u;
    act_ok = ar[0] == ar[0];
  } else {
    bits |= (fabs(tt.x) > lim.taumax[0] || fabs(tt.y) > lim.taumax[1] || fabs(tt.z) > lim.taumax[2]) ? 4u : 0u;
  }
  fin = fin && fin3(qa) && fin3(td) && fin3(tt);
  if (qdd) { qdd[3 * i] = (TIO)(fin ? qa.x : nan); qdd[3 * i + 1] = (TIO)(fin ? qa.y : nan); qdd[3 * i + 2] = (TIO)(fin ? qa.z : nan); }
  if (tau_dyn) { tau_dyn[3 * i] = (TIO)(fin ? td.x : nan); tau_dyn[3 * i + 1] = (TIO)(fin ? td.y : nan); tau_dyn[3 * i + 2] = (TIO)(fin ? td.z : nan); }
  if (tau) { tau[3 * i] = (TIO)(fin ? tt.x : nan); tau[3 * i + 1] = (TIO)(fin ? tt.y : nan); tau[3 * i + 2] = (TIO)(fin ? tt.z : nan); }
  if (power) power[i] = (TIO)(fin ? qr[3] + pd : nan);
  if (limit) limit[i] = (fin && act_ok) ? (uint8_t)bits : (uint8_t)0xff;
}

}  // namespace
