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
// ACTROW (act_rows, mpcqp_actuators.h) is empty, or double: mpcqp_swing_track_kernel<TIO, double> is the kernel with an actuator table
// set (include/mpcqp_actuators.h) and takes it, act [B,9], as one more argument; the clamp of a control period is then the envelope
// of row b of the table at the rate the period starts from, not lim.taumax.
template <typename TIO, typename... ACTROW>
__global__ void __launch_bounds__(256)
mpcqp_swing_track_kernel(const SwingIn<TIO> in, TIO* __restrict__ state, const PlantModel model, const LegGeoDev geo, const LegLinkInr i0,
                         const LegLinkInr i1, const LegLinkInr i2, const LegLimDev lim, const SwingOut<TIO> out, const int64_t B, const int T,
                         const int n, const double h, const ACTROW* __restrict__... actp) {
  constexpr bool ACT = sizeof...(ACTROW) != 0;
  const double* const act = act_rows(actp...);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;   // (whole quads: 4 B is a multiple of 4)
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  const V3 zero = {0.0, 0.0, 0.0};
  // the lane's own rows of the geometry and of the three links, selected once: the row loop below reads slot 0 of these copies
  LegGeoDev gl = geo;
  LegLinkInr j0, j1, j2;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    gl.hx[0][a] = geo.hx[l][a]; gl.hy[0][a] = geo.hy[l][a];
    j0.c[0][a] = i0.c[l][a]; j1.c[0][a] = i1.c[l][a]; j2.c[0][a] = i2.c[l][a];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) { j0.I[0][a] = i0.I[l][a]; j1.I[0][a] = i1.I[l][a]; j2.I[0][a] = i2.I[l][a]; }
  j0.m[0] = i0.m[l]; j1.m[0] = i1.m[l]; j2.m[0] = i2.m[l];
  double kp = SWING_KP, kd = SWING_KD;
  if (in.gains) { kp = (double)in.gains[2 * b]; kd = (double)in.gains[2 * b + 1]; }
  const bool gain_ok = isfinite(kp) && isfinite(kd) && kp >= 0.0 && kd >= 0.0;
  V3 sq = zero, sqd = zero;
  bool live = false;
  if (state) {
    sq = load3(state + 7 * i); sqd = load3(state + 7 * i + 3);
    live = !((double)state[7 * i + 6] == 0.0);
  }
  bool bad = live && !(fin3(sq) && fin3(sqd));
  // the robot's body row (read only without base_acc)
  double bd[7] = {1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0}, Ii[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool body_ok = true;
  if (!in.base_acc) {
    plant_body_row(in.body, model, b, bd);
    const double Ib[6] = {bd[1], bd[2], bd[3], bd[4], bd[5], bd[6]};
    body_ok = plant_inertia(bd[0], Ib, Ii);
  }
#pragma nounroll
  for (int t = 0; t < T; ++t) {
    const int64_t row = b * T + t, il = 4 * row + l;
    const TIO* x = in.actual + 12 * row;   // rotation vector, CoM, omega, v
    double qt[4];
    plant_rotvec_to_quat((double)x[0], (double)x[1], (double)x[2], qt);
    const M3 Rw = quat_rot(qt);
    const double R[9] = {Rw.r0.x, Rw.r0.y, Rw.r0.z, Rw.r1.x, Rw.r1.y, Rw.r1.z, Rw.r2.x, Rw.r2.y, Rw.r2.z};
    const V3 c = load3(x + 3), om = load3(x + 6), v = load3(x + 9);
    const TIO* sw = in.swing + 12 * il;    // pos, vel, acc, target
    const V3 pos = load3(sw), vel = load3(sw + 3), acc = load3(sw + 6);
    const V3 fv = load3(in.forces + 3 * il), held = load3(in.feet_log + 3 * il);
    const bool stance = in.contact[il] != 0;
    // the on-trajectory state of the row: mpcqp_joint_rates' q, qd and (R J)^T (-f) at the desired foot
    const V3 pv = pos - c, vrel = (vel - v) - cross(om, pv);
    const double pw[3] = {pv.x, pv.y, pv.z}, f[3] = {fv.x, fv.y, fv.z}, vr[3] = {vrel.x, vrel.y, vrel.z};
    double ql[3], tl[3], qr[4];
    const bool ok = leg_joints<true, true>(gl, 0, R, pw, f, ql, tl, vr, qr);
    const V3 q_on = {ql[0], ql[1], ql[2]}, qd_on = {qr[0], qr[1], qr[2]}, tau_f = {tl[0], tl[1], tl[2]};
    // the torso's angular acceleration and the CoM's acceleration over the tick, world axes
    V3 alw, aw;
    if (in.base_acc) {
      const TIO* s = in.base_acc + 6 * row;
      alw = load3(s); aw = load3(s + 3);
    } else {   // the unpushed plant's right-hand side at the row, as mpcqp_leg_effort forms it, over the feet the plant held
      const V3 cr = cross(held - c, fv);
      const V3 Fs = {quad_sum(fv.x), quad_sum(fv.y), quad_sum(fv.z)}, Ms = {quad_sum(cr.x), quad_sum(cr.y), quad_sum(cr.z)};
      const V3 wb = mtv(Rw, om), tb = mtv(Rw, Ms);
      aw = {Fs.x / bd[0], Fs.y / bd[0], Fs.z / bd[0] + lim.g};
      const S3 SIb = {bd[1], bd[2], bd[3], bd[4], bd[5], bd[6]}, SIi = {Ii[0], Ii[1], Ii[2], Ii[3], Ii[4], Ii[5]};
      alw = mv(Rw, symv(SIi, tb - cross(wb, symv(SIb, wb))));
    }
    bool fin = gain_ok && body_ok && fin3(alw) && fin3(aw) && fin3(c) && fin3(om) && fin3(v) && fin3(pos) && fin3(vel) && fin3(acc) &&
               fin3(fv) && fin3(held) && isfinite((double)x[0]) && isfinite((double)x[1]) && isfinite((double)x[2]);
    // a landing row logs the miss of the carried leg before the leg is re-initialised
    const bool landing = stance && live, init = stance || !live;
    const bool carried_bad = landing && bad;   // a poisoned swing ends NaN: its miss is not known
    LegChain ch;
    leg_chain(gl, 0, sq, ch);
    const double miss = norm3((c + mv(Rw, ch.p3)) - pos);
    sq = sel3(init, q_on, sq); sqd = sel3(init, qd_on, sqd);
    bad = init ? !fin : (bad || !fin);
    live = !stance;
    unsigned bits = (stance ? (landing ? 64u : 0u) : 1u) | ((init && !ok) ? 16u : 0u);
    leg_chain(gl, 0, sq, ch);
    const V3 foot = c + mv(Rw, ch.p3);
    const double err = landing ? miss : norm3(pos - foot);
    // what the row logs of the state is written now (the serial loop below is short of registers) and taken back after it, should the
    // row turn out non-finite there
    const bool good0 = !bad && !carried_bad && isfinite(err);
    if (out.q) store3(out.q + 3 * il, good0, sq);
    if (out.qd) store3(out.qd + 3 * il, good0, sqd);
    if (out.foot) store3(out.foot + 3 * il, good0, foot);
    if (out.err) out.err[il] = (TIO)(good0 ? err : __builtin_nan(""));
    V3 tau_log = tau_f;
    if (stance) {
      bits |= swing_limits(lim, sq, sqd);
    } else {
#pragma nounroll
      for (int k = 0; k < n; ++k) {
        const M3 Rk = quat_rot(qt);
        const double s = (double)k * h, s2 = 0.5 * s * s;
        const V3 cs = (c + s * v) + s2 * aw, vs = v + s * aw, oms = om + s * alw;
        const V3 pd = (pos + s * vel) + s2 * acc, vd = vel + s * acc;
        if (k) leg_chain(gl, 0, sq, ch);
        // J = d foot / d q of the chain (column j = z_j x (foot - p_j)), by rows
        const V3 k0 = cross(ch.z0, ch.p3 - ch.p0), k1 = cross(ch.z1, ch.p3 - ch.p1), k2 = cross(ch.z2, ch.p3 - ch.p2);
        const M3 J = {{k0.x, k1.x, k2.x}, {k0.y, k1.y, k2.y}, {k0.z, k1.z, k2.z}};
        const V3 rp = mv(Rk, ch.p3);
        const V3 jq = (sqd.x * k0 + sqd.y * k1) + sqd.z * k2;
        const V3 fvel = (vs + cross(oms, rp)) + mv(Rk, jq);
        const V3 F = kp * (pd - (cs + rp)) + kd * (vd - fvel);
        const V3 w0 = mtv(Rk, oms), al0 = mtv(Rk, alw), a0 = mtv(Rk, aw), gb = lim.g * Rk.r2;   // world -> torso axes
        V3 bias, af0;
        leg_rnea<true>(j0, j1, j2, 0, ch, w0, al0, a0, gb, sqd, zero, bias, af0);
        const M3 M = leg_mass(j0, j1, j2, 0, ch);
        double dj, dm;
        const V3 qx = adj_solve(J, mtv(Rk, acc) - af0, dj);
        const V3 qdes = sel3(dj != 0.0, qx, zero);
        const V3 gF = mtv(Rk, F);
        const V3 cmd = (V3{dot(k0, gF), dot(k1, gF), dot(k2, gF)} + mv(M, qdes)) + bias;
        V3 app;
        if constexpr (ACT) {   // (the row is read here, period by period: nothing of it is held across the loop)
          const double* ar = act_row_here(act + ACT_ROW * b);
          app = {act_clamp(ar, 0, cmd.x, sqd.x), act_clamp(ar, 1, cmd.y, sqd.y), act_clamp(ar, 2, cmd.z, sqd.z)};
        } else {
          app = {clamp_sym(cmd.x, lim.taumax[0]), clamp_sym(cmd.y, lim.taumax[1]), clamp_sym(cmd.z, lim.taumax[2])};
        }
        const V3 ax = adj_solve(M, app - bias, dm);
        const V3 qdd = sel3(dm != 0.0, ax, zero);
        bits |= swing_limits(lim, sq, sqd) | ((app.x != cmd.x || app.y != cmd.y || app.z != cmd.z) ? 2u : 0u) | (dj == 0.0 ? 16u : 0u);
        if (k == 0) tau_log = app;
        sqd = sqd + h * qdd;
        sq = sq + h * sqd;
        // the torso's orientation: one Euler step of the plant's quaternion rate at omega(s), renormalised
        const double qw = qt[0], qxx = qt[1], qy = qt[2], qz = qt[3];
        const double d0 = 0.5 * (-((oms.x * qxx + oms.y * qy) + oms.z * qz)), d1 = 0.5 * (qw * oms.x + (oms.y * qz - oms.z * qy));
        const double d2 = 0.5 * (qw * oms.y + (oms.z * qxx - oms.x * qz)), d3 = 0.5 * (qw * oms.z + (oms.x * qy - oms.y * qxx));
        qt[0] = qw + h * d0; qt[1] = qxx + h * d1; qt[2] = qy + h * d2; qt[3] = qz + h * d3;
        const double nq = sqrt(((qt[0] * qt[0] + qt[1] * qt[1]) + qt[2] * qt[2]) + qt[3] * qt[3]);
        qt[0] = qt[0] / nq; qt[1] = qt[1] / nq; qt[2] = qt[2] / nq; qt[3] = qt[3] / nq;
      }
      bad = bad || !(fin3(sq) && fin3(sqd));
    }
    const bool good = good0 && !bad && fin3(tau_log);
    if (out.tau) store3(out.tau + 3 * il, good, tau_log);
    if (out.flag) out.flag[il] = good ? (uint8_t)bits : (uint8_t)0xff;
    if (good0 && !good) {
      if (out.q) store3(out.q + 3 * il, false, zero);
      if (out.qd) store3(out.qd + 3 * il, false, zero);
      if (out.foot) store3(out.foot + 3 * il, false, zero);
      if (out.err) out.err[il] = (TIO)__builtin_nan("");
    }
  }
  if (state) {
    store3(state + 7 * i, !bad, sq);
    store3(state + 7 * i + 3, !bad, sqd);
    state[7 * i + 6] = (TIO)(live ? 1.0 : 0.0);
  }
}

}  // namespace
