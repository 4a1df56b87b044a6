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
// ACTROW (act_rows, mpcqp_actuators.h) is empty, or double: mpcqp_legs_step_kernel<TIO, double> is the kernel with an actuator table
// set (include/mpcqp_actuators.h) and takes it, act [B,9], as one more argument; the clamp of a control period is then the envelope
// of row b of the table at the rate the period starts from, not lim.taumax.
template <typename TIO, typename... ACTROW>
__global__ void __launch_bounds__(256)
mpcqp_legs_step_kernel(const TIO* __restrict__ x, const TIO* __restrict__ ref, const PhaseRows<TIO> ph, const int32_t* __restrict__ tick,
                       const TIO* __restrict__ u, const TIO* __restrict__ step_height, const TIO* __restrict__ gains,
                       double* __restrict__ legs, const PlantIn<TIO> pin, const LegGeoDev geo, const LegLinkInr i0, const LegLinkInr i1,
                       const LegLinkInr i2, const LegLimDev lim, const LegRollOut<TIO> out, const double d, const int N, const int64_t B,
                       const int T, const int it, const int n, const double h, const ACTROW* __restrict__... actp) {
  constexpr bool ACT = sizeof...(ACTROW) != 0;
  const double* const act = act_rows(actp...);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;   // (whole quads: 4 B is a multiple of 4)
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  const V3 zero = {0.0, 0.0, 0.0};
  // the lane's own rows of the geometry and of the three links, selected once
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
  if (gains) { kp = (double)gains[2 * b]; kd = (double)gains[2 * b + 1]; }
  const bool gain_ok = isfinite(kp) && isfinite(kd) && kp >= 0.0 && kd >= 0.0;
  V3 sq = {legs[7 * i], legs[7 * i + 1], legs[7 * i + 2]}, sqd = {legs[7 * i + 3], legs[7 * i + 4], legs[7 * i + 5]};
  bool live = !(legs[7 * i + 6] == 0.0);
  bool bad = live && !(fin3(sq) && fin3(sqd));
  double bd[7], Ii[6];
  plant_body_row(pin.body, pin.model, b, bd);
  const double Ib[6] = {bd[1], bd[2], bd[3], bd[4], bd[5], bd[6]};
  const bool body_ok = plant_inertia(bd[0], Ib, Ii);
  // the row of the tick, from the live buffers
  const int64_t row = b * T + it, il = 4 * row + l;
  const TIO* xb = x + 13 * b;   // rotation vector, CoM, omega, v
  const TIO* rf = ref + 10 * b;
  const int tk = tick[b];
  const GaitLeg gc = gait_leg(ph.gait + b * GAIT_ROW, l);
  const int phi = gait_phase(gc, (uint32_t)max(tk, 0));
  const bool stance = phi < gc.st;
  double o[12];
  legroll_swing_row(xb, rf, ph.feet + 12 * b + 3 * l, ph.stand + 12 * b + 3 * l, gc, phi, phase_rows_finite(ph, b), (double)step_height[b],
                    ph.gain ? (double)ph.gain[b] : 0.0, d, o);
  // ... as the I/O type holds it: what mpcqp_swing_track would read from mpcqp_phase_swing's output
#pragma unroll
  for (int e = 0; e < 12; ++e) o[e] = (double)(TIO)o[e];
  if (out.swing) {
#pragma unroll
    for (int e = 0; e < 12; ++e) out.swing[12 * il + e] = (TIO)o[e];
  }
  const V3 pos = {o[0], o[1], o[2]}, vel = {o[3], o[4], o[5]}, acc = {o[6], o[7], o[8]};
  double qt[4];
  plant_rotvec_to_quat((double)xb[0], (double)xb[1], (double)xb[2], qt);
  const M3 Rw = quat_rot(qt);
  const double R[9] = {Rw.r0.x, Rw.r0.y, Rw.r0.z, Rw.r1.x, Rw.r1.y, Rw.r1.z, Rw.r2.x, Rw.r2.y, Rw.r2.z};
  const V3 c = load3(xb + 3), om = load3(xb + 6), v = load3(xb + 9);
  const V3 fv = load3(u + (size_t)b * N * 12 + 3 * l), held = load3(ph.feet + 12 * b + 3 * l);
  // the on-trajectory state of the row: mpcqp_joint_rates' q, qd and (R J)^T (-f) at the desired foot
  const V3 pv = pos - c, vrel = (vel - v) - cross(om, pv);
  const double pw[3] = {pv.x, pv.y, pv.z}, f[3] = {fv.x, fv.y, fv.z}, vr[3] = {vrel.x, vrel.y, vrel.z};
  double ql[3], tl[3], qr[4];
  const bool ok = leg_joints<true, true>(gl, 0, R, pw, f, ql, tl, vr, qr);
  const V3 q_on = {ql[0], ql[1], ql[2]}, qd_on = {qr[0], qr[1], qr[2]}, tau_f = {tl[0], tl[1], tl[2]};
  // the torso's angular acceleration and the CoM's acceleration over the tick, world axes: the plant's right-hand side at the row over
  // the feet the plant holds, with the robot's push where its window is open
  const bool pushed = pin.push && pin.push_ticks[2 * b] <= tk && tk < pin.push_ticks[2 * b + 1];
  V3 Fp = zero, Tp = zero;
  if (pushed) { Fp = load3(pin.push + 6 * b); Tp = load3(pin.push + 6 * b + 3); }
  const V3 cr = cross(held - c, fv);
  const V3 Fs = V3{quad_sum(fv.x), quad_sum(fv.y), quad_sum(fv.z)} + Fp, Ms = V3{quad_sum(cr.x), quad_sum(cr.y), quad_sum(cr.z)} + Tp;
  const V3 wb = mtv(Rw, om), tb = mtv(Rw, Ms);
  const V3 aw64 = {Fs.x / bd[0], Fs.y / bd[0], Fs.z / bd[0] + lim.g};
  const S3 SIb = {bd[1], bd[2], bd[3], bd[4], bd[5], bd[6]}, SIi = {Ii[0], Ii[1], Ii[2], Ii[3], Ii[4], Ii[5]};
  const V3 alw64 = mv(Rw, symv(SIi, tb - cross(wb, symv(SIb, wb))));
  // ... as the I/O type holds it, like the swing row: the base_acc row mpcqp_swing_track would have to be handed for this tick
  const V3 aw = {(double)(TIO)aw64.x, (double)(TIO)aw64.y, (double)(TIO)aw64.z};
  const V3 alw = {(double)(TIO)alw64.x, (double)(TIO)alw64.y, (double)(TIO)alw64.z};
  const bool fin = gain_ok && body_ok && fin3(alw) && fin3(aw) && fin3(c) && fin3(om) && fin3(v) && fin3(pos) && fin3(vel) && fin3(acc) &&
                   fin3(fv) && fin3(held) && isfinite((double)xb[0]) && isfinite((double)xb[1]) && isfinite((double)xb[2]);
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
  // what the row logs of the state is written now and taken back after the control periods, should the row turn out non-finite there
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
      if constexpr (ACT) {   // (the row is read here, period by period: the kernel has no registers to hold it across the loop)
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
  store3(legs + 7 * i, !bad, sq);
  store3(legs + 7 * i + 3, !bad, sqd);
  legs[7 * i + 6] = live ? 1.0 : 0.0;
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
