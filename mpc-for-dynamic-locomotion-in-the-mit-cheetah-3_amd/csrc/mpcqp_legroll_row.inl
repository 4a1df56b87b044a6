// The text of mpcqp_legs_step_kernel and mpcqp_legs_step_act_kernel (mpcqp_legroll.h, which includes it once in each): the legs step of
// tick `it`, i = 4 b + leg.  ACT (a constant of the including kernel): the clamp of a control period is the envelope of row b of `act` at
// the rate the period starts from, not lim.taumax.
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
