// The text of mpcqp_stance_drive_kernel and mpcqp_stance_drive_act_kernel (mpcqp_drive.h, which includes it once in each): the rule for
// one (robot, leg), i = 4 b + leg.  ACT (a constant of the including kernel): the joint rates with the foot at rest in the world,
// J^-1 R^T (-v - omega x (foot - c)) from x[6..11] by leg_joints<true, true> (0 out of reach or where det J = 0), enter the envelope of
// row b of `act`.
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  const TIO* xb = x + 13 * b;   // rotation vector, CoM, ...
  const TIO* fb = f + b * fstride + 3 * l;
  const TIO fr[3] = {fb[0], fb[1], fb[2]};
  bool stance;
  if (contact) {
    stance = contact[i] != 0;
  } else {
    const GaitLeg gc = gait_leg(gait + b * GAIT_ROW, l);
    stance = gait_phase(gc, (uint32_t)max(tick[b], 0)) < gc.st;
  }
  // mpcqp_joint_log's row: R from the rotation vector, the foot seen from the CoM, q and tau_cmd
  double qt[4], pw[3], fl[3], ql[3], tl[3];
  plant_rotvec_to_quat((double)xb[0], (double)xb[1], (double)xb[2], qt);
  const double qw = qt[0], qx = qt[1], qy = qt[2], qz = qt[3];
  const double R[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                       2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                       2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    pw[a] = (double)feet[3 * i + a] - (double)xb[3 + a];
    fl[a] = (double)fr[a];
  }
  bool reach;
  V3 rate = {0.0, 0.0, 0.0};
  if constexpr (ACT) {
    const double om[3] = {(double)xb[6], (double)xb[7], (double)xb[8]};
    double wxr[3], vr[3], qr[4];
    cross3(om, pw, wxr);
#pragma unroll
    for (int a = 0; a < 3; ++a) vr[a] = (0.0 - (double)xb[9 + a]) - wxr[a];
    reach = leg_joints<true, true>(geo, l, R, pw, fl, ql, tl, vr, qr);
    rate = {qr[0], qr[1], qr[2]};
  } else {
    reach = leg_joints<true>(geo, l, R, pw, fl, ql, tl);
  }
  double pf[3], J[9];
  leg_fk_jac(geo, l, ql, pf, J);
  const V3 fv = {fl[0], fl[1], fl[2]}, tc = {tl[0], tl[1], tl[2]}, q = {ql[0], ql[1], ql[2]}, zero = {0.0, 0.0, 0.0};
  const double mu = ground ? (double)ground[b] : 0.0;
  V3 fo, to;
  unsigned bits;
  if constexpr (ACT) bits = drive_rule<true>(R, J, reach, fv, tc, lim, drive == DRIVE_LIMITED, ground != nullptr, mu, fo, to, act + ACT_ROW * b, rate);
  else bits = drive_rule(R, J, reach, fv, tc, lim, drive == DRIVE_LIMITED, ground != nullptr, mu, fo, to);
  bits |= swing_limits(lim, q, zero);   // 4: q outside its limits
  // the robot's x and ground row poison its four legs, a leg's own operands that leg
  bool robot = isfinite(mu) && mu >= 0.0;
#pragma unroll
  for (int a = 0; a < 12; ++a) robot = robot && isfinite((double)xb[a]);
  const bool good = robot && (!stance || (fin3(fv) && isfinite(pw[0]) && isfinite(pw[1]) && isfinite(pw[2]) && fin3(fo) && fin3(to)));
  const double nan = __builtin_nan("");
  TIO* fw = f_out + 12 * b + 3 * l;
  if (cmd) {
    TIO* cw = cmd + b * cstride + 3 * l;
    cw[0] = fr[0]; cw[1] = fr[1]; cw[2] = fr[2];
  }
  // a swing leg keeps its commanded force as read
  fw[0] = good ? (stance ? (TIO)fo.x : fr[0]) : (TIO)nan;
  fw[1] = good ? (stance ? (TIO)fo.y : fr[1]) : (TIO)nan;
  fw[2] = good ? (stance ? (TIO)fo.z : fr[2]) : (TIO)nan;
  if (tau) store3(tau + 3 * i, good, sel3(stance, to, zero));
  if (flag) flag[i] = good ? (uint8_t)(stance ? bits : 0u) : (uint8_t)0xff;
