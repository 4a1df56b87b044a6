// The text of mpcqp_leg_effort_kernel and mpcqp_leg_effort_act_kernel (mpcqp_legdyn.h, which includes it once in each): one (row, leg),
// i = 4 row + leg.  ACT (a constant of the including kernel): limit bit 4 is the envelope of row (row / T) of `act` at the row's qd, not
// lim.taumax, and an invalid row gives limit = 0xff.
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
