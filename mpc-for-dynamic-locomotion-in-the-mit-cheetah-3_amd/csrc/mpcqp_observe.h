// mpcqp_observe.h -- sensors and the state estimator inside the slip roll-out's tick loop (the C-ABI is include/mpcqp_observe.h, which
// has the rule; the entry point lives in mpcqp_kernels.hip).  Two kernels around the unchanged kernels of mpcqp_rollout_slip:
//   mpcqp_observe_update_kernel    before the expand: the tick's encoder and gyro rows from the live buffers, then steps 1-3 of
//                                  mpcqp_estimate_track's row on est_state -- the fresh start, the scalar updates, the outputs -- and the
//                                  state the controller may read, x^ [B,13] and f^eet [B,4,3], in a side buffer
//   mpcqp_observe_predict_kernel   after the slip rule, before the legs step: the accelerometer row from the applied forces, the imu log
//                                  row, and step 4 of the filter's row on est_state
// Four lanes per robot, the mapping of mpcqp_estimate_track_kernel: in the update lane l does leg l's encoder and forward map, in both
// kernels lanes 0..2 own one axis each (xi[a] and the upper triangle of P[a] in registers, every index a constant) and lane 3 the
// orientation's outputs; quad exchanges by DPP lane moves, no LDS, no scratch.  The filter's arithmetic is the est_* helpers, est_update
// and est_leg of mpcqp_estimate.h, not contracted; the encoder row is legroll_swing_row and leg_joints<true, true> with the operands and
// the order of mpcqp_legs_step_kernel.  Between the two kernels the state passes through est_state in fp64, so the two halves of a row
// are the row of mpcqp_estimate_track_kernel bit for bit.  Poison is the state itself: a robot whose row is not finite gets a NaN
// state, and a NaN state poisons every later row.
// mpcqp_rollout_observe_gated (include/mpcqp_gate.h) launches the update kernel's GATE variant: the same kernel with est_gate between
// steps 1 and 2, which leaves the gated trust where the update leaves "the trust of step 1" for the predict kernel; the predict kernel,
// the side buffers and the launch count are the ungated call's.
#pragma once
#include "mpcqp_estimate.h"
#include "mpcqp_legroll.h"
#include "../../include/mpcqp_observe.h"

namespace {

constexpr int OBS_SENSE = 8;   // the sensor row step 4 reads back, per robot: gyro [3], trust [4], one spare

// The optional operands of the update (each may be null), the side buffers, and the logs (each may be null).
template <typename TIO>
struct ObsIn { const TIO *est_init, *height, *bias, *noise, *enc_noise; };
template <typename TIO>
struct ObsWs { TIO *xhat, *feet, *sense; };   // [B,13], [B,4,3], [B,OBS_SENSE]
template <typename TIO>
struct ObsOut { TIO *imu, *q_enc, *qd_enc, *est, *feet_est, *sigma, *nis; };

template <typename TIO>
__device__ __forceinline__ double obs_io(const double v) { return (double)(TIO)v; }   // a value as the I/O type holds it

// The estimator's log rows of a poisoned robot: lanes 0..2 their axis, lane 3 the orientation's.
template <typename TIO>
__device__ __forceinline__ void obs_nan_row(const ObsOut<TIO>& out, const int64_t row, const int l) {
  const TIO nan = (TIO)__builtin_nan("");
  if (l < 3) {
    if (out.est) { out.est[12 * row + 3 + l] = nan; out.est[12 * row + 9 + l] = nan; }
    if (out.feet_est) {
#pragma unroll
      for (int j = 0; j < 4; ++j) out.feet_est[3 * (4 * row + j) + l] = nan;
    }
    if (out.sigma) { out.sigma[6 * row + l] = nan; out.sigma[6 * row + 3 + l] = nan; }
  } else {
    if (out.est) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { out.est[12 * row + c] = nan; out.est[12 * row + 6 + c] = nan; }
    }
    if (out.nis) out.nis[row] = nan;
  }
}

// The encoders of leg l at the live tick, before noise: the carried joint state of a leg that is in swing on the clock and live, else the
// on-trajectory state mpcqp_legs_step_kernel will form for the row -- its operands in its order -- with a held foot moving at its slip
// velocity.  gl holds the leg's own geometry rows in slot 0.  (Contracted like the legs step: not part of the filter's arithmetic.)
template <typename TIO>
__device__ __forceinline__ void obs_encoders(const TIO* __restrict__ xb, const TIO* __restrict__ rf, const PhaseRows<TIO>& ph, const int64_t b,
                                             const int l, const GaitLeg& gc, const int phi, const double* __restrict__ slip2,
                                             const double* __restrict__ leg7, const double hh, const double d, const LegGeoDev& gl, V3& qe,
                                             V3& qde) {
  const bool stance = phi < gc.st;
  const bool carried = !stance && !(leg7[6] == 0.0);
  double o[12];
  legroll_swing_row(xb, rf, ph.feet + 12 * b + 3 * l, ph.stand + 12 * b + 3 * l, gc, phi, phase_rows_finite(ph, b), hh,
                    ph.gain ? (double)ph.gain[b] : 0.0, d, o);
#pragma unroll
  for (int e = 0; e < 12; ++e) o[e] = (double)(TIO)o[e];
  const V3 pos = {o[0], o[1], o[2]};
  // (the slip velocity as the I/O type holds it, like the swing row: the foot_vel row mpcqp_joint_rates would be handed)
  const V3 vel = stance ? V3{(double)(TIO)slip2[0], (double)(TIO)slip2[1], 0.0} : V3{o[3], o[4], o[5]};
  double qt[4];
  plant_rotvec_to_quat((double)xb[0], (double)xb[1], (double)xb[2], qt);
  const M3 Rw = quat_rot(qt);
  const double R[9] = {Rw.r0.x, Rw.r0.y, Rw.r0.z, Rw.r1.x, Rw.r1.y, Rw.r1.z, Rw.r2.x, Rw.r2.y, Rw.r2.z};
  const V3 c = load3(xb + 3), om = load3(xb + 6), v = load3(xb + 9);
  const V3 pv = pos - c, vrel = (vel - v) - cross(om, pv);
  const double pw[3] = {pv.x, pv.y, pv.z}, f[3] = {0.0, 0.0, 0.0}, vr[3] = {vrel.x, vrel.y, vrel.z};
  double ql[3], tl[3], qr[4];
  (void)leg_joints<true, true>(gl, 0, R, pw, f, ql, tl, vr, qr);
  qe = carried ? V3{leg7[0], leg7[1], leg7[2]} : V3{ql[0], ql[1], ql[2]};
  qde = carried ? V3{leg7[3], leg7[4], leg7[5]} : V3{qr[0], qr[1], qr[2]};
}

// Sense and update of tick `it`: i = 4 b + lane.  GATE (mpcqp_rollout_observe_gated) adds step 1g of the filter's row (est_gate,
// include/mpcqp_gate.h): the sensor row the predict reads back then carries w in the place of the clock's trust, and trust_log (may be
// null) gets the row's w; without it `gate` and `trust_log`, the last two arguments, are not read.
template <typename TIO, bool GATE>
__global__ void __launch_bounds__(256)
mpcqp_observe_update_kernel(const TIO* __restrict__ x, const TIO* __restrict__ ref, const PhaseRows<TIO> ph, const int32_t* __restrict__ tick,
                            const double* __restrict__ slip, const double* __restrict__ legs, const TIO* __restrict__ step_height,
                            const ObsIn<TIO> in, const EstPar par, const LegGeoDev geo, double* state, const ObsWs<TIO> ws,
                            const ObsOut<TIO> out, const double d, const int64_t B, const int T, const int it, const EstGate gate,
                            TIO* __restrict__ trust_log) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;   // (whole quads leave: the lane moves below see all four lanes or none)
  const int l = (int)(i % 4), a = l < 3 ? l : 2;
  const int64_t b = i / 4, row = b * T + it, il = 4 * row + l;
  const double nan = __builtin_nan("");
  const TIO* xb = x + 13 * b;
  // ---- the encoders of leg l
  LegGeoDev gl = geo;
#pragma unroll
  for (int c = 0; c < 3; ++c) { gl.hx[0][c] = geo.hx[l][c]; gl.hy[0][c] = geo.hy[l][c]; }
  const GaitLeg gc = gait_leg(ph.gait + b * GAIT_ROW, l);
  const int phi = gait_phase(gc, (uint32_t)max(tick[b], 0));
  const bool stance = phi < gc.st;
  V3 qe, qde;
  obs_encoders(xb, ref + 10 * b, ph, b, l, gc, phi, slip + 2 * i, legs + 7 * i, (double)step_height[b], d, gl, qe, qde);
  bool mine = true;   // this lane's operands are finite
  if (in.enc_noise) {
    const V3 nq = load3(in.enc_noise + 6 * il), nd = load3(in.enc_noise + 6 * il + 3);
    qe = est_add(qe, nq); qde = est_add(qde, nd);
  }
  qe = {obs_io<TIO>(qe.x), obs_io<TIO>(qe.y), obs_io<TIO>(qe.z)};
  qde = {obs_io<TIO>(qde.x), obs_io<TIO>(qde.y), obs_io<TIO>(qde.z)};
  if (out.q_enc) store3(out.q_enc + 3 * il, true, qe);
  if (out.qd_enc) store3(out.qd_enc + 3 * il, true, qde);
  mine = mine && fin3(qe) && fin3(qde);
  // ---- the gyro, as mpcqp_imu_log_kernel forms it, and the trust from the clock
  V3 gy;
  {
    const V3 om = load3(xb + 6);
    double qt[4];
    plant_rotvec_to_quat((double)xb[0], (double)xb[1], (double)xb[2], qt);
    gy = est_mtv(est_rot(qt), om);
    bool fin = isfinite((double)xb[0]) && isfinite((double)xb[1]) && isfinite((double)xb[2]) && fin3(om);
    if (in.bias) {
      const V3 bg = load3(in.bias + 6 * b), ba = load3(in.bias + 6 * b + 3);
      gy = est_add(gy, bg);
      fin = fin && fin3(bg) && fin3(ba);
    }
    if (in.noise) {
      const V3 ng = load3(in.noise + 6 * row), na = load3(in.noise + 6 * row + 3);
      gy = est_add(gy, ng);
      fin = fin && fin3(ng) && fin3(na);
    }
    gy = {fin ? obs_io<TIO>(gy.x) : nan, fin ? obs_io<TIO>(gy.y) : nan, fin ? obs_io<TIO>(gy.z) : nan};
  }
  mine = mine && fin3(gy);
  const double tme = stance ? 1.0 : 0.0;
  double tr[4] = {quad_bcast<0>(tme), quad_bcast<1>(tme), quad_bcast<2>(tme), quad_bcast<3>(tme)};
  if constexpr (!GATE) {
    if (l == 3) {
      TIO* s = ws.sense + OBS_SENSE * b;
      store3(s, true, gy);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[3 + j] = (TIO)tr[j];
    }
  }
  // ---- the filter state: a fresh start from est_init (null: the robot's x as stored), or est_state
  double* const sb = state + b * EST_STATE;
  const bool fresh = sb[EST_LIVE] == 0.0;
  double qh[4], xi[6], U[21], hl[4] = {0.0, 0.0, 0.0, 0.0};
  if (fresh) {
    const TIO* x0 = in.est_init ? in.est_init + 12 * b : xb;
#pragma unroll
    for (int c = 0; c < 3; ++c) mine = mine && isfinite((double)x0[c]) && isfinite((double)x0[3 + c]) && isfinite((double)x0[9 + c]);
    plant_rotvec_to_quat((double)x0[0], (double)x0[1], (double)x0[2], qh);
    xi[0] = (double)x0[3 + a]; xi[1] = (double)x0[9 + a];
#pragma unroll
    for (int c = 2; c < 6; ++c) xi[c] = 0.0;   // (the feet are set below, from the row's rho)
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) U[est_ut(r, c)] = r != c ? 0.0 : (r == 0 ? par.p0p : (r == 1 ? par.p0v : par.p0f));
  } else {
    mine = mine && isfinite(sb[EST_LIVE]);
#pragma unroll
    for (int c = 0; c < 4; ++c) { qh[c] = sb[c]; mine = mine && isfinite(qh[c]); }
#pragma unroll
    for (int c = 0; c < 6; ++c) { xi[c] = sb[EST_XI + 6 * a + c]; mine = mine && isfinite(xi[c]); }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) { U[est_ut(r, c)] = sb[EST_P + 36 * a + 6 * r + c]; mine = mine && isfinite(U[est_ut(r, c)]); }
  }
  if (in.height) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { hl[j] = (double)in.height[4 * b + j]; mine = mine && isfinite(hl[j]); }
  }
  const bool hgt = in.height != nullptr && a == 2;
  float bad = mine ? 0.0f : 1.0f;
  bad = bad + dpp_mov<0xB1>(bad);
  bad = bad + dpp_mov<0x4E>(bad);
  const bool ok = bad == 0.0f;   // the robot's flag: the same in its four lanes
  // 1. the leg's foot and its velocity relative to the CoM, world axes
  const M3 R = est_rot(qh);
  const double ql[3] = {qe.x, qe.y, qe.z};
  double pf[3], J[9];
  leg_fk_jac(gl, 0, ql, pf, J);
  const V3 pb = {pf[0], pf[1], pf[2]};
  const V3 jq = {(J[0] * qde.x + J[1] * qde.y) + J[2] * qde.z, (J[3] * qde.x + J[4] * qde.y) + J[5] * qde.z,
                 (J[6] * qde.x + J[7] * qde.y) + J[8] * qde.z};
  const V3 rho = est_mv(R, pb), rhod = est_mv(R, est_add(est_cross(gy, pb), jq));
  const double zr[4] = {est_pick(a, quad_bcast<0>(rho.x), quad_bcast<0>(rho.y), quad_bcast<0>(rho.z)),
                        est_pick(a, quad_bcast<1>(rho.x), quad_bcast<1>(rho.y), quad_bcast<1>(rho.z)),
                        est_pick(a, quad_bcast<2>(rho.x), quad_bcast<2>(rho.y), quad_bcast<2>(rho.z)),
                        est_pick(a, quad_bcast<3>(rho.x), quad_bcast<3>(rho.y), quad_bcast<3>(rho.z))};
  const double zv[4] = {est_pick(a, quad_bcast<0>(rhod.x), quad_bcast<0>(rhod.y), quad_bcast<0>(rhod.z)),
                        est_pick(a, quad_bcast<1>(rhod.x), quad_bcast<1>(rhod.y), quad_bcast<1>(rhod.z)),
                        est_pick(a, quad_bcast<2>(rhod.x), quad_bcast<2>(rhod.y), quad_bcast<2>(rhod.z)),
                        est_pick(a, quad_bcast<3>(rhod.x), quad_bcast<3>(rhod.y), quad_bcast<3>(rhod.z))};
  if (fresh) {
#pragma unroll
    for (int j = 0; j < 4; ++j) xi[2 + j] = xi[0] + zr[j];
  }
  // 1g. the gate: tr becomes w, which is what the predict reads back (a poisoned robot's predict does not use it: its state is NaN)
  if constexpr (GATE) {
    est_gate<TIO>(gate, par, xi, U, zv, tr);
    if (l == 3) {
      TIO* s = ws.sense + OBS_SENSE * b;
      store3(s, true, gy);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[3 + j] = (TIO)tr[j];
      if (trust_log) {
#pragma unroll
        for (int j = 0; j < 4; ++j) trust_log[4 * row + j] = (TIO)(ok ? tr[j] : nan);
      }
    }
  }
  // 2. the scalar updates
  double na = 0.0;
  est_leg<0>(par, xi, U, zr[0], zv[0], tr[0], hgt, hl[0], na);
  est_leg<1>(par, xi, U, zr[1], zv[1], tr[1], hgt, hl[1], na);
  est_leg<2>(par, xi, U, zr[2], zv[2], tr[2], hgt, hl[2], na);
  est_leg<3>(par, xi, U, zr[3], zv[3], tr[3], hgt, hl[3], na);
  const double nis = (quad_bcast<0>(na) + quad_bcast<1>(na)) + quad_bcast<2>(na);
  // 3. outputs, the controller's side buffers and the posterior: lanes 0..2 their axis, lane 3 the orientation's
  const V3 omh = est_mv(R, gy);
  if (l < 3) {
    const TIO ep = (TIO)(ok ? xi[0] : nan), ev = (TIO)(ok ? xi[1] : nan);
    if (out.est) { out.est[12 * row + 3 + a] = ep; out.est[12 * row + 9 + a] = ev; }
    ws.xhat[13 * b + 3 + a] = ep; ws.xhat[13 * b + 9 + a] = ev;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const TIO ef = (TIO)(ok ? xi[2 + j] : nan);
      if (out.feet_est) out.feet_est[3 * (4 * row + j) + a] = ef;
      ws.feet[12 * b + 3 * j + a] = ef;
    }
    if (out.sigma) { out.sigma[6 * row + a] = (TIO)(ok ? sqrt(U[est_ut(0, 0)]) : nan); out.sigma[6 * row + 3 + a] = (TIO)(ok ? sqrt(U[est_ut(1, 1)]) : nan); }
#pragma unroll
    for (int c = 0; c < 6; ++c) sb[EST_XI + 6 * a + c] = ok ? xi[c] : nan;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) sb[EST_P + 36 * a + 6 * r + c] = ok ? U[est_sym(r, c)] : nan;
  } else {
    double th[3];
    plant_quat_to_rotvec(qh, th);
    if (out.est) {
      store3(out.est + 12 * row, ok, V3{th[0], th[1], th[2]});
      store3(out.est + 12 * row + 6, ok, omh);
    }
    store3(ws.xhat + 13 * b, ok, V3{th[0], th[1], th[2]});
    store3(ws.xhat + 13 * b + 6, ok, omh);
    ws.xhat[13 * b + 12] = xb[12];
    if (out.nis) out.nis[row] = (TIO)(ok ? nis : nan);
#pragma unroll
    for (int c = 0; c < 4; ++c) sb[c] = ok ? qh[c] : nan;
    sb[EST_LIVE] = ok ? 1.0 : nan;
  }
}

// Predict of tick `it`: i = 4 b + lane.  u is the applied forces of the tick, [B,12] (the slip rule's side buffer).
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_observe_predict_kernel(const TIO* __restrict__ x, const int32_t* __restrict__ tick, const TIO* __restrict__ u, const PlantIn<TIO> pin,
                             const ObsIn<TIO> in, const EstPar par, double* state, const ObsWs<TIO> ws, const ObsOut<TIO> out,
                             const int64_t B, const int T, const int it) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;
  const int64_t b = i / 4, row = b * T + it;
  const int l = (int)(i % 4), a = l < 3 ? l : 2;
  const double nan = __builtin_nan("");
  // ---- the accelerometer: the plant's right-hand side under the applied forces and the push, as mpcqp_imu_log_kernel forms the row
  const TIO* xb = x + 13 * b;
  const V3 th = load3(xb), om = load3(xb + 6);
  double qt[4];
  plant_rotvec_to_quat(th.x, th.y, th.z, qt);
  const M3 Rw = est_rot(qt);
  bool fin = fin3(th) && fin3(om);
  double bd[7], Ii[6];
  plant_body_row(pin.body, pin.model, b, bd);
  const double Ib[6] = {bd[1], bd[2], bd[3], bd[4], bd[5], bd[6]};
  fin = fin && plant_inertia(bd[0], Ib, Ii);
  const TIO* f = u + 12 * b;
  const V3 f0 = load3(f), f1 = load3(f + 3), f2 = load3(f + 6), f3 = load3(f + 9);
  V3 Fs = est_add(est_add(f0, f1), est_add(f2, f3));
  fin = fin && fin3(f0) && fin3(f1) && fin3(f2) && fin3(f3);
  const int tk = tick[b];
  if (pin.push && pin.push_ticks[2 * b] <= tk && tk < pin.push_ticks[2 * b + 1]) {
    const V3 Fp = load3(pin.push + 6 * b);
    Fs = est_add(Fs, Fp);
    fin = fin && fin3(Fp);
  }
  const V3 aw3 = {Fs.x / bd[0], Fs.y / bd[0], Fs.z / bd[0] + par.g};
  const V3 sp = {aw3.x, aw3.y, aw3.z - par.g};
  V3 acc = est_mtv(Rw, sp);
  if (in.bias) {
    const V3 bg = load3(in.bias + 6 * b), ba = load3(in.bias + 6 * b + 3);
    acc = est_add(acc, ba);
    fin = fin && fin3(bg) && fin3(ba);
  }
  if (in.noise) {
    const V3 ng = load3(in.noise + 6 * row), na = load3(in.noise + 6 * row + 3);
    acc = est_add(acc, na);
    fin = fin && fin3(ng) && fin3(na);
  }
  const TIO* s = ws.sense + OBS_SENSE * b;
  const V3 gy = {fin ? (double)s[0] : nan, fin ? (double)s[1] : nan, fin ? (double)s[2] : nan};
  const V3 sf = {fin ? obs_io<TIO>(acc.x) : nan, fin ? obs_io<TIO>(acc.y) : nan, fin ? obs_io<TIO>(acc.z) : nan};
  const double tr[4] = {(double)s[3], (double)s[4], (double)s[5], (double)s[6]};
  if (l == 3 && out.imu) {
    store3(out.imu + 6 * row, true, gy);
    store3(out.imu + 6 * row + 3, true, sf);
  }
  // ---- step 4 of the filter's row on the posterior the update left in est_state
  double* const sb = state + b * EST_STATE;
  double qh[4], xi[6], U[21];
  bool mine = isfinite(sb[EST_LIVE]) && fin3(gy) && fin3(sf);
#pragma unroll
  for (int c = 0; c < 4; ++c) { qh[c] = sb[c]; mine = mine && isfinite(qh[c]); }
#pragma unroll
  for (int c = 0; c < 6; ++c) { xi[c] = sb[EST_XI + 6 * a + c]; mine = mine && isfinite(xi[c]); }
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) { U[est_ut(r, c)] = sb[EST_P + 36 * a + 6 * r + c]; mine = mine && isfinite(U[est_ut(r, c)]); }
  float bad = mine ? 0.0f : 1.0f;
  bad = bad + dpp_mov<0xB1>(bad);
  bad = bad + dpp_mov<0x4E>(bad);
  const bool ok = bad == 0.0f;
  const M3 R = est_rot(qh);
  const double aw = ((est_pick(a, R.r0.x, R.r1.x, R.r2.x) * sf.x + est_pick(a, R.r0.y, R.r1.y, R.r2.y) * sf.y) +
                     est_pick(a, R.r0.z, R.r1.z, R.r2.z) * sf.z) + (a == 2 ? par.g : 0.0);
  xi[0] = (xi[0] + par.d * xi[1]) + par.hd2 * aw;
  xi[1] = xi[1] + par.d * aw;
  U[est_ut(0, 0)] = (U[est_ut(0, 0)] + par.d * U[est_ut(0, 1)]) + par.d * (U[est_ut(0, 1)] + par.d * U[est_ut(1, 1)]);
#pragma unroll
  for (int j = 1; j < 6; ++j) U[est_ut(0, j)] = U[est_ut(0, j)] + par.d * U[est_ut(1, j)];
  U[est_ut(0, 0)] = U[est_ut(0, 0)] + par.d * par.qp;
  U[est_ut(1, 1)] = U[est_ut(1, 1)] + par.d * par.qv;
#pragma unroll
  for (int j = 0; j < 4; ++j) U[est_ut(2 + j, 2 + j)] = U[est_ut(2 + j, 2 + j)] + par.d * (par.qf * (1.0 + (1.0 - tr[j]) * par.ks));
  const double sn = est_norm(sf), ga = fabs(par.g);
  const bool pull = sn > 0.0;
  const V3 sh = {pull ? sf.x / sn : 0.0, pull ? sf.y / sn : 0.0, pull ? sf.z / sn : 0.0};
  const double c0 = 1.0 - fabs(sn - ga) / ga;
  const double kap = pull ? par.kappa * (c0 < 0.0 ? 0.0 : (c0 > 1.0 ? 1.0 : c0)) : 0.0;
  const V3 cr = est_cross(sh, R.r2);
  const V3 wh = est_mv(R, V3{gy.x + kap * cr.x, gy.y + kap * cr.y, gy.z + kap * cr.z});
  double dq[4];
  plant_rotvec_to_quat(par.d * wh.x, par.d * wh.y, par.d * wh.z, dq);
  const double n0 = ((dq[0] * qh[0] - dq[1] * qh[1]) - dq[2] * qh[2]) - dq[3] * qh[3];
  const double n1 = ((dq[0] * qh[1] + dq[1] * qh[0]) + dq[2] * qh[3]) - dq[3] * qh[2];
  const double n2 = ((dq[0] * qh[2] - dq[1] * qh[3]) + dq[2] * qh[0]) + dq[3] * qh[1];
  const double n3 = ((dq[0] * qh[3] + dq[1] * qh[2]) - dq[2] * qh[1]) + dq[3] * qh[0];
  const double nq = sqrt(((n0 * n0 + n1 * n1) + n2 * n2) + n3 * n3);
  if (!ok) obs_nan_row(out, row, l);   // (a row whose accelerometer is not finite: mpcqp_estimate_track's outputs of that row are NaN)
  if (l < 3) {
#pragma unroll
    for (int c = 0; c < 6; ++c) sb[EST_XI + 6 * a + c] = ok ? xi[c] : nan;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) sb[EST_P + 36 * a + 6 * r + c] = ok ? U[est_sym(r, c)] : nan;
  } else {
    sb[0] = ok ? n0 / nq : nan; sb[1] = ok ? n1 / nq : nan; sb[2] = ok ? n2 / nq : nan; sb[3] = ok ? n3 / nq : nan;
    sb[EST_LIVE] = ok ? 1.0 : nan;
  }
}

}  // namespace
