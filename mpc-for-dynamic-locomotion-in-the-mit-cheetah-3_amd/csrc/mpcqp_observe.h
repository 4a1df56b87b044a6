// mpcqp_observe.h -- sensors and the state estimator inside the slip roll-out's tick loop (the C-ABI is include/mpcqp_observe.h, which
// has the rule; the entry point lives in mpcqp_kernels.hip).  Two kernels around the unchanged kernels of mpcqp_rollout_slip:
//   mpcqp_observe_update_kernel    before the expand: the tick's encoder and gyro rows from the live buffers, then steps 1-3 of
//                                  mpcqp_estimate_track's row on est_state -- the fresh start, the scalar updates, the outputs -- and the
//                                  state the controller may read, x^ [B,13] and f^eet [B,4,3], in a side buffer
//   mpcqp_observe_predict_kernel   after the slip rule, before the legs step: the accelerometer row from the applied forces, the imu log
//                                  row, and step 4 of the filter's row on est_state
// Four lanes per robot, the mapping of mpcqp_estimate_track_kernel: in the update lane l does leg l's encoder and forward map, in both
// kernels lanes 0..2 own one axis each (xi[a] and the upper triangle of P[a] in registers, every index a constant) and lane 3 the
// orientation's outputs; quad exchanges by DPP lane moves, no LDS, no scratch.  The filter's row and the sensor rows are not written
// here: both kernels call the helpers of mpcqp_estimate.h that mpcqp_estimate_track_kernel and mpcqp_imu_log_kernel call (the list is
// at the top of that file), and what is left in them is the operands, the calls in step order and the stores.  Between the two kernels
// the state passes through est_state in fp64, so the two halves of a row are the row of mpcqp_estimate_track_kernel bit for bit.  The
// encoder row is this file's: legroll_swing_row and leg_joints<true, true> with the operands and the order of mpcqp_legs_step_kernel.
// Poison is the state itself: a robot whose row is not finite gets a NaN state, and a NaN state poisons every later row.
// mpcqp_rollout_observe_gated (include/mpcqp_gate.h) launches the update kernel's GATE variant: est_measure then runs est_gate between
// steps 1 and 2, and the gated trust goes where the update leaves "the trust of step 1" for the predict kernel; the predict kernel,
// the side buffers and the launch count are the ungated call's.
// mpcqp_rollout_observe_aided (include/mpcqp_attitude.h) launches the AIDED variants of both: the update reads b^ from att_state, runs the
// row with g' = gyro - b^ and stores e_b there; the predict reads b^ and e_b back, forms g' from the raw gyro of the sensor row again,
// and steps the orientation and b^ with est_predict<true>.  Nothing else passes between the two, and the side buffers are unchanged.
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
// velocity.  (Contracted like the legs step: not part of the filter's arithmetic.)
template <typename TIO>
__device__ __forceinline__ void obs_encoders(const TIO* __restrict__ xb, const TIO* __restrict__ rf, const PhaseRows<TIO>& ph, const int64_t b,
                                             const int l, const GaitLeg& gc, const int phi, const double* __restrict__ slip2,
                                             const double* __restrict__ leg7, const double hh, const double d, const LegGeoDev& geo, V3& qe,
                                             V3& qde) {
  // The leg's own geometry rows in slot 0, as mpcqp_legs_step_kernel hands them to leg_joints: the inverse map is contracted, and this
  // is the form in which its fused multiply-adds are known to come out as that kernel's.  The filter's forward map (est_foot) needs no
  // such copy: it takes geo and the leg, like mpcqp_estimate_track_kernel.
  LegGeoDev gl = geo;
#pragma unroll
  for (int c = 0; c < 3; ++c) { gl.hx[0][c] = geo.hx[l][c]; gl.hy[0][c] = geo.hy[l][c]; }
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
// null) gets the row's w; without it `gate` and `trust_log` are not read.  AIDED (mpcqp_rollout_observe_aided) adds items 1 to 4 of
// include/mpcqp_attitude.h's rule, writes trust_log with or without GATE, and reads the last two arguments: att_state and bias_log (may
// be null).
template <typename TIO, bool GATE, bool AIDED = false>
__global__ void __launch_bounds__(256)
mpcqp_observe_update_kernel(const TIO* __restrict__ x, const TIO* __restrict__ ref, const PhaseRows<TIO> ph, const int32_t* __restrict__ tick,
                            const double* __restrict__ slip, const double* __restrict__ legs, const TIO* __restrict__ step_height,
                            const ObsIn<TIO> in, const EstPar par, const LegGeoDev geo, double* state, const ObsWs<TIO> ws,
                            const ObsOut<TIO> out, const double d, const int64_t B, const int T, const int it, const EstGate gate,
                            TIO* __restrict__ trust_log, const EstAid aid = EstAid{}, double* att = nullptr,
                            TIO* __restrict__ bias_log = nullptr) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;   // (whole quads leave: the lane moves below see all four lanes or none)
  const int l = (int)(i % 4), a = l < 3 ? l : 2;
  const int64_t b = i / 4, row = b * T + it, il = 4 * row + l;
  const double nan = __builtin_nan("");
  const TIO* xb = x + 13 * b;
  // ---- the encoders of leg l
  const GaitLeg gc = gait_leg(ph.gait + b * GAIT_ROW, l);
  const int phi = gait_phase(gc, (uint32_t)max(tick[b], 0));
  const bool stance = phi < gc.st;
  V3 qe, qde;
  obs_encoders(xb, ref + 10 * b, ph, b, l, gc, phi, slip + 2 * i, legs + 7 * i, (double)step_height[b], d, geo, qe, qde);
  if (in.enc_noise) {
    const V3 nq = load3(in.enc_noise + 6 * il), nd = load3(in.enc_noise + 6 * il + 3);
    qe = est_add(qe, nq); qde = est_add(qde, nd);
  }
  qe = {obs_io<TIO>(qe.x), obs_io<TIO>(qe.y), obs_io<TIO>(qe.z)};
  qde = {obs_io<TIO>(qde.x), obs_io<TIO>(qde.y), obs_io<TIO>(qde.z)};
  if (out.q_enc) store3(out.q_enc + 3 * il, true, qe);
  if (out.qd_enc) store3(out.qd_enc + 3 * il, true, qde);
  // ---- the gyro, mpcqp_imu_log_kernel's, as the I/O type holds it, and the trust from the clock
  const V3 th = load3(xb), om = load3(xb + 6);
  bool fin = fin3(th) && fin3(om);
  V3 gy, later;   // (the accelerometer's half of the row is the predict kernel's, once the tick's forces are known)
  est_sense(est_rotvec_rot(th), om, V3{0.0, 0.0, 0.0}, in.bias, b, in.noise, row, fin, gy, later);
  gy = {fin ? obs_io<TIO>(gy.x) : nan, fin ? obs_io<TIO>(gy.y) : nan, fin ? obs_io<TIO>(gy.z) : nan};
  const double tme = stance ? 1.0 : 0.0;
  double tr[4] = {quad_bcast<0>(tme), quad_bcast<1>(tme), quad_bcast<2>(tme), quad_bcast<3>(tme)};
  // ---- the filter state: a fresh start from est_init (null: the robot's x as stored), or est_state
  double* const sb = state + b * EST_STATE;
  const bool fresh = sb[EST_LIVE] == 0.0;
  double qh[4], xi[6], U[21], hl[4];
  bool mine = fin3(qe) && fin3(qde) && fin3(gy);   // this lane's operands are finite
  if (fresh) est_fresh(in.est_init ? in.est_init + 12 * b : xb, par, a, qh, xi, U, mine); else est_load(sb, a, qh, xi, U, mine);
  est_heights(in.height, b, hl, mine);
  const bool hgt = in.height != nullptr && a == 2;
  V3 bh = {0.0, 0.0, 0.0}, gp = gy;
  if constexpr (AIDED) {
    bh = est_aid_load(att + b * ATT_STATE, fresh, mine);
    gp = est_aid_sense(gy, bh);
  }
  const bool ok = est_quad_all(mine);   // the robot's flag
  // ---- steps 1, 1g and 2 of the row.  With GATE tr becomes w, which is what the predict reads back (a poisoned robot's predict does not
  //      use it: its state is NaN).
  const M3 R = est_rot(qh);
  V3 rho, rhod;
  double zr[4], zv[4];
  est_foot(geo, l, qe, qde, R, gp, rho, rhod);
  est_across(a, rho, zr); est_across(a, rhod, zv);
  if (fresh) est_first_feet(zr, xi);
  const double vpred = xi[1];
  const double nis = est_measure<TIO, GATE>(par, gate, hgt, hl, zr, zv, tr, xi, U);
  // ---- step 3: the log rows, the controller's side buffers, the sensor row for the predict, and the posterior
  const V3 omh = est_mv(R, gp);
  if (l < 3) {
    const TIO ep = est_out<TIO>(ok, xi[0]), ev = est_out<TIO>(ok, xi[1]);
    if (out.est) { out.est[12 * row + 3 + a] = ep; out.est[12 * row + 9 + a] = ev; }
    ws.xhat[13 * b + 3 + a] = ep; ws.xhat[13 * b + 9 + a] = ev;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const TIO ef = est_out<TIO>(ok, xi[2 + j]);
      if (out.feet_est) out.feet_est[3 * (4 * row + j) + a] = ef;
      ws.feet[12 * b + 3 * j + a] = ef;
    }
    if (out.sigma) { out.sigma[6 * row + a] = est_out<TIO>(ok, est_sigma(U, 0)); out.sigma[6 * row + 3 + a] = est_out<TIO>(ok, est_sigma(U, 1)); }
  } else {
    const V3 th = est_rotvec(qh);
    if (out.est) {
      store3(out.est + 12 * row, ok, th);
      store3(out.est + 12 * row + 6, ok, omh);
    }
    store3(ws.xhat + 13 * b, ok, th);
    store3(ws.xhat + 13 * b + 6, ok, omh);
    ws.xhat[13 * b + 12] = xb[12];
    if (out.nis) out.nis[row] = est_out<TIO>(ok, nis);
    TIO* s = ws.sense + OBS_SENSE * b;
    store3(s, true, gy);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[3 + j] = (TIO)tr[j];
    if constexpr (GATE || AIDED) {
      if (trust_log) {
#pragma unroll
        for (int j = 0; j < 4; ++j) trust_log[4 * row + j] = est_out<TIO>(ok, tr[j]);
      }
    }
  }
  if constexpr (AIDED) {   // (every lane runs the broadcasts of est_aid_error; lane 3 stores)
    const V3 eb = est_aid_error(aid, R, vpred, xi[1]);
    if (l == 3) {
      if (bias_log) store3(bias_log + 3 * row, ok, bh);
      est_aid_store(att + b * ATT_STATE, ok, bh, eb);
    }
  }
  est_store(sb, l, a, ok, qh, xi, U);
}

// Predict of tick `it`: i = 4 b + lane.  u is the applied forces of the tick, [B,12] (the slip rule's side buffer).  AIDED reads the
// last three arguments: the gains, att_state (b^ and the e_b the update left) and bias_log (may be null; a poisoned row's is NaN).
template <typename TIO, bool AIDED = false>
__global__ void __launch_bounds__(256)
mpcqp_observe_predict_kernel(const TIO* __restrict__ x, const int32_t* __restrict__ tick, const TIO* __restrict__ u, const PlantIn<TIO> pin,
                             const ObsIn<TIO> in, const EstPar par, double* state, const ObsWs<TIO> ws, const ObsOut<TIO> out,
                             const int64_t B, const int T, const int it, const EstAid aid = EstAid{}, double* att = nullptr,
                             TIO* __restrict__ bias_log = nullptr) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;
  const int64_t b = i / 4, row = b * T + it;
  const int l = (int)(i % 4), a = l < 3 ? l : 2;
  const double nan = __builtin_nan("");
  // ---- the accelerometer: the plant's right-hand side under the applied forces and the push, as mpcqp_imu_log_kernel forms the row
  const TIO* xb = x + 13 * b;
  const V3 th = load3(xb), om = load3(xb + 6);
  bool fin = fin3(th) && fin3(om);
  const int tk = tick[b];
  const bool pushed = pin.push && pin.push_ticks[2 * b] <= tk && tk < pin.push_ticks[2 * b + 1];
  const V3 sp = est_specific_force(u + 12 * b, pushed, pin.push, pin.body, pin.model, b, par.g, fin);
  V3 made, acc;   // (the gyro's half of the row was made by the update kernel, which left it in ws.sense)
  est_sense(est_rotvec_rot(th), om, sp, in.bias, b, in.noise, row, fin, made, acc);
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
  bool mine = fin3(gy) && fin3(sf);
  est_load(sb, a, qh, xi, U, mine);
  if constexpr (AIDED) {
    double* const ab = att + b * ATT_STATE;
    V3 bh = {ab[0], ab[1], ab[2]};
    const V3 eb = {ab[3], ab[4], ab[5]};
    mine = mine && fin3(bh) && fin3(eb);
    const bool ok = est_quad_all(mine);
    est_predict<true>(par, a, est_rot(qh), est_aid_sense(gy, bh), sf, tr, qh, xi, U, aid, eb, &bh);
    if (!ok) obs_nan_row(out, row, l);
    if (l == 3) {
      if (!ok && bias_log) store3(bias_log + 3 * row, false, bh);
      est_aid_store(ab, ok, bh, eb);
    }
    est_store(sb, l, a, ok, qh, xi, U);
    return;
  }
  const bool ok = est_quad_all(mine);
  est_predict(par, a, est_rot(qh), gy, sf, tr, qh, xi, U);
  if (!ok) obs_nan_row(out, row, l);   // (a row whose accelerometer is not finite: mpcqp_estimate_track's outputs of that row are NaN)
  est_store(sb, l, a, ok, qh, xi, U);
}

}  // namespace
