// mpcqp_estimate.h -- the torso state estimated from an IMU and leg kinematics (the C-ABI is include/mpcqp_estimate.h, which has the
// rule; the entry points live in mpcqp_kernels.hip): mpcqp_imu_log (what an IMU at the CoM reads on every row of a log) and
// mpcqp_estimate_track (orientation filter plus three 6-state Kalman filters over the rows) and, as a compile-time variant of its
// kernel, mpcqp_estimate_track_gated (include/mpcqp_gate.h: the trust of each leg gated on its velocity innovation before the updates),
// and as a second one mpcqp_estimate_track_aided (include/mpcqp_attitude.h: the velocity update's correction fed back into the
// orientation as a PI term whose integral is a gyro-bias state).
//
// The filter is serial in T and parallel in B.  Four lanes per robot, the mapping of the leg kernels: lane l does leg l's forward map,
// then lanes 0..2 own one axis each (xi[a] and the upper triangle of P[a], 6 + 21 doubles in registers) and take the four legs' rho,
// rhod components from their quad neighbours by DPP lane moves.  The orientation step is a few dozen flops on values every lane has,
// so every lane carries it and nothing is sent back; lane 3 runs the z axis a second time and stores the quaternion, the rotation
// vector, omega and nis.  Every lane of a quad runs the same instructions but for the height rows, which only the z lanes enter.
// No LDS, no scratch: the measurement order is unrolled, so every index into xi and P is a constant.
// Poison is a per-robot flag, combined over the quad once per row; outputs and the returned state are selects on it.
// The gate (est_gate) keeps the mapping: lanes 0 and 1 form the legs' normalised innovations along x and y from their own xi and P, two
// quad broadcasts per leg sum them in every lane, and every lane then holds the four gated trusts; lane 3 stores them.
// The aided rule (est_aid_*) keeps it too: every lane carries b^ (it needs g' = gyro - b^ for its leg), lanes 0 and 1 hold dv along x and
// y, two quad broadcasts give both to every lane, and every lane forms e_b and the orientation step; lane 3 stores b^, e_b and bias_log.
//
// One row of the filter is written once, as the helpers below, for this file's kernel over a log and for the two kernels of
// mpcqp_observe.h, which run the same row around a tick of the slip roll-out; that the three compute the same bits rests on that:
//   state      est_fresh / est_load / est_heights (each folds what it read into the lane's finite flag), est_quad_all, est_store
//   step 1     est_foot (a leg's rho and rhod), est_across (what a lane's axis sees of the four legs)
//   steps 1g-2 est_first_feet on a fresh start's first row; est_measure: est_gate, the four legs' scalar updates (est_leg, est_update), nis
//   step 3     est_out, est_sigma, est_rotvec: the values; each kernel stores them where it keeps them
//   step 4     est_predict
//   aided      est_aid_load, est_aid_sense (g'), est_aid_error (e_b from dv), est_aid_orient (inside est_predict: w^ and b^), est_aid_store
//   sensors    est_rotvec_rot, est_sense (R^T v + bias + noise), est_specific_force (applied forces over the body row)
#pragma once
#include "mpcqp_legsim.h"
#include "../../include/mpcqp_attitude.h"

namespace {

constexpr int EST_STATE = MPCQP_EST_STATE, EST_XI = 4, EST_P = 22, EST_LIVE = 130;

// MpcQpEstimator as the kernels take it (checked on the host, estimator_row in mpcqp_kernels.hip), with the handle's delta.
struct EstPar { double g, kappa, qp, qv, qf, rp, rv, rz, ks, p0p, p0v, p0f, d, hd2; };

// P[i][j], i <= j, of a symmetric 6 x 6 kept as its upper triangle by rows
__host__ __device__ constexpr int est_ut(const int i, const int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }
__host__ __device__ constexpr int est_sym(const int i, const int j) { return i <= j ? est_ut(i, j) : est_ut(j, i); }

// The small-vector arithmetic of the filter, not contracted (the V3 operators of mpcqp_legdyn.h are).
__device__ __forceinline__ V3 est_add(const V3 a, const V3 b) {
#pragma clang fp contract(off)
  return {a.x + b.x, a.y + b.y, a.z + b.z};
}
__device__ __forceinline__ V3 est_cross(const V3 a, const V3 b) {
#pragma clang fp contract(off)
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ V3 est_mv(const M3& A, const V3 v) {
#pragma clang fp contract(off)
  return {(A.r0.x * v.x + A.r0.y * v.y) + A.r0.z * v.z, (A.r1.x * v.x + A.r1.y * v.y) + A.r1.z * v.z, (A.r2.x * v.x + A.r2.y * v.y) + A.r2.z * v.z};
}
__device__ __forceinline__ V3 est_mtv(const M3& A, const V3 v) {   // A^T v
#pragma clang fp contract(off)
  return {(A.r0.x * v.x + A.r1.x * v.y) + A.r2.x * v.z, (A.r0.y * v.x + A.r1.y * v.y) + A.r2.y * v.z, (A.r0.z * v.x + A.r1.z * v.y) + A.r2.z * v.z};
}
__device__ __forceinline__ M3 est_rot(const double (&qt)[4]) {   // quat_rot's formula
#pragma clang fp contract(off)
  const double qw = qt[0], qx = qt[1], qy = qt[2], qz = qt[3];
  return {{1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)},
          {2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)},
          {2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)}};
}
__device__ __forceinline__ double est_norm(const V3 d) {
#pragma clang fp contract(off)
  return sqrt((d.x * d.x + d.y * d.y) + d.z * d.z);
}

template <int J>
__device__ __forceinline__ double quad_bcast(const double v) { return dpp_mov<J * 0x55>(v); }   // quad_perm [J,J,J,J]

// One scalar measurement z with variance r on an axis.  KIND 0: h = e_C - e_p, 1: h = e_v, 2: h = e_C.
template <int KIND, int C>
__device__ __forceinline__ void est_update(double (&xi)[6], double (&U)[21], const double z, const double r, double& nis) {
#pragma clang fp contract(off)
  double w[6], k[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) w[i] = KIND == 0 ? U[est_sym(i, C)] - U[est_sym(i, 0)] : (KIND == 1 ? U[est_sym(i, 1)] : U[est_sym(i, C)]);
  const double hw = KIND == 0 ? w[C] - w[0] : (KIND == 1 ? w[1] : w[C]);
  const double hx = KIND == 0 ? xi[C] - xi[0] : (KIND == 1 ? xi[1] : xi[C]);
  const double S = hw + r, e = z - hx;
#pragma unroll
  for (int i = 0; i < 6; ++i) { k[i] = w[i] / S; xi[i] = xi[i] + k[i] * e; }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) U[est_ut(i, j)] = U[est_ut(i, j)] - k[i] * w[j];
  nis = nis + (e * e) / S;
}

// The three measurements of leg J on an axis; `hgt` only where the lane owns z and height is given.
template <int J>
__device__ __forceinline__ void est_leg(const EstPar& par, double (&xi)[6], double (&U)[21], const double zr, const double zv, const double tr,
                                        const bool hgt, const double hz, double& nis) {
#pragma clang fp contract(off)
  const double s = 1.0 + (1.0 - tr) * par.ks;
  est_update<0, 2 + J>(xi, U, zr, par.rp * s, nis);
  est_update<1, 2 + J>(xi, U, -zv, par.rv * s, nis);
  if (hgt) est_update<2, 2 + J>(xi, U, hz, par.rz * s, nis);
}

__device__ __forceinline__ double est_pick(const int a, const double x, const double y, const double z) { return a == 0 ? x : (a == 1 ? y : z); }

// MpcQpTrustGate as the kernels take it (checked on the host, gate_row in mpcqp_kernels.hip): d_lo, d_hi, d_hi - d_lo.
struct EstGate { double lo, hi, span; };

// Step 1g of the row (include/mpcqp_gate.h): the four legs' trust c gated on the legs' velocity innovations along x and y against the
// predicted state, in place.  Lanes 0 and 1 own x and y and form the four m_la from their xi and U; lanes 2 and 3 run the same
// instructions on z and their values are not read.  Afterwards every lane of the quad holds the four w_l, as the I/O type holds them.
template <typename TIO>
__device__ __forceinline__ void est_gate(const EstGate& gate, const EstPar& par, const double (&xi)[6], const double (&U)[21],
                                         const double (&zv)[4], double (&tr)[4]) {
#pragma clang fp contract(off)
  const double S = U[est_ut(1, 1)] + par.rv;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double e = (-zv[j]) - xi[1];
    const double m = (e * e) / S;
    const double dl = quad_bcast<0>(m) + quad_bcast<1>(m);
    const double g = dl <= gate.lo ? 1.0 : (dl < gate.hi ? (gate.hi - dl) / gate.span : 0.0);
    tr[j] = (double)(TIO)(tr[j] * g);
  }
}

// MpcQpAttitude as the kernels take it (checked on the host, attitude_row in mpcqp_kernels.hip): k_s, k_v, k_b delta, b_max, delta |g|.
struct EstAid { double ks, kv, kbd, bmax, dg; };
constexpr int ATT_STATE = MPCQP_ATT_STATE;

// The aided rule (include/mpcqp_attitude.h).  b^ of a live robot from its att_state row (null or fresh: zero), folded into the lane's
// finite flag.
__device__ __forceinline__ V3 est_aid_load(const double* ab, const bool fresh, bool& fin) {
  if (!ab || fresh) return {0.0, 0.0, 0.0};
  const V3 bh = {ab[0], ab[1], ab[2]};
  fin = fin && fin3(bh);
  return bh;
}
// g' = gyro - b^
__device__ __forceinline__ V3 est_aid_sense(const V3 gy, const V3 bh) {
#pragma clang fp contract(off)
  return {gy.x - bh.x, gy.y - bh.y, gy.z - bh.z};
}
// e_b of the row from what step 2 did to this lane's velocity entry: lanes 0 and 1 own x and y, every lane gets both.
__device__ __forceinline__ V3 est_aid_error(const EstAid& aid, const M3& R, const double vpred, const double vpost) {
#pragma clang fp contract(off)
  const double dv = vpost - vpred;
  const double dx = quad_bcast<0>(dv), dy = quad_bcast<1>(dv);
  return est_mtv(R, V3{(-dy) / aid.dg, dx / aid.dg, 0.0});
}
// The body rate the orientation step integrates, before R: (g' + (k_s kap) (s^ x u)) + k_v e_b; and b^'s step, clamped.
__device__ __forceinline__ V3 est_aid_orient(const EstAid& aid, const V3 gp, const double kap, const V3 cr, const V3 eb, V3& bh) {
#pragma clang fp contract(off)
  const double kk = aid.ks * kap;
  const V3 w = {(gp.x + kk * cr.x) + aid.kv * eb.x, (gp.y + kk * cr.y) + aid.kv * eb.y, (gp.z + kk * cr.z) + aid.kv * eb.z};
  const double nx = bh.x - aid.kbd * eb.x, ny = bh.y - aid.kbd * eb.y, nz = bh.z - aid.kbd * eb.z;
  bh = {nx < -aid.bmax ? -aid.bmax : (nx > aid.bmax ? aid.bmax : nx), ny < -aid.bmax ? -aid.bmax : (ny > aid.bmax ? aid.bmax : ny),
        nz < -aid.bmax ? -aid.bmax : (nz > aid.bmax ? aid.bmax : nz)};
  return w;
}
// One lane stores the row: b^, e_b and the reserved pair; a poisoned robot's row is NaN.
__device__ __forceinline__ void est_aid_store(double* ab, const bool ok, const V3 bh, const V3 eb) {
  const double nan = __builtin_nan("");
  ab[0] = ok ? bh.x : nan; ab[1] = ok ? bh.y : nan; ab[2] = ok ? bh.z : nan;
  ab[3] = ok ? eb.x : nan; ab[4] = ok ? eb.y : nan; ab[5] = ok ? eb.z : nan;
  ab[6] = ok ? 0.0 : nan; ab[7] = ok ? 0.0 : nan;
}

// ---- the filter's state of lane axis a: qh, xi[a] and the upper triangle of P[a].  What is read folds into the lane's finite flag.

// A fresh start from a row that holds rotation vector, CoM and velocity at 0, 3 and 9 (a 12-wide init row, a 13-wide x row).
template <typename TIO>
__device__ __forceinline__ void est_fresh(const TIO* __restrict__ x0, const EstPar& par, const int a, double (&qh)[4], double (&xi)[6],
                                          double (&U)[21], bool& fin) {
#pragma unroll
  for (int c = 0; c < 3; ++c) fin = fin && isfinite((double)x0[c]) && isfinite((double)x0[3 + c]) && isfinite((double)x0[9 + c]);
  plant_rotvec_to_quat((double)x0[0], (double)x0[1], (double)x0[2], qh);
  xi[0] = (double)x0[3 + a]; xi[1] = (double)x0[9 + a];
#pragma unroll
  for (int c = 2; c < 6; ++c) xi[c] = 0.0;   // (the feet are set on the first row, from its rho: est_first_feet)
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) U[est_ut(r, c)] = r != c ? 0.0 : (r == 0 ? par.p0p : (r == 1 ? par.p0v : par.p0f));
}
__device__ __forceinline__ void est_load(const double* sb, const int a, double (&qh)[4], double (&xi)[6], double (&U)[21], bool& fin) {
  fin = fin && isfinite(sb[EST_LIVE]);
#pragma unroll
  for (int c = 0; c < 4; ++c) { qh[c] = sb[c]; fin = fin && isfinite(qh[c]); }
#pragma unroll
  for (int c = 0; c < 6; ++c) { xi[c] = sb[EST_XI + 6 * a + c]; fin = fin && isfinite(xi[c]); }
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) { U[est_ut(r, c)] = sb[EST_P + 36 * a + 6 * r + c]; fin = fin && isfinite(U[est_ut(r, c)]); }
}
// Lanes 0..2 store their axis a, lane 3 the quaternion and the live flag; a poisoned robot's state is NaN.
__device__ __forceinline__ void est_store(double* sb, const int l, const int a, const bool ok, const double (&qh)[4], const double (&xi)[6],
                                          const double (&U)[21]) {
  const double nan = __builtin_nan("");
  if (l < 3) {
    double* const xa = sb + EST_XI + 6 * a;
    double* const Pa = sb + EST_P + 36 * a;   // (the full 6 x 6 of the axis, where est_load reads the upper triangle)
#pragma unroll
    for (int c = 0; c < 6; ++c) xa[c] = ok ? xi[c] : nan;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) Pa[6 * r + c] = ok ? U[est_sym(r, c)] : nan;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) sb[c] = ok ? qh[c] : nan;
    sb[EST_LIVE] = ok ? 1.0 : nan;
  }
}
// The ground heights under robot b's four feet (height may be null: zeros, which are not read).
template <typename TIO>
__device__ __forceinline__ void est_heights(const TIO* __restrict__ height, const int64_t b, double (&hl)[4], bool& fin) {
#pragma unroll
  for (int j = 0; j < 4; ++j) hl[j] = 0.0;
  if (height) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { hl[j] = (double)height[4 * b + j]; fin = fin && isfinite(hl[j]); }
  }
}
// Whether all four lanes of the quad say `mine`: the robot's flag, the same in its four lanes.  (Call it where the whole quad runs.)
__device__ __forceinline__ bool est_quad_all(const bool mine) {
  float bad = mine ? 0.0f : 1.0f;
  bad = bad + dpp_mov<0xB1>(bad);
  bad = bad + dpp_mov<0x4E>(bad);
  return bad == 0.0f;
}

// ---- the row

// Step 1: the foot of the leg in geometry slot `slot` and its velocity, relative to the CoM, world axes, from the leg's q and qd.
__device__ __forceinline__ void est_foot(const LegGeoDev& geo, const int slot, const V3 q, const V3 qd, const M3& R, const V3 gy, V3& rho,
                                         V3& rhod) {
#pragma clang fp contract(off)
  const double ql[3] = {q.x, q.y, q.z};
  double pf[3], J[9];
  leg_fk_jac(geo, slot, ql, pf, J);
  const V3 pb = {pf[0], pf[1], pf[2]};
  const V3 jq = {(J[0] * qd.x + J[1] * qd.y) + J[2] * qd.z, (J[3] * qd.x + J[4] * qd.y) + J[5] * qd.z, (J[6] * qd.x + J[7] * qd.y) + J[8] * qd.z};
  rho = est_mv(R, pb); rhod = est_mv(R, est_add(est_cross(gy, pb), jq));
}
// ... and what lane axis a sees of a vector that lane j of the quad holds for leg j
__device__ __forceinline__ void est_across(const int a, const V3 v, double (&z)[4]) {
  z[0] = est_pick(a, quad_bcast<0>(v.x), quad_bcast<0>(v.y), quad_bcast<0>(v.z));
  z[1] = est_pick(a, quad_bcast<1>(v.x), quad_bcast<1>(v.y), quad_bcast<1>(v.z));
  z[2] = est_pick(a, quad_bcast<2>(v.x), quad_bcast<2>(v.y), quad_bcast<2>(v.z));
  z[3] = est_pick(a, quad_bcast<3>(v.x), quad_bcast<3>(v.y), quad_bcast<3>(v.z));
}

// The first row of a fresh start: the feet from the row's rho (est_fresh left them zero).
__device__ __forceinline__ void est_first_feet(const double (&zr)[4], double (&xi)[6]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 4; ++j) xi[2 + j] = xi[0] + zr[j];
}
// Steps 1g and 2: with GATE tr becomes w (else `gate` is not read), then the scalar updates of the four legs.  Returns the row's nis,
// the sum over the three axes.
template <typename TIO, bool GATE>
__device__ __forceinline__ double est_measure(const EstPar& par, const EstGate& gate, const bool hgt, const double (&hl)[4],
                                              const double (&zr)[4], const double (&zv)[4], double (&tr)[4], double (&xi)[6], double (&U)[21]) {
#pragma clang fp contract(off)
  if constexpr (GATE) est_gate<TIO>(gate, par, xi, U, zv, tr);
  double na = 0.0;
  est_leg<0>(par, xi, U, zr[0], zv[0], tr[0], hgt, hl[0], na);
  est_leg<1>(par, xi, U, zr[1], zv[1], tr[1], hgt, hl[1], na);
  est_leg<2>(par, xi, U, zr[2], zv[2], tr[2], hgt, hl[2], na);
  est_leg<3>(par, xi, U, zr[3], zv[3], tr[3], hgt, hl[3], na);
  return (quad_bcast<0>(na) + quad_bcast<1>(na)) + quad_bcast<2>(na);
}

// Step 3, what a row puts out after the updates: xi as it stands, the sigma of the axis' position (i = 0) or velocity (i = 1), the
// rotation vector of qh and omega = est_mv(R, gyro); est_out is a value as a log holds it, NaN for a poisoned robot (store3 takes ok).
template <typename TIO>
__device__ __forceinline__ TIO est_out(const bool ok, const double v) { return (TIO)(ok ? v : __builtin_nan("")); }
__device__ __forceinline__ double est_sigma(const double (&U)[21], const int i) { return sqrt(U[est_ut(i, i)]); }
__device__ __forceinline__ V3 est_rotvec(const double (&qh)[4]) {
  double th[3];
  plant_quat_to_rotvec(qh, th);
  return {th[0], th[1], th[2]};
}

// Step 4, the predict of lane axis a from the row's gyro, accelerometer and (gated) trust; R is est_rot(qh).  Leaves the normalised
// quaternion in qh.  AIDED: gy is g', the rate gets est_aid_orient's terms from the row's e_b, and bh is stepped; without it `aid`,
// `eb` and `bh`, the last three arguments, are not read.
template <bool AIDED = false>
__device__ __forceinline__ void est_predict(const EstPar& par, const int a, const M3& R, const V3 gy, const V3 sf, const double (&tr)[4],
                                            double (&qh)[4], double (&xi)[6], double (&U)[21], const EstAid& aid = EstAid{},
                                            const V3 eb = V3{0.0, 0.0, 0.0}, V3* bh = nullptr) {
#pragma clang fp contract(off)
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
  V3 wb;
  if constexpr (AIDED) wb = est_aid_orient(aid, gy, kap, cr, eb, *bh);
  else wb = V3{gy.x + kap * cr.x, gy.y + kap * cr.y, gy.z + kap * cr.z};
  const V3 wh = est_mv(R, wb);
  double dq[4];
  plant_rotvec_to_quat(par.d * wh.x, par.d * wh.y, par.d * wh.z, dq);
  const double n0 = ((dq[0] * qh[0] - dq[1] * qh[1]) - dq[2] * qh[2]) - dq[3] * qh[3];
  const double n1 = ((dq[0] * qh[1] + dq[1] * qh[0]) + dq[2] * qh[3]) - dq[3] * qh[2];
  const double n2 = ((dq[0] * qh[2] - dq[1] * qh[3]) + dq[2] * qh[0]) + dq[3] * qh[1];
  const double n3 = ((dq[0] * qh[3] + dq[1] * qh[2]) - dq[2] * qh[1]) + dq[3] * qh[0];
  const double nq = sqrt(((n0 * n0 + n1 * n1) + n2 * n2) + n3 * n3);
  qh[0] = n0 / nq; qh[1] = n1 / nq; qh[2] = n2 / nq; qh[3] = n3 / nq;
}

// ---- the sensor rows: what an IMU at the CoM of the true state reads

__device__ __forceinline__ M3 est_rotvec_rot(const V3 th) {
  double qt[4];
  plant_rotvec_to_quat(th.x, th.y, th.z, qt);
  return est_rot(qt);
}
// The body-frame readings of the world vectors wg (the gyro's) and wa (the accelerometer's): R^T w plus row b of bias and row `row` of
// noise (rows of [gyro 3, acc 3]; either may be null).  Both halves of a row given fold into fin, whichever reading the caller keeps.
template <typename TIO>
__device__ __forceinline__ void est_sense(const M3& R, const V3 wg, const V3 wa, const TIO* __restrict__ bias, const int64_t b,
                                          const TIO* __restrict__ noise, const int64_t row, bool& fin, V3& gyro, V3& acc) {
  gyro = est_mtv(R, wg); acc = est_mtv(R, wa);
  if (bias) {
    const V3 bg = load3(bias + 6 * b), ba = load3(bias + 6 * b + 3);
    gyro = est_add(gyro, bg); acc = est_add(acc, ba);
    fin = fin && fin3(bg) && fin3(ba);
  }
  if (noise) {
    const V3 ng = load3(noise + 6 * row), na = load3(noise + 6 * row + 3);
    gyro = est_add(gyro, ng); acc = est_add(acc, na);
    fin = fin && fin3(ng) && fin3(na);
  }
}
// The specific force, world axes, of the plant's right-hand side under the applied leg forces f [4,3] and, where `pushed`, the force of
// row b of push: the sum across the four legs in mpcqp_leg_effort's order, (0 + 1) + (2 + 3), over the mass of robot b's body row,
// through the acceleration the plant forms.  The body row's check and the operands fold into fin.
template <typename TIO>
__device__ __forceinline__ V3 est_specific_force(const TIO* __restrict__ f, const bool pushed, const TIO* __restrict__ push,
                                                 const TIO* __restrict__ body, const PlantModel& model, const int64_t b, const double g,
                                                 bool& fin) {
#pragma clang fp contract(off)
  double bd[7], Ii[6];
  plant_body_row(body, model, b, bd);
  const double Ib[6] = {bd[1], bd[2], bd[3], bd[4], bd[5], bd[6]};
  fin = fin && plant_inertia(bd[0], Ib, Ii);
  const V3 f0 = load3(f), f1 = load3(f + 3), f2 = load3(f + 6), f3 = load3(f + 9);
  V3 Fs = est_add(est_add(f0, f1), est_add(f2, f3));
  fin = fin && fin3(f0) && fin3(f1) && fin3(f2) && fin3(f3);
  if (pushed) {
    const V3 Fp = load3(push + 6 * b);
    Fs = est_add(Fs, Fp);
    fin = fin && fin3(Fp);
  }
  const V3 aw = {Fs.x / bd[0], Fs.y / bd[0], Fs.z / bd[0] + g};
  return {aw.x, aw.y, aw.z - g};
}

// mpcqp_estimate_track (GATE = false) and mpcqp_estimate_track_gated: i = 4 b + lane.  trust / height / state and each output may be
// null.  GATE adds step 1g and the trust_out rows (lane 3's); without it `gate` and `trust_out` are not read.  AIDED
// (mpcqp_estimate_track_aided) adds the rule of include/mpcqp_attitude.h, writes trust_out with or without GATE, and reads the last
// three arguments: the gains, att_state (may be null) and bias_log (may be null).
template <typename TIO, bool GATE, bool AIDED = false>
__global__ void __launch_bounds__(256)
mpcqp_estimate_track_kernel(const TIO* __restrict__ imu, const TIO* __restrict__ q, const TIO* __restrict__ qd,
                            const uint8_t* __restrict__ contact, const TIO* __restrict__ trust, const TIO* __restrict__ height,
                            const TIO* __restrict__ init, const EstPar par, const LegGeoDev geo, double* state, TIO* __restrict__ est,
                            TIO* __restrict__ feet_est, TIO* __restrict__ sigma, TIO* __restrict__ nis_out, const int64_t B, const int T,
                            const EstGate gate, TIO* __restrict__ trust_out, const EstAid aid = EstAid{}, double* att = nullptr,
                            TIO* __restrict__ bias_log = nullptr) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;   // (whole quads leave: the lane moves below see all four lanes or none)
  const int64_t b = i / 4;
  const int l = (int)(i % 4), a = l < 3 ? l : 2;
  double* const sb = state ? state + b * EST_STATE : nullptr;
  const bool fresh = !sb || sb[EST_LIVE] == 0.0;
  double qh[4], xi[6], U[21], hl[4];
  bool mine = true;   // this lane's operands are finite
  if (fresh) est_fresh(init + 12 * b, par, a, qh, xi, U, mine); else est_load(sb, a, qh, xi, U, mine);
  est_heights(height, b, hl, mine);
  double* ab = nullptr;
  V3 bh = {0.0, 0.0, 0.0}, eb = {0.0, 0.0, 0.0};
  if constexpr (AIDED) {
    ab = att ? att + b * ATT_STATE : nullptr;
    bh = est_aid_load(ab, fresh, mine);
  }
  const bool hgt = height != nullptr && a == 2;
  bool ok = true;   // the robot's flag
  for (int t = 0; t < T; ++t) {
    const int64_t row = b * T + t;
    const V3 gy = load3(imu + 6 * row), sf = load3(imu + 6 * row + 3);
    const V3 ql = load3(q + 3 * (4 * row + l)), qr = load3(qd + 3 * (4 * row + l));
    double tr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) tr[j] = trust ? (double)trust[4 * row + j] : (contact[4 * row + j] != 0 ? 1.0 : 0.0);
    mine = mine && fin3(gy) && fin3(sf) && fin3(qr) && fin3(ql) && isfinite(tr[0]) && isfinite(tr[1]) && isfinite(tr[2]) && isfinite(tr[3]);
    const bool row_ok = est_quad_all(mine);
    ok = ok && row_ok;
    // 1, 1g, 2
    const M3 R = est_rot(qh);
    V3 rho, rhod, gp = gy;
    double zr[4], zv[4];
    if constexpr (AIDED) gp = est_aid_sense(gy, bh);
    est_foot(geo, l, ql, qr, R, gp, rho, rhod);
    est_across(a, rho, zr); est_across(a, rhod, zv);
    if (fresh && t == 0) est_first_feet(zr, xi);
    const double vpred = xi[1];
    const double nis = est_measure<TIO, GATE>(par, gate, hgt, hl, zr, zv, tr, xi, U);
    if constexpr (AIDED) eb = est_aid_error(aid, R, vpred, xi[1]);
    // 3. outputs: lanes 0..2 their axis, lane 3 the orientation's
    const V3 om = est_mv(R, gp);
    if (l < 3) {
      if (est) { est[12 * row + 3 + a] = est_out<TIO>(ok, xi[0]); est[12 * row + 9 + a] = est_out<TIO>(ok, xi[1]); }
      if (feet_est) {
#pragma unroll
        for (int j = 0; j < 4; ++j) feet_est[3 * (4 * row + j) + a] = est_out<TIO>(ok, xi[2 + j]);
      }
      if (sigma) { sigma[6 * row + a] = est_out<TIO>(ok, est_sigma(U, 0)); sigma[6 * row + 3 + a] = est_out<TIO>(ok, est_sigma(U, 1)); }
    } else {
      if (est) {
        store3(est + 12 * row, ok, est_rotvec(qh));
        store3(est + 12 * row + 6, ok, om);
      }
      if (nis_out) nis_out[row] = est_out<TIO>(ok, nis);
      if constexpr (GATE || AIDED) {
        if (trust_out) {
#pragma unroll
          for (int j = 0; j < 4; ++j) trust_out[4 * row + j] = est_out<TIO>(ok, tr[j]);
        }
      }
      if constexpr (AIDED) {
        if (bias_log) store3(bias_log + 3 * row, ok, bh);
      }
    }
    // 4
    if constexpr (AIDED) est_predict<true>(par, a, R, gp, sf, tr, qh, xi, U, aid, eb, &bh);
    else est_predict(par, a, R, gy, sf, tr, qh, xi, U);
  }
  if (sb) est_store(sb, l, a, ok, qh, xi, U);
  if constexpr (AIDED) {
    if (ab && l == 3) est_aid_store(ab, ok, bh, eb);
  }
}

// mpcqp_imu_log: one lane per row of the log.  base_acc / body / bias / noise may be null.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_imu_log_kernel(const TIO* __restrict__ actual, const TIO* __restrict__ forces, const TIO* __restrict__ base_acc,
                     const TIO* __restrict__ body, const TIO* __restrict__ bias, const TIO* __restrict__ noise, const PlantModel model,
                     const double g, TIO* __restrict__ imu, const int64_t rows, const int64_t T) {
#pragma clang fp contract(off)
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const int64_t b = row / T;
  const V3 th = load3(actual + 12 * row), om = load3(actual + 12 * row + 6);
  const M3 R = est_rotvec_rot(th);
  bool fin = fin3(th) && fin3(om);
  V3 sp;
  if (base_acc) {
    const V3 al = load3(base_acc + 6 * row), aw = load3(base_acc + 6 * row + 3);
    fin = fin && fin3(al) && fin3(aw);
    sp = {aw.x, aw.y, aw.z - g};
  } else {   // the unpushed plant's right-hand side
    sp = est_specific_force(forces + 12 * row, false, (const TIO*)nullptr, body, model, b, g, fin);
  }
  V3 gyro, acc;
  est_sense(R, om, sp, bias, b, noise, row, fin, gyro, acc);
  store3(imu + 6 * row, fin, gyro);
  store3(imu + 6 * row + 3, fin, acc);
}

}  // namespace
