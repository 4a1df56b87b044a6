// mpcqp_disturb.h -- per-robot disturbance wrench rows for the MPC and the wrench observer over a roll-out's logs (the C-ABI is
// include/mpcqp_disturb.h, which has the rule; the entry points live in mpcqp_kernels.hip): the conversion of the caller's table, the
// shift kernel that runs in front of a solve (xdes - s), the add-back kernel that runs behind it (X + s), and the observer.
//
// Shift and add-back are memory-bound passes over [B,N+1,13]: one lane per (robot, stage) row.  The lane forms the robot's two
// accelerations once -- a sine and a cosine of the yaw, a dozen fp64 multiplies -- and then moves its 13 elements; the 64 rows of a
// wave are one contiguous span of 64 x 13 elements, so every cache line a wave fetches is used in full by that wave (the same lines
// serve its 13 loads).  A lane per element coalesces each single load and pays the sine and cosine 13 times over: measured at twice the
// cost of the row form at 65 536 robots (+149 against +68 us per roll-out tick for the pair, profiles/r29_disturbance.txt).  What a lane
// reads besides -- the wrench row, the model row, x0[2] -- is the same address in the N + 1 lanes of a robot.
// The observer is serial in T and parallel in B: one lane per robot carries d^ and the previous row (39 doubles) in registers.
// No LDS, no scratch (every index is a constant after unrolling); masks and poison are selects.  Its row is written once, as a device
// function, for the pass over a log here and for the tick kernel of mpcqp_compensate.h.
#pragma once
#include "mpcqp_estimate.h"
#include "../../include/mpcqp_disturb.h"

namespace {

constexpr int DIST_ROW = 6, DIST_STATE = MPCQP_DIST_STATE, DIST_PREV = 6, DIST_LIVE = 39;

// What the shift rule takes from the configuration: the tick, theta (0 Euler, 1 / 2 zero-order hold), 1 / m and 1 / I of a robot
// without a model row.
struct DistCfg { double d, theta, inv_m, ib[3]; };

// One thread per row of the caller's table: a row with a non-finite entry becomes six NaNs.
__global__ void __launch_bounds__(256)
mpcqp_disturb_rows_kernel(const double* __restrict__ rows, double* __restrict__ table, const int64_t B) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double v[DIST_ROW];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < DIST_ROW; ++i) { v[i] = rows[b * DIST_ROW + i]; ok = ok && isfinite(v[i]); }
#pragma unroll
  for (int i = 0; i < DIST_ROW; ++i) table[b * DIST_ROW + i] = ok ? v[i] : __builtin_nan("");
}

// s[k] of robot b, the closed form of s[0] = 0, s[k+1] = Ad s[k] + Cd; false when the wrench row, the model row or the yaw is not
// finite (s is then not to be used).  `model`: the converted model table (1 / m, 1 / Ixx, 1 / Iyy, 1 / Izz, ...) or null.
template <typename TIO>
__device__ __forceinline__ bool dist_offset(const double* __restrict__ table, const double* __restrict__ model, const DistCfg& c,
                                            const TIO* __restrict__ x0, const int64_t b, const int k, double (&s)[13]) {
#pragma clang fp contract(off)
  double w[DIST_ROW], im = c.inv_m, ib[3] = {c.ib[0], c.ib[1], c.ib[2]};
#pragma unroll
  for (int i = 0; i < DIST_ROW; ++i) w[i] = table[b * DIST_ROW + i];
  if (model) {
    im = model[b * MODEL_ROW];
#pragma unroll
    for (int i = 0; i < 3; ++i) ib[i] = model[b * MODEL_ROW + 1 + i];
  }
  const double yaw = (double)x0[b * 13 + 2];
  bool fin = isfinite(yaw) && isfinite(im) && isfinite(ib[0]) && isfinite(ib[1]) && isfinite(ib[2]);
#pragma unroll
  for (int i = 0; i < DIST_ROW; ++i) fin = fin && isfinite(w[i]);
  const double cs = cos(yaw), sn = sin(yaw);
  // alpha = Rz diag(1 / I) Rz^T tau, a = F / m, and Rz alpha, which the orientation rows integrate (A[0:3,6:9] = Rz)
  const double tb[3] = {cs * w[3] + sn * w[4], cs * w[4] - sn * w[3], w[5]};
  const double wb[3] = {ib[0] * tb[0], ib[1] * tb[1], ib[2] * tb[2]};
  const double al[3] = {cs * wb[0] - sn * wb[1], sn * wb[0] + cs * wb[1], wb[2]};
  const double ra[3] = {cs * al[0] - sn * al[1], sn * al[0] + cs * al[1], al[2]};
  const double a[3] = {w[0] * im, w[1] * im, w[2] * im};
  const double kk = (double)k;
  const double c1 = kk * c.d, c2 = (c.d * c.d) * (0.5 * (kk * (kk - 1.0)) + c.theta * kk);
#pragma unroll
  for (int i = 0; i < 3; ++i) { s[i] = c2 * ra[i]; s[3 + i] = c2 * a[i]; s[6 + i] = c1 * al[i]; s[9 + i] = c1 * a[i]; }
  s[12] = 0.0;
  return fin;
}

// mpcqp_disturbance_shift and the hook in front of a solve: out = xdes - s, NaN for a robot that is not finite.  i = b (N + 1) + k.
// out may be xdes (each lane reads its row before it writes it).
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_disturb_shift_kernel(const double* __restrict__ table, const double* __restrict__ model, const DistCfg c, const TIO* __restrict__ x0,
                           const TIO* xdes, TIO* out, const int N1, const int64_t rows) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  double s[13], v[13];
  const bool fin = dist_offset(table, model, c, x0, i / N1, (int)(i % N1), s);
#pragma unroll
  for (int e = 0; e < 13; ++e) v[e] = (double)xdes[i * 13 + e];
#pragma unroll
  for (int e = 0; e < 13; ++e) out[i * 13 + e] = (TIO)(fin ? v[e] - s[e] : __builtin_nan(""));
}

// The same two passes with one lane per element, i = (b (N + 1) + k) 13 + e: every load and store of a wave is one contiguous span,
// and every lane pays the sine, the cosine and the whole of s for its one element.  Built only with -DMPCQP_DIST_LANE_PER_ELEMENT=1
// (`make dist_elem`), the variant tools/disturbance_rate.py measured the row form against (profiles/r29_disturbance.txt).
template <typename TIO, bool ADD>
__global__ void __launch_bounds__(256)
mpcqp_disturb_element_kernel(const double* __restrict__ table, const double* __restrict__ model, const DistCfg c, const TIO* __restrict__ x0,
                             const TIO* src, TIO* out, const int N1, const int64_t elems) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= elems) return;
  const int64_t row = i / 13;
  const int e = (int)(i % 13);
  double s[13];
  const bool fin = dist_offset(table, model, c, x0, row / N1, (int)(row % N1), s);
  double se = s[0];
#pragma unroll
  for (int j = 1; j < 13; ++j) se = e == j ? s[j] : se;
  const double v = (double)src[i];
  out[i] = (TIO)(ADD ? (fin ? v + se : v) : (fin ? v - se : __builtin_nan("")));
}

// The hook behind a solve: X += s; a robot that is not finite (its solve reported MPCQP_STATUS_NONFINITE) keeps what the solve wrote.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_disturb_addback_kernel(const double* __restrict__ table, const double* __restrict__ model, const DistCfg c, const TIO* __restrict__ x0,
                             TIO* __restrict__ X, const int N1, const int64_t rows) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  double s[13], v[13];
  const bool fin = dist_offset(table, model, c, x0, i / N1, (int)(i % N1), s);
#pragma unroll
  for (int e = 0; e < 13; ++e) v[e] = (double)X[i * 13 + e];
#pragma unroll
  for (int e = 0; e < 13; ++e) X[i * 13 + e] = (TIO)(fin ? v[e] + s[e] : v[e]);
}

// MpcQpWrenchObserver as the kernel takes it (checked on the host, observer_row in mpcqp_kernels.hip), with the handle's delta.
struct DistPar { double g, kappa, flim, tlim, d; };

__device__ __forceinline__ double dist_clamp(const double v, const double lim) { return v > lim ? lim : (v < -lim ? -lim : v); }

// The observer of one robot as a lane carries it: the robot's flag, d^ and the previous row.  dist_state_load / dist_state_store move it
// between the lane and the robot's 40 doubles of `state`, dist_observer_row is one row of the rule: mpcqp_disturb_track_kernel runs it over
// the T rows of a log, mpcqp_compensate_tick_kernel (mpcqp_compensate.h) once per tick of a roll-out.
struct DistLane { bool ok, live; double dh[6], Lp[3], vp[3], pp[3], fp[12], ftp[12]; };

// A fresh observer under the body row `ok` speaks for, then, where there is a state, the robot's.
__device__ __forceinline__ void dist_state_load(const double* sb, const bool ok, DistLane& s) {
  s.ok = ok;
  s.live = false;
#pragma unroll
  for (int i = 0; i < 6; ++i) s.dh[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) { s.Lp[i] = 0.0; s.vp[i] = 0.0; s.pp[i] = 0.0; }
#pragma unroll
  for (int i = 0; i < 12; ++i) { s.fp[i] = 0.0; s.ftp[i] = 0.0; }
  if (sb) {
#pragma unroll
    for (int i = 0; i < DIST_STATE; ++i) s.ok = s.ok && isfinite(sb[i]);
    s.live = sb[DIST_LIVE] != 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) s.dh[i] = sb[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { s.Lp[i] = sb[DIST_PREV + i]; s.vp[i] = sb[DIST_PREV + 3 + i]; s.pp[i] = sb[DIST_PREV + 6 + i]; }
#pragma unroll
    for (int i = 0; i < 12; ++i) { s.fp[i] = sb[DIST_PREV + 9 + i]; s.ftp[i] = sb[DIST_PREV + 21 + i]; }
  }
}

__device__ __forceinline__ void dist_state_store(double* sb, const DistLane& s) {
  const double nan = __builtin_nan("");
#pragma unroll
  for (int i = 0; i < 6; ++i) sb[i] = s.ok ? s.dh[i] : nan;
#pragma unroll
  for (int i = 0; i < 3; ++i) { sb[DIST_PREV + i] = s.ok ? s.Lp[i] : nan; sb[DIST_PREV + 3 + i] = s.ok ? s.vp[i] : nan; sb[DIST_PREV + 6 + i] = s.ok ? s.pp[i] : nan; }
#pragma unroll
  for (int i = 0; i < 12; ++i) { sb[DIST_PREV + 9 + i] = s.ok ? s.fp[i] : nan; sb[DIST_PREV + 21 + i] = s.ok ? s.ftp[i] : nan; }
  sb[DIST_LIVE] = s.ok ? (s.live ? 1.0 : 0.0) : nan;
}

// One row of the rule of include/mpcqp_disturb.h on the lane's observer: xr the torso row (12), fr the forces over the row's tick (12),
// ftr the feet (12), each as the I/O type holds it; m, Ib the body the observer believes.  Folds the row's operands into s.ok, leaves
// the residual in res and d^ in s.dh, and makes the row the previous one.  fp64, not contracted; masks and poison are selects.
template <typename TIO>
__device__ __forceinline__ void dist_observer_row(const TIO* __restrict__ xr, const TIO* __restrict__ fr, const TIO* __restrict__ ftr,
                                                  const double m, const double (&Ib)[6], const DistPar& par, DistLane& s, double (&res)[6]) {
#pragma clang fp contract(off)
  const V3 th = load3(xr), pc = load3(xr + 3), om = load3(xr + 6), vc = load3(xr + 9);
  double f[12], ft[12];
  bool fin = fin3(th) && fin3(pc) && fin3(om) && fin3(vc);
#pragma unroll
  for (int i = 0; i < 12; ++i) { f[i] = (double)fr[i]; fin = fin && isfinite(f[i]); }
#pragma unroll
  for (int l = 0; l < 4; ++l) {   // a leg without force is left out: its foot is not read, the state keeps a zero
    const bool on = f[3 * l] != 0.0 || f[3 * l + 1] != 0.0 || f[3 * l + 2] != 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double v = (double)ftr[3 * l + a];
      ft[3 * l + a] = on ? v : 0.0;
      fin = fin && isfinite(ft[3 * l + a]);
    }
  }
  s.ok = s.ok && fin;
  const M3 R = est_rotvec_rot(th);
  const V3 wb = est_mtv(R, om);
  const double wv[3] = {wb.x, wb.y, wb.z};
  double Lb[3];
  plant_symv(Ib, wv, Lb);
  const V3 Lw = est_mv(R, V3{Lb[0], Lb[1], Lb[2]});
  const double L[3] = {Lw.x, Lw.y, Lw.z}, v[3] = {vc.x, vc.y, vc.z}, p[3] = {pc.x, pc.y, pc.z};
  double Fs[3], Ms[3], cr[4][3];
  const double pm[3] = {0.5 * (s.pp[0] + p[0]), 0.5 * (s.pp[1] + p[1]), 0.5 * (s.pp[2] + p[2])};
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const bool on = s.fp[3 * l] != 0.0 || s.fp[3 * l + 1] != 0.0 || s.fp[3 * l + 2] != 0.0;
    const double r[3] = {s.ftp[3 * l] - pm[0], s.ftp[3 * l + 1] - pm[1], s.ftp[3 * l + 2] - pm[2]};
    const double fl[3] = {s.fp[3 * l], s.fp[3 * l + 1], s.fp[3 * l + 2]};
    double c3[3];
    plant_cross(r, fl, c3);
#pragma unroll
    for (int a = 0; a < 3; ++a) cr[l][a] = on ? c3[a] : 0.0;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    Fs[a] = (s.fp[a] + s.fp[3 + a]) + (s.fp[6 + a] + s.fp[9 + a]);
    Ms[a] = (cr[0][a] + cr[1][a]) + (cr[2][a] + cr[3][a]);
    const double rf = (m * (v[a] - s.vp[a])) / par.d - Fs[a];
    res[a] = s.live ? (a == 2 ? rf - m * par.g : rf) : 0.0;
    res[3 + a] = s.live ? (L[a] - s.Lp[a]) / par.d - Ms[a] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) s.dh[i] = s.live ? dist_clamp(s.dh[i] + par.kappa * (res[i] - s.dh[i]), i < 3 ? par.flim : par.tlim) : s.dh[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) { s.Lp[i] = L[i]; s.vp[i] = v[i]; s.pp[i] = p[i]; }
#pragma unroll
  for (int i = 0; i < 12; ++i) { s.fp[i] = f[i]; s.ftp[i] = ft[i]; }
  s.live = true;
}

// mpcqp_disturbance_track: lane b runs robot b over its T rows.  body / state / dist / resid may be null.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_disturb_track_kernel(const TIO* __restrict__ actual, const TIO* __restrict__ forces, const TIO* __restrict__ feet,
                           const TIO* __restrict__ body, const PlantModel model, const DistPar par, double* state, TIO* __restrict__ dist,
                           TIO* __restrict__ resid, const int64_t B, const int T) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double* const sb = state ? state + b * DIST_STATE : nullptr;
  double bd[7], Ii[6];
  plant_body_row(body, model, b, bd);
  const double Ib[6] = {bd[1], bd[2], bd[3], bd[4], bd[5], bd[6]};
  DistLane s;
  dist_state_load(sb, plant_inertia(bd[0], Ib, Ii), s);   // (the robot's flag starts from its body row)
  for (int t = 0; t < T; ++t) {
    const int64_t row = b * T + t;
    double res[6];
    dist_observer_row(actual + 12 * row, forces + 12 * row, feet + 12 * row, bd[0], Ib, par, s, res);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      if (dist) dist[6 * row + i] = est_out<TIO>(s.ok, s.dh[i]);
      if (resid) resid[6 * row + i] = est_out<TIO>(s.ok, res[i]);
    }
  }
  if (sb) dist_state_store(sb, s);
}

}  // namespace
