// mpcqp_score.h -- the score row of a roll-out's logs (the C-ABI is mpcqp_rollout_score in include/mpcqp_sim.h, which has the fields and
// the rules; the entry point lives in mpcqp_kernels.hip).  One kernel, an HBM-bound reduction over [B,T] log rows into fp64 [B,33].
//
// Layout: ONE WAVE PER ROBOT, four robots per block of 256.  Lane l takes the ticks t = l, l + 64, ... of its robot in that order and
// keeps every sum and maximum in an fp64 register of its own; a lane without a tick contributes the exact identities (0 for sums and
// maxima, "no row" for fall_row).  The counts are wave-uniform from the start: every condition is a ballot over the wave and a population
// count, added up in scalar registers.  Then every sum and maximum goes through one fixed reduction over the wave (score_wave below: a
// DPP butterfly inside each row of 16 lanes, the four row results through v_readlane as (r0 + r1) + (r2 + r3); add, max, and min for
// fall_row), and lane 0 combines the row with the one already in `score` (accumulate) and writes it with plain stores.  No atomics, no LDS, no narrower groups for small T: a robot's row is a function of its own T rows
// alone -- not of B, of its slot in the batch or of the launch geometry.
//
// Loads: a log row is 12 (or 4) values of the I/O type, 16-byte aligned (the entry point checks the bases), read as float4 / double2; a
// lane's rows are 48 / 96 bytes apart, so the wave's three (six) load instructions per log together cover one contiguous span of the
// robot's rows.  The u8 rows are read as one dword.
//
// Arithmetic: fp64, without contraction, every row term summed in the one order written here -- so that score.score_host, which
// writes the same expressions in numpy, forms every term with the same bits and differs only in the order of the sum over t.
#pragma once
#include <cstdint>
#include "mpcqp_device.h"   // dpp_mov

namespace {

// The fields, in the order of MPCQP_SCORE_* (include/mpcqp_sim.h).
enum ScoreField : int {
  SC_ROWS, SC_BAD_ROWS, SC_FALL_ROW, SC_Z_SQ, SC_Z_MAX, SC_VEL_SQ, SC_VEL_MAX, SC_ANG_SQ, SC_ANG_MAX, SC_TILT_MAX, SC_VX_SUM, SC_VY_SUM,
  SC_FZ_MAX, SC_FRIC_MAX, SC_F_SQ, SC_STANCE_ROWS, SC_FLIGHT_ROWS = SC_STANCE_ROWS + 4,
  SC_TAU_MAX, SC_TAU_SQ, SC_WORK_POS, SC_WORK_ABS, SC_SWING_ROWS, SC_CLAMP_ROWS, SC_QLIM_ROWS, SC_RATE_ROWS, SC_SINGULAR_ROWS, SC_POISONED_ROWS,
  SC_LANDINGS, SC_MISS_MAX, SC_MISS_SQ, SCORE_FIELDS
};
static_assert(SCORE_FIELDS == MPCQP_SCORE_FIELDS, "the score row of include/mpcqp_sim.h");

// Which fields combine by max; fall_row combines by "the first"; every other field by +.
constexpr uint64_t SCORE_MAX_FIELDS = (1ull << SC_Z_MAX) | (1ull << SC_VEL_MAX) | (1ull << SC_ANG_MAX) | (1ull << SC_TILT_MAX) | (1ull << SC_FZ_MAX) |
                                      (1ull << SC_FRIC_MAX) | (1ull << SC_TAU_MAX) | (1ull << SC_MISS_MAX);
constexpr bool score_is_max(int f) { return (SCORE_MAX_FIELDS >> f) & 1; }
// Which fields count rows or leg-rows: the wave keeps them as integers (c[] of score_row), the score row holds them as doubles.
constexpr uint64_t SCORE_COUNT_FIELDS = (1ull << SC_ROWS) | (1ull << SC_BAD_ROWS) | (0xfull << SC_STANCE_ROWS) | (1ull << SC_FLIGHT_ROWS) |
                                        (0x3full << SC_SWING_ROWS) | (1ull << SC_LANDINGS);
constexpr bool score_is_count(int f) { return (SCORE_COUNT_FIELDS >> f) & 1; }
constexpr int SCORE_NO_ROW = 0x7fffffff;

// The logs; tau, qd, flag (the leg group: all or none) and miss may be null.
template <typename TIO>
struct ScoreIn { const TIO *actual, *desired, *forces; const uint8_t* contact; const TIO *tau, *qd; const uint8_t* flag; const TIO* miss; };

// n values (12 or 4) of a 16-byte aligned log row, as the log holds them.
template <int n>
__device__ __forceinline__ void score_load(const float* __restrict__ p, float (&v)[n]) {
  const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
  for (int i = 0; i < n / 4; ++i) {
    const float4 w = q[i];
    v[4 * i] = w.x; v[4 * i + 1] = w.y; v[4 * i + 2] = w.z; v[4 * i + 3] = w.w;
  }
}
template <int n>
__device__ __forceinline__ void score_load(const double* __restrict__ p, double (&v)[n]) {
  const double2* q = reinterpret_cast<const double2*>(p);
#pragma unroll
  for (int i = 0; i < n / 2; ++i) {
    const double2 w = q[i];
    v[2 * i] = w.x; v[2 * i + 1] = w.y;
  }
}

// How many lanes of the wave say p: wave-uniform, so a count lives in scalar registers and needs no reduction.  Every lane of the wave
// must be active.
__device__ __forceinline__ uint64_t score_votes(const bool p) { return (uint64_t)__popcll(__ballot(p)); }

// One log row per lane into the lane's sums and maxima a[], the wave's counts c[] and the lane's first fallen or bad row `fall` (the
// row's index t in this piece).  The whole wave runs this together: a lane without a row (live = false) is handed a row that exists and
// contributes identities; a bad row and a poisoned leg-row are computed on and selected away term by term, as the host does.
template <typename TIO>
__device__ __forceinline__ void score_row(const ScoreIn<TIO>& in, const int64_t row, const int t, const bool live, const double z_frac,
                                          const double tilt_lim, double (&a)[SCORE_FIELDS], uint64_t (&c)[SCORE_FIELDS], int& fall) {
#pragma clang fp contract(off)
  TIO xa[12], xd[12], f[12];
  score_load<12>(in.actual + 12 * row, xa);
  score_load<12>(in.desired + 12 * row, xd);
  score_load<12>(in.forces + 12 * row, f);
  bool ok = live;   // a row that counts: there, and not a bad row
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && isfinite(xa[i]) && isfinite(xd[i]) && isfinite(f[i]);
  // ---- body
  c[SC_ROWS] += score_votes(ok);
  c[SC_BAD_ROWS] += score_votes(live && !ok);
  const double dz = (double)xa[5] - (double)xd[5];
  a[SC_Z_SQ] += ok ? dz * dz : 0.0;
  a[SC_Z_MAX] = fmax(a[SC_Z_MAX], ok ? fabs(dz) : 0.0);
  const double dvx = (double)xa[9] - (double)xd[9], dvy = (double)xa[10] - (double)xd[10];
  const double ev = dvx * dvx + dvy * dvy;
  a[SC_VEL_SQ] += ok ? ev : 0.0;
  a[SC_VEL_MAX] = fmax(a[SC_VEL_MAX], ok ? sqrt(ev) : 0.0);
  const double d0 = (double)xa[0] - (double)xd[0], d1 = (double)xa[1] - (double)xd[1], d2 = (double)xa[2] - (double)xd[2];
  const double ea = (d0 * d0 + d1 * d1) + d2 * d2;
  a[SC_ANG_SQ] += ok ? ea : 0.0;
  a[SC_ANG_MAX] = fmax(a[SC_ANG_MAX], ok ? sqrt(ea) : 0.0);
  const double tilt = sqrt((double)xa[0] * (double)xa[0] + (double)xa[1] * (double)xa[1]);
  a[SC_TILT_MAX] = fmax(a[SC_TILT_MAX], ok ? tilt : 0.0);
  a[SC_VX_SUM] += ok ? (double)xa[9] : 0.0;
  a[SC_VY_SUM] += ok ? (double)xa[10] : 0.0;
  const bool down = live && (!ok || (double)xa[5] < z_frac * (double)xd[5] || tilt > tilt_lim);   // a bad row, or a fallen one
  fall = down ? min(fall, t) : fall;
  // ---- forces, stance legs only
  const uint32_t cw = *reinterpret_cast<const uint32_t*>(in.contact + 4 * row);
  double fs = 0.0;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const bool st = ok && ((cw >> (8 * l)) & 0xffu) != 0;
    const double fx = (double)f[3 * l], fy = (double)f[3 * l + 1], fz = (double)f[3 * l + 2];
    const double e = (fx * fx + fy * fy) + fz * fz;
    fs += st ? e : 0.0;
    c[SC_STANCE_ROWS + l] += score_votes(st);
    a[SC_FZ_MAX] = fmax(a[SC_FZ_MAX], st ? fz : 0.0);
    const bool up = st && fz > 0.0;   // (a leg that is not loaded has no friction use: it never divides)
    a[SC_FRIC_MAX] = fmax(a[SC_FRIC_MAX], up ? fmax(fabs(fx), fabs(fy)) / (up ? fz : 1.0) : 0.0);
  }
  a[SC_F_SQ] += fs;
  c[SC_FLIGHT_ROWS] += score_votes(ok && cw == 0);
  // ---- legs
  if (in.tau) {
    TIO tq[12], qd[12];
    score_load<12>(in.tau + 12 * row, tq);
    score_load<12>(in.qd + 12 * row, qd);
    const uint32_t fw = *reinterpret_cast<const uint32_t*>(in.flag + 4 * row);
    double ts = 0.0, wp = 0.0, wa = 0.0;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const uint32_t fl = (fw >> (8 * l)) & 0xffu;
      bool sound = fl != 0xffu;   // (a poisoned leg-row: the flag, or a non-finite entry, which the roll-outs write only under that flag)
#pragma unroll
      for (int j = 0; j < 3; ++j) sound = sound && isfinite(tq[3 * l + j]) && isfinite(qd[3 * l + j]);
      const bool on = ok && sound;
      const double t0 = (double)tq[3 * l], t1 = (double)tq[3 * l + 1], t2 = (double)tq[3 * l + 2];
      const double e = (t0 * t0 + t1 * t1) + t2 * t2;
      const double p = (t0 * (double)qd[3 * l] + t1 * (double)qd[3 * l + 1]) + t2 * (double)qd[3 * l + 2];
      ts += on ? e : 0.0;
      wp += on ? fmax(p, 0.0) : 0.0;
      wa += on ? fabs(p) : 0.0;
      a[SC_TAU_MAX] = fmax(a[SC_TAU_MAX], on ? fmax(fmax(fabs(t0), fabs(t1)), fabs(t2)) : 0.0);
      c[SC_SWING_ROWS] += score_votes(on && (fl & 1u));
      c[SC_CLAMP_ROWS] += score_votes(on && (fl & 2u));
      c[SC_QLIM_ROWS] += score_votes(on && (fl & 4u));
      c[SC_RATE_ROWS] += score_votes(on && (fl & 8u));
      c[SC_SINGULAR_ROWS] += score_votes(on && (fl & 16u));
      c[SC_POISONED_ROWS] += score_votes(ok && !sound);
    }
    a[SC_TAU_SQ] += ts;
    a[SC_WORK_POS] += wp;
    a[SC_WORK_ABS] += wa;
  }
  // ---- landing misses
  if (in.miss) {
    TIO m[4];
    score_load<4>(in.miss + 4 * row, m);
    double ms = 0.0;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const bool sound = ok && isfinite(m[l]);
      const double ml = (double)m[l];
      c[SC_LANDINGS] += score_votes(ok && m[l] != (TIO)0);   // (a NaN miss is a landing)
      ms += sound ? ml * ml : 0.0;
      a[SC_MISS_MAX] = fmax(a[SC_MISS_MAX], sound ? ml : 0.0);
    }
    a[SC_MISS_SQ] += ms;
  }
}

// One field over the 64 lanes of the wave, in one fixed order and without LDS: a butterfly inside each row of 16 (DPP: the two quad
// permutations, the half-row mirror, the row mirror), then the four row results through v_readlane as (r0 + r1) + (r2 + r3) (or the
// max).  Wave-uniform.  Every lane of the wave must be active.
template <bool MAX>
__device__ __forceinline__ double score_wave(double v) {
  const auto op = [](double x, double y) { return MAX ? fmax(x, y) : x + y; };
  v = op(v, dpp_mov<0xB1>(v));    // quad_perm [1,0,3,2]
  v = op(v, dpp_mov<0x4E>(v));    // quad_perm [2,3,0,1]
  v = op(v, dpp_mov<0x141>(v));   // row_half_mirror
  v = op(v, dpp_mov<0x140>(v));   // row_mirror
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const int lo = (int)(unsigned)u, hi = (int)(unsigned)(u >> 32);
  double r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    r[k] = __builtin_bit_cast(double, ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, 16 * k) << 32) |
                                          (unsigned)__builtin_amdgcn_readlane(lo, 16 * k));
  return op(op(r[0], r[1]), op(r[2], r[3]));
}
template <int CTRL>
__device__ __forceinline__ int score_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
// ... the first row: min.
__device__ __forceinline__ int score_wave_first(int v) {
  v = min(v, score_dpp<0xB1>(v)); v = min(v, score_dpp<0x4E>(v)); v = min(v, score_dpp<0x141>(v)); v = min(v, score_dpp<0x140>(v));
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

}  // namespace

// grid = ceil(B / 4) blocks of 256: wave w of block g scores robot 4 g + w.  T may be 0 (the identity row).
template <typename TIO>
__global__ __launch_bounds__(256) void mpcqp_score_kernel(const ScoreIn<TIO> in, const double z_frac, const double tilt_lim, const int accumulate,
                                                         double* __restrict__ score, const int B, const int T) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;   // (the whole wave)
  double a[SCORE_FIELDS];
  uint64_t c[SCORE_FIELDS];   // (wave-uniform)
#pragma unroll
  for (int i = 0; i < SCORE_FIELDS; ++i) { a[i] = 0.0; c[i] = 0u; }
  int fall = SCORE_NO_ROW;
  // the whole wave together: a lane past the last tick re-reads that tick and contributes nothing (t0 is 64-bit: T may be 2^31 - 1)
  for (int64_t t0 = 0; t0 < T; t0 += 64) {
    const int t = (int)min(t0 + lane, (int64_t)0x7fffffff);
    score_row(in, b * T + min(t, T - 1), t, t < T, z_frac, tilt_lim, a, c, fall);
  }
#pragma unroll
  for (int i = 0; i < SCORE_FIELDS; ++i)
    if (i != SC_FALL_ROW) a[i] = score_is_count(i) ? (double)c[i] : score_is_max(i) ? score_wave<true>(a[i]) : score_wave<false>(a[i]);
  fall = score_wave_first(fall);
  if (lane != 0) return;
  double* out = score + b * SCORE_FIELDS;
  double base = 0.0, first = -1.0;
  if (accumulate) {   // this piece's first row is row rows + bad_rows of the score carried in
    base = out[SC_ROWS] + out[SC_BAD_ROWS];
    first = out[SC_FALL_ROW];
#pragma unroll
    for (int i = 0; i < SCORE_FIELDS; ++i) {
      if (i == SC_FALL_ROW) continue;
      const double o = out[i];
      a[i] = score_is_max(i) ? fmax(o, a[i]) : o + a[i];
    }
  }
  a[SC_FALL_ROW] = first >= 0.0 ? first : (fall == SCORE_NO_ROW ? -1.0 : base + (double)fall);
#pragma unroll
  for (int i = 0; i < SCORE_FIELDS; ++i) out[i] = a[i];
}
