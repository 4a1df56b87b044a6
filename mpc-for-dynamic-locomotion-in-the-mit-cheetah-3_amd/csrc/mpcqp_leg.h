// mpcqp_leg.h -- what the two solve engines (mpcqp_wrench.h, mpcqp_stage.h) share: lane-level helpers, the data of one leg-stage as
// both engines hold it in registers (LegMapAdmm / LegMapPolish of mpcqp_legmap.h, LegAdmm, ActSet, LegAA), the Anderson step, and the parts of OSQP's iteration on the five
// rows  fz | fx - mu fz | fx + mu fz | fy - mu fz | fy + mu fz  (src/mpc.py:138-173) that both engines call as functions from register
// values to register values: residuals and rho ratio, right-hand side, projection.  No LDS, no sync, no engine type in here.
// What is NOT here: the functions that fill the leg's ADMM / polish systems (they fill the same types), the active-set rule, the warm start and the relaxation step exist once per engine
// (w_* / sg_*): through a common function every wrench kernel loses its assembly (profiles/r07_leg_share_check.txt).
#pragma once
#include "mpcqp_common.h"
#include "mpcqp_legmap.h"

namespace {

__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }
// A zero the optimiser cannot see through.  A 64-bit constant needs a register pair, LLVM hoists such pairs out of the persistent QP loop,
// and with the register file full it then SPILLS the constant at kernel entry and reloads it per QP (scratch stores are written through:
// 10 bytes per lane and wave of HBM writes for three zeros and a one, profiles/r03f_hbm_traffic.json).  Materialised where it is used instead.
__device__ __forceinline__ double opaque_zero_f64() {
  unsigned lo, hi;
  asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0" : "=v"(lo), "=v"(hi));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <typename T> __device__ __forceinline__ T opaque_zero() {
  if constexpr (sizeof(T) == 8) return (T)opaque_zero_f64();
  else { float z; asm volatile("v_mov_b32 %0, 0" : "=v"(z)); return (T)z; }
}
// A wave-uniform float, moved to a scalar register (loop-carried uniform values otherwise occupy a vector register each).
__device__ __forceinline__ float ufloat(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

template <int NW>
__device__ __forceinline__ void wsync() {
  if constexpr (NW == 1) {   // one wave: its LDS operations execute in order; only the compiler has to be told
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

template <int Q, int NW>
__device__ __forceinline__ void wmax(float (&v)[Q], float* red, int tid) {
  if constexpr (NW == 1) {
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = wave_max(v[q]);
  } else {
    block_max<Q, NW>(v, red, tid);
  }
}

template <int Q, int NW>
__device__ __forceinline__ void wsum(float (&v)[Q], float* red, int tid) {
  if constexpr (NW == 1) {
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = wave_sum(v[q]);
  } else {
    block_sum<Q, NW>(v, red, tid);
  }
}

template <typename T> __device__ __forceinline__ T quad_sum(T v) { v += dpp_mov<0xB1>(v); v += dpp_mov<0x4E>(v); return v; }

// Reduce-scatter of 8 values over the 8 lanes of a group: lane gc ends with the group total of element gc.
template <typename T>
__device__ __forceinline__ T rs8(const T (&v)[8], int gc) {
  const bool hi = (gc & 4) != 0, b1 = (gc & 2) != 0, b0 = (gc & 1) != 0;
  T t[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) { const T keep = hi ? v[4 + m] : v[m], send = hi ? v[m] : v[4 + m]; t[m] = keep + dpp_mov<0x141>(send); }
  T s2[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) { const T keep = b1 ? t[2 + m] : t[m], send = b1 ? t[m] : t[2 + m]; s2[m] = keep + dpp_mov<0x4E>(send); }
  const T keep = b0 ? s2[1] : s2[0], send = b0 ? s2[0] : s2[1];
  return keep + dpp_mov<0xB1>(send);
}

// The same reduce-scatter with the first step's keep / send selects done by the write mask of the DPP add (fp32; the 8 lanes of a
// group are the 8 consecutive lanes 8 gr + gc of a wave: one wave per QP at horizon 10).  In that step a lane with gc & 4 clear adds
// its own v[m] to its partner's v[m] (the partner, lane 7 - gc of the group, has the bit set and sends v[m]); a lane with the bit
// set does the same with v[4 + m].  The lanes with the bit clear are DPP banks 0 and 2 of every row of 16 (bank = 2 (gr & 1) +
// (gc >> 2)), so two adds into one destination -- `v[m] + v[m]'` under bank_mask 0x5, `v[4 + m] + v[4 + m]'` under 0xa, lanes outside
// the mask keep the destination -- give every lane the sum the select form gives it, with the operands swapped; an IEEE add commutes
// bit for bit (two NaNs of different payloads aside: tools/rs8_forms.hip compares the words of the two forms, tests/test_rs8_forms.py).
// Eight instructions for twelve, and the mask of bit 2 is never formed.  The later steps pair lanes inside a quad, where no bank mask
// separates them: they are rs8's.  (A write mask cannot be said through __builtin_amdgcn_update_dpp and an add -- the DPP combine
// folds full masks only -- hence the asm; its DPP sources may have been written by the instruction just before, which needs two
// wait states that the compiler does not count for an asm: the s_nop.  The destinations are written in full by the two adds and
// first read by a select, not by a DPP operand.)  fp64 keeps the selects: a masked 64-bit value is three moves per word.
// Preconditions of the block, which the hazard recognizer cannot check inside an asm and the caller has to keep (w_matvec in w_solve:
// "all lanes call", uniform control flow around it):  no VALU instruction writes EXEC within five wait states before it (a DPP
// instruction after a VALU write of EXEC needs them);  all 64 lanes are active -- without bound_ctrl a source lane that is switched
// off leaves its partner's destination unwritten, and the "=&v" destinations have no defined value to fall back to.
__device__ __forceinline__ float rs8_banked(const float (&v)[8], int gc) {
  const bool b1 = (gc & 2) != 0, b0 = (gc & 1) != 0;
  float t[4];
  asm("s_nop 1\n\t"
      "v_add_f32_dpp %0, %4, %4 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
      "v_add_f32_dpp %1, %5, %5 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
      "v_add_f32_dpp %2, %6, %6 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
      "v_add_f32_dpp %3, %7, %7 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
      "v_add_f32_dpp %0, %8, %8 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
      "v_add_f32_dpp %1, %9, %9 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
      "v_add_f32_dpp %2, %10, %10 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
      "v_add_f32_dpp %3, %11, %11 row_half_mirror row_mask:0xf bank_mask:0xa"
      : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3])
      : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]));
  float s2[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) { const float keep = b1 ? t[2 + m] : t[m], send = b1 ? t[m] : t[2 + m]; s2[m] = keep + dpp_mov<0x4E>(send); }
  const float keep = b0 ? s2[1] : s2[0], send = b0 ? s2[0] : s2[1];
  return keep + dpp_mov<0xB1>(send);
}

__device__ __forceinline__ float w_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ double w_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}

template <typename TM> __device__ __forceinline__ void ld8(const TM* p, TM (&o)[8]);
template <> __device__ __forceinline__ void ld8<float>(const float* p, float (&o)[8]) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
template <> __device__ __forceinline__ void ld8<double>(const double* p, double (&o)[8]) {
#pragma unroll
  for (int h = 0; h < 4; ++h) { const double2 a = reinterpret_cast<const double2*>(p)[h]; o[2 * h] = a.x; o[2 * h + 1] = a.y; }
}
template <typename TM> __device__ __forceinline__ void st8(TM* p, const TM (&o)[8]);
template <> __device__ __forceinline__ void st8<float>(float* p, const float (&o)[8]) {
  reinterpret_cast<float4*>(p)[0] = make_float4(o[0], o[1], o[2], o[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(o[4], o[5], o[6], o[7]);
}
template <> __device__ __forceinline__ void st8<double>(double* p, const double (&o)[8]) {
#pragma unroll
  for (int h = 0; h < 4; ++h) reinterpret_cast<double2*>(p)[h] = make_double2(o[2 * h], o[2 * h + 1]);
}

// Per-leg data of a linear solve with M = D + A-stack' K A-stack -- the 6 x 3 wrench map and the inverse diagonal -- is a LegMapAdmm
// or a LegMapPolish (mpcqp_legmap.h): both engines' *_sys functions build the same structured types.

// OSQP algorithm 1 on the rows  fz | fx - mu fz | fx + mu fz | fy - mu fz | fy + mu fz  of a leg-stage
// (src/mpc.py:138-173), one lane per leg-stage, scaled duals yh = y / rho.
template <typename TM>
struct LegAdmm {
  TM u[3], z[5], yh[5], g[3];
  TM lo0, hi0, loA, hiB;     // fz box; friction rows: A rows in [loA, 0], B rows in [0, hiB]
  TM mu;
};

// The active set of a leg-stage as the polish uses it: zs / xs / ys in {-1, 0, +1} (fz at fmin / free / at fmax; fx, fy tied
// to -mu fz / free / tied to +mu fz), packed as (zs + 1) | (xs + 1) << 2 | (ys + 1) << 4.
struct ActSet {
  int zs, xs, ys;
  bool ez, ex, ey;
  __device__ __forceinline__ ActSet(int code, bool stance) {
    zs = (code & 3) - 1; xs = ((code >> 2) & 3) - 1; ys = ((code >> 4) & 3) - 1;
    ez = stance && zs == 0; ex = stance && xs == 0; ey = stance && ys == 0;
  }
};

// ----------------------------------------------------------------------------------------------------- Anderson acceleration
// The ADMM block exists to find the active set, and on the QPs that end a launch (two-legged support at low friction) plain
// ADMM needs 300 - 400 iterations for it: the iteration is a contraction with a factor close to 1 along a few directions.
// Anderson acceleration (type II, memory AA_M) of the map  v -> f^p(v),  v = z + y / rho  the pre-projection variable of
// OSQP's iteration (z = clip(v), y / rho = v - z: the five rows of a leg-stage, five numbers per lane):  every p-th iterate is
// replaced by the combination of the last AA_M + 1 of them that minimises the fixed-point residual in the least-squares sense,
//     gam = argmin | r - dF gam |,   v+ = f(v) - dX gam,     dF / dX: differences of consecutive residuals / images
// -- nine inner products over the wave (seven DPP steps each), a regularised 3 x 3 solve in uniform registers, fifteen FMAs per
// lane, once per p iterations.  (Of the nine numbers the solve takes, the three Gram entries among the two older columns are the
// previous call's entries among its two newer ones -- the same lane products, summed in the same order.  CARRY = true, the MIXED
// horizon-10 kernels, keeps them in three words of LDS and sums six: bit-identical, tests/test_gpu_accel_identity.py on the device
// and tools/aa_carry_check.cpp on the host; 192 -> 153 VALU per call, kernel -1.5 %, profiles/r07_accel_carry.txt.  A restart of
// the history clears them with the columns.)  numpy study on the condensed QP (tools/accel_study.py): the hardest QPs of five batches reach a
// polishable iterate in half the iterations (worst case of a batch 375 -> 250 us of solve), the easy ones are unchanged.
// Only with the polish (MPCQP_FLAG_POLISH): an ADMM-only run is OSQP's algorithm 1 unchanged.  History in fp32 (it steers an
// extrapolation, it is not part of the answer); base point and images in the iteration's element type.
#ifndef MPCQP_AA_M
#define MPCQP_AA_M 3
#endif
constexpr int AA_M = MPCQP_AA_M;
constexpr int AA_NS = 2 * AA_M;                  // inner products summed per call: the newest column against every column, the right-hand sides
constexpr int AA_NC = AA_M * (AA_M - 1) / 2;   // Gram entries among the AA_M - 1 columns that survive a call: carried, not summed again
// The carried entries are uniform over the workgroup and live in LDS between calls, in the words of `red` (12 per wave) that follow
// the AA_NS partial sums of wave 0: held in scalar registers from call to call they cost the headline kernel four spilled vector
// registers (hipcc's resource report; in LDS: none).  Every thread stores the same values.
static_assert(AA_NS + AA_NC <= 12, "the carried Gram entries share wave 0's row of the partial sums");
// Position of dF_i . dF_j (i <= j) in the upper triangle of the Gram matrix, row by row (M = 3: 00 01 02 11 12 22).
constexpr int aa_gram_at(int i, int j) { return i * AA_M - i * (i - 1) / 2 + (j - i); }
struct LegAA {
  float rp[5];                       // previous residual f(v) - v
  float dX[AA_M][5], dF[AA_M][5];    // column AA_M - 1 is the newest
};

// Empty history; `red`: the partial-sum words w_aa_step is called with (the carried Gram entries of empty columns are zeros).
template <bool CARRY>
__device__ __forceinline__ void w_aa_reset(LegAA& h, float* __restrict__ red) {
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    h.rp[k] = 0.f;
#pragma unroll
    for (int j = 0; j < AA_M; ++j) { h.dX[j][k] = 0.f; h.dF[j][k] = 0.f; }
  }
#pragma unroll
  for (int c = 0; c < (CARRY ? AA_NC : 0); ++c) red[AA_NS + c] = 0.f;
}

// One extrapolation: fx = f^p(xb) has just been computed.  Files (fx, fx - xb) in the history and returns the next base point in
// xb (the extrapolated iterate, or fx itself while the history is empty / when the least-squares problem is degenerate -- then the
// history restarts).  `have_prev`: an earlier image exists (uniform).  Uniform control flow; ends with the caller's state untouched
// except xb / fp / h.  CARRY = false sums all the Gram entries in every call (horizon 20 and the stage-wise engine: there the
// carried form costs three to nine more spilled registers per kernel, hipcc's resource report).
template <typename TM, int NW, bool CARRY>
__device__ __forceinline__ void w_aa_step(LegAA& h, TM (&xb)[5], TM (&fp)[5], const TM (&fx)[5], bool& have_prev, const bool leg,
                                          float* __restrict__ red, const int tid) {
  static_assert(AA_M == 3 || AA_M == 2, "the solve below is written for two or three columns");
  constexpr int M = AA_M, NG = M * (M + 1) / 2, NQ_ = NG + M, NS = AA_NS, NC = CARRY ? AA_NC : 0;
  float r[5];
  if (!have_prev) {   // (uniform) the first image of a history: nothing to combine yet -- file it and go on from it
#pragma unroll
    for (int k = 0; k < 5; ++k) { h.rp[k] = leg ? (float)(fx[k] - xb[k]) : 0.f; fp[k] = fx[k]; xb[k] = fx[k]; }
    have_prev = true;
    return;
  }
  float gc[AA_NC];   // Gram entries of columns 0 .. M - 2 (upper triangle, row by row) as the last call left them
#pragma unroll
  for (int c = 0; c < NC; ++c) gc[c] = red[NS + c];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    r[k] = leg ? (float)(fx[k] - xb[k]) : 0.f;
    const float dx = have_prev ? (float)(fx[k] - fp[k]) : 0.f, df = have_prev ? r[k] - h.rp[k] : 0.f;
#pragma unroll
    for (int j = 0; j + 1 < M; ++j) { h.dX[j][k] = h.dX[j + 1][k]; h.dF[j][k] = h.dF[j + 1][k]; }
    h.dX[M - 1][k] = dx; h.dF[M - 1][k] = df;
    fp[k] = fx[k]; h.rp[k] = r[k];
  }
  have_prev = true;
  float q[NQ_];   // M = 3: 00 01 02 11 12 22 | 0r 1r 2r;  M = 2: 00 01 11 | 0r 1r
  if constexpr (CARRY) {
    // (uniform: read ahead of the filing above, moved to scalar registers here -- no vector register next to the products and the sums)
#pragma unroll
    for (int c = 0; c < NC; ++c) gc[c] = ufloat(gc[c]);
    // Summed in this call: the newest column against every column and the right-hand sides (M = 3: 02 12 22 | 0r 1r 2r).  The other
    // Gram entries are the previous call's, one column on (00 01 11 <- 11 12 22): the same lane products summed in the same order.
    float p[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) p[i] = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
      for (int i = 0; i < M; ++i) p[i] = fmaf(h.dF[i][k], h.dF[M - 1][k], p[i]);
#pragma unroll
      for (int i = 0; i < M; ++i) p[M + i] = fmaf(h.dF[i][k], r[k], p[M + i]);
    }
    wsum<NS, NW>(p, red, tid);
    int ac = 0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
      for (int j = i; j < M; ++j) q[aa_gram_at(i, j)] = j == M - 1 ? p[i] : gc[ac++];
      q[NG + i] = p[M + i];
    }
    ac = 0;
#pragma unroll
    for (int i = 0; i + 1 < M; ++i) {
#pragma unroll
      for (int j = i; j + 1 < M; ++j) red[NS + ac++] = q[aa_gram_at(i + 1, j + 1)];   // (cleared again below if the history restarts)
    }
  } else {
#pragma unroll
    for (int i = 0; i < NQ_; ++i) q[i] = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      int at = 0;
#pragma unroll
      for (int i = 0; i < M; ++i) {
#pragma unroll
        for (int j = i; j < M; ++j) { q[at] = fmaf(h.dF[i][k], h.dF[j][k], q[at]); ++at; }
      }
#pragma unroll
      for (int i = 0; i < M; ++i) { q[at] = fmaf(h.dF[i][k], r[k], q[at]); ++at; }
    }
    wsum<NQ_, NW>(q, red, tid);
  }
  float g[M];
  bool ok;
  if constexpr (M == 3) {
    const float tr = q[0] + q[3] + q[5];
    const bool have = tr > 0.f;
    const float reg = 1e-6f * tr + 1e-30f;
    // regularised normal equations by L D L' (uniform values)
    const float a00 = q[0] + reg, a11 = q[3] + reg, a22 = q[5] + reg, a01 = q[1], a02 = q[2], a12 = q[4];
    const float i0 = w_rcp(a00), l10 = a01 * i0, l20 = a02 * i0;
    const float d1 = fmaf(-l10, a01, a11), i1 = w_rcp(d1), t21 = fmaf(-l20, a01, a12), l21 = t21 * i1;
    const float d2 = fmaf(-l21, t21, fmaf(-l20, a02, a22)), i2 = w_rcp(d2);
    const float y0 = q[6], y1 = fmaf(-l10, y0, q[7]), y2 = fmaf(-l21, y1, fmaf(-l20, y0, q[8]));
    g[2] = y2 * i2; g[1] = fmaf(-l21, g[2], y1 * i1); g[0] = fmaf(-l20, g[2], fmaf(-l10, g[1], y0 * i0));
    ok = have && d1 > 0.f && d2 > 0.f && fabsf(g[0]) + fabsf(g[1]) + fabsf(g[2]) <= 1e4f;   // (a NaN fails the comparison)
    if (!have) have_prev = true; else if (!ok) { w_aa_reset<CARRY>(h, red); have_prev = false; }   // degenerate history: start again from this iterate
  } else {
    const float tr = q[0] + q[2];
    const bool have = tr > 0.f;
    const float reg = 1e-6f * tr + 1e-30f;
    const float a00 = q[0] + reg, a11 = q[2] + reg, a01 = q[1];
    const float i0 = w_rcp(a00), l10 = a01 * i0, d1 = fmaf(-l10, a01, a11), i1 = w_rcp(d1);
    const float y0 = q[3], y1 = fmaf(-l10, y0, q[4]);
    g[1] = y1 * i1; g[0] = fmaf(-l10, g[1], y0 * i0);
    ok = have && d1 > 0.f && fabsf(g[0]) + fabsf(g[1]) <= 1e4f;
    if (have && !ok) { w_aa_reset<CARRY>(h, red); have_prev = false; }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    float c = 0.f;
#pragma unroll
    for (int j = 0; j < M; ++j) c = fmaf(g[j], h.dX[j][k], c);
    xb[k] = ok ? fx[k] - (TM)c : fx[k];
  }
}

// ----------------------------------------------------------------------------------------------------- residuals of an ADMM iterate
// The leg-stage's share of OSQP's residuals of an ADMM iterate (u, z, y), hv = H u + g:  q = |r_prim|, |r_dual|, norm_prim, norm_dual
// (running maxima; differences in TV: the ADMM-only termination test of an fp64 run looks below fp32 resolution).
template <typename TV>
__device__ __forceinline__ void leg_residuals(const TV (&u)[3], const TV (&z)[5], const TV (&y)[5], const TV (&g)[3], const TV (&hv)[3], const TV mu,
                                              float (&q)[4]) {
  const TV m = mu * u[2];
  const TV gu[5] = {u[2], u[0] - m, u[0] + m, u[1] - m, u[1] + m};
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    q[0] = fmaxf(q[0], fabsf((float)(gu[i] - z[i])));
    q[2] = fmaxf(q[2], fmaxf(fabsf((float)gu[i]), fabsf((float)z[i])));
  }
  const TV Gy[3] = {y[1] + y[2], y[3] + y[4], y[0] + mu * (-y[1] + y[2] - y[3] + y[4])};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    q[1] = fmaxf(q[1], fabsf((float)(hv[a] + Gy[a])));
    q[3] = fmaxf(q[3], fmaxf(fabsf((float)(hv[a] - g[a])), fabsf((float)Gy[a])));
  }
}
// OSQP's rho-adaptation ratio sqrt((|r_prim| / norm_prim) / (|r_dual| / norm_dual)) from the reduced q, with sd = max(q[3], |g|_inf).
__device__ __forceinline__ float admm_ratio(const float (&q)[4], const float sd) {
  return sqrtf((q[0] / fmaxf(q[2], 1e-12f)) / fmaxf(q[1] / fmaxf(sd, 1e-12f), 1e-30f));
}

// ----------------------------------------------------------------------------------------------------- ADMM iteration
// rhs = sigma u - g + rho G'(z - yh)
template <typename TM>
__device__ __forceinline__ void leg_admm_rhs(const LegAdmm<TM>& A, const TM sigma, const TM r, TM (&rhs)[3]) {
  TM v[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) v[k] = A.z[k] - A.yh[k];
  const TM w0 = v[1] + v[2], w1 = v[3] + v[4], w2 = fma(A.mu, (v[2] - v[1]) + (v[4] - v[3]), v[0]);
  rhs[0] = fma(r, w0, fma(sigma, A.u[0], -A.g[0]));
  rhs[1] = fma(r, w1, fma(sigma, A.u[1], -A.g[1]));
  rhs[2] = fma(r, w2, fma(sigma, A.u[2], -A.g[2]));
}
// clip(t) to [lo, hi].  MED3 = false: fmin(fmax(t, lo), hi) -- a max, a min and, in a loop, one more max per bound that is not a
// constant: the instruction selector quiets every operand of a min / max that it cannot see to be canonical, and sees no further than
// the basic block (v_max x, x on the loop-invariant lo0 / hi0 / loA / hiB in EVERY iteration: four of the fourteen instructions that
// the five rows of the MIXED horizon-10 iteration spent on their clamps).  MED3 = true (fp32): the median of the three, one v_med3_f32,
// no quieting.  For finite t and lo <= hi the median is the clamp; the result WORDS of the two forms were compared on the device
// over every bound pair the kernels form and +-0, denormals, +-1e30, +-inf, NaN, the bounds and their neighbours: no difference,
// tools/clamp_forms.hip (tests/test_clamp_forms.py), and every row kind takes the median.  (A QP with a non-finite input never gets here.)
template <bool MED3, typename TM>
__device__ __forceinline__ TM leg_clip(const TM t, const TM lo, const TM hi) {
  if constexpr (MED3) {
    static_assert(sizeof(TM) == 4, "v_med3_f32");
    return __builtin_amdgcn_fmed3f(t, lo, hi);
  } else {
    return fmin(fmax(t, lo), hi);
  }
}
// Row k from its pre-projection value t = z + yh:  z = clip(t),  yh = t - z.
template <typename TM, bool MED3 = false>
__device__ __forceinline__ void leg_admm_project(LegAdmm<TM>& A, const int k, const TM t) {
  const TM lo = k == 0 ? A.lo0 : ((k & 1) ? A.loA : (TM)0), hi = k == 0 ? A.hi0 : ((k & 1) ? (TM)0 : A.hiB);
  const TM zn = leg_clip<MED3, TM>(t, lo, hi);
  A.yh[k] = t - zn;
  A.z[k] = zn;
}

}  // namespace
