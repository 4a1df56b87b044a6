// mpcqp_order.h -- the score of the dispatch-order pre-pass (mpcqp_common.h: mpcqp_order_kernel): what one stage contributes
// (order_stage) and the class of expected cost of a QP from the terms gathered over its stages (cost_class).
// Plain C++: a host compiler can include this file (no device builtin, no lane operation).  Host check: tools/order_check.cpp
// (tests/test_order_host.py).  The fit that produced the constants: tools/order_fit.py.
//
// WHAT IS PREDICTED.  A QP of the bench workload costs one ADMM round (60 iterations, 1-3 polish steps, ~100-150 us in a full
// device) or, 3 % of them, two rounds or more (160+ iterations, 3-7 polish steps, 225-270 us).  A launch of a few device-fills ends
// with the two-round QPs that were dispatched after the first fill, so the score is the log-odds of a second round; the
// one-round cost (stance-leg count) no longer enters it (its weight fitted to -0.01 per swing leg-stage and changes no rank).
// Which QPs take a second round (224 seeds of the bench workload, 26 000 of them out of 917 000):
//   * those whose horizon BEGINS inside a run of two-legged, friction-saturated stages (demand / mu > 1: the com is further from
//     the line through the two feet than mu h): 0 / 2 / 15 / 49 / 74 / 83 % for a leading run of <= 2 / 3 / 4 / 5 / 6 / 7+ stages at
//     mu = 0.3, a third of that at 0.5, none at 0.7.  The same run at the END of the horizon costs nothing (0 of 3 100): the
//     stages before it pre-load the body.  The round-1 predictor (maximum demand over the horizon, times 34 us, plus 2.2 us per
//     stance leg-stage) ranked both alike and put a long saturated run BEHIND a short one, for its fewer stance legs.
//   * rarely (0.4 %) a QP that starts on four legs and goes to two within the first stages: the sooner and the longer the run,
//     the likelier (1.4 % for one four-leg stage followed by nine two-leg stages, 0.01 % for a horizon that starts on two).
//   * with the size of the commanded horizontal velocity correction over mu (the implied horizontal-to-vertical force ratio
//     against the cone): rank correlation with a second round inside a support-pattern cell 0.73 (area under the ROC curve).
// Position, attitude and vertical errors of the free response, and the implied vertical force against n_stance f_max, were fitted
// and carry nothing in this workload (area under the curve 0.49-0.54, coefficient within its standard error of zero): left out.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ORDER_FN __host__ __device__ __forceinline__
#else
#define ORDER_FN inline
#endif

namespace {

constexpr int ORDER_BUCKETS = 16;

// Friction demand of a support pattern: for a stage carried by two feet, the horizontal distance d of the com from the line
// through the feet over the com height h is the friction coefficient a static stance would need; one foot: its own offset.
// NaN when an intermediate is not finite (order_stage then marks the stage bad); a swing leg's lever arm is never read.
ORDER_FN float support_demand(int nst, const float (&fx)[4], const float (&fy)[4], const float (&fz)[4], const bool (&st)[4]) {
  if (nst == 2) {
    int a = -1, bidx = -1;
    for (int l = 0; l < 4; ++l) { if (st[l]) { if (a < 0) a = l; else bidx = l; } }
    const float dx = fx[a] - fx[bidx], dy = fy[a] - fy[bidx];
    const float n2 = dx * dx + dy * dy, cr = fabsf(fx[a] * fy[bidx] - fy[a] * fx[bidx]), hz = -0.5f * (fz[a] + fz[bidx]);
    if (!std::isfinite(n2 + cr + fabsf(hz))) return NAN;   // (an overflowed square would otherwise divide to a finite 0)
    return cr / fmaxf(sqrtf(n2), 1e-6f) / fmaxf(hz, 1e-3f);
  }
  if (nst == 1) {
    for (int l = 0; l < 4; ++l) {
      if (!st[l]) continue;
      const float n2 = fx[l] * fx[l] + fy[l] * fy[l];
      if (!std::isfinite(n2 + fabsf(fz[l]))) return NAN;
      return sqrtf(n2) / fmaxf(-fz[l], 1e-3f);
    }
  }
  return 0.f;   // three or four feet (or flight): no friction-limited moment balance
}

// One stage's terms.  r: the stage's 12 lever-arm entries, ct: its 4 contact flags, ev: horizontal velocity of the state minus the
// stage's target (x0[9..10] - xdes[k + 1][9..10]), inv_mu = 1 / max(|mu|, 1e-3).
struct OrderStage {
  float nst;       // stance legs
  float demand;    // support_demand / mu
  float hv;        // |ev| / mu
  bool two;        // carried by one or two feet
  bool sat;        // ... and friction-saturated: demand > 1
  bool bad;        // a non-finite term: the QP goes to class 0
};
ORDER_FN OrderStage order_stage(const float (&r)[12], const bool (&ct)[4], float evx, float evy, float inv_mu) {
  float fx[4], fy[4], fz[4];
  int nst = 0;
  for (int l = 0; l < 4; ++l) { fx[l] = r[3 * l]; fy[l] = r[3 * l + 1]; fz[l] = r[3 * l + 2]; nst += ct[l] ? 1 : 0; }
  OrderStage s;
  s.nst = (float)nst;
  s.demand = support_demand(nst, fx, fy, fz, ct) * inv_mu;
  s.hv = sqrtf(evx * evx + evy * evy) * inv_mu;
  s.two = nst == 1 || nst == 2;
  s.bad = !(std::isfinite(s.demand) && std::isfinite(s.hv));
  s.sat = s.two && s.demand > 1.f;
  return s;
}

ORDER_FN int order_ctz(uint32_t v) { return v ? __builtin_ctz(v) : 32; }
ORDER_FN int order_popc(uint32_t v) { return __builtin_popcount(v); }

// Class of a QP, dearest = ORDER_BUCKETS - 1, from the terms over its N <= 32 stages (bit k of a mask = stage k):
//   two / sat   OrderStage::two / ::sat;   nst_sum  stance leg-stages;   dmax  max demand;   hvmax  max hv;   bad  any OrderStage::bad
// z is the log-odds of a second ADMM round: logistic regression on the engine's own iteration counts, 200 batches of 4096 of the bench
// workload (seeds 25-224; the bench seed and seeds 1-24 held out; tools/order_fit.py, profiles/r30_order_predictor.txt):
//   two-round QPs dispatched after the first 2048 of 4096, per batch, held-out seeds: 4.7 with the round-1 score, 1.4 with this one
//   (a score that knew every support-pattern cell's true rate: 1.0 -- the rest are one-in-a-thousand QPs of any pattern).
// A class is half a unit of z; positions inside a class are in batch order.  Every index below is an integer clamped to its range.
ORDER_FN int cost_class(int N, uint32_t two, uint32_t sat, float nst_sum, float dmax, float hvmax, bool bad) {
#ifdef MPCQP_ORDER_ROUND1   // diagnostic build: the round-1 score (2.2 us per stance leg-stage + 34 us per unit of demand, classes of 10 us)
  const float us = 2.2f * (nst_sum * (10.f / (float)N)) + 34.f * fminf(dmax, 2.f);   // under this pre-pass, to time the two apart
  return (!bad && std::isfinite(us)) ? (int)fminf(us * 0.1f, (float)(ORDER_BUCKETS - 1)) : 0;
#endif
  const uint32_t all = N >= 32 ? 0xffffffffu : ((1u << N) - 1u);
  two &= all; sat &= all;
  const int lead = order_ctz(~sat);                            // saturated stages the horizon begins with
  int s = order_ctz(two); if (s > N) s = N;                     // first two-legged stage, its run [s, s + L) and the saturated ones in it
  const uint32_t from_s = s < 32 ? (two >> s) : 0u;
  const int L = order_ctz(~from_s);
  const uint32_t run = (L >= 32 ? 0xffffffffu : ((1u << L) - 1u)) << (s < 32 ? s : 0);
  const int nsat = order_popc(sat & run);
  const float late = s >= 1 ? ldexpf((float)L, 1 - s) : 0.f;   // a run that starts after s four-legged stages: L / 2^(s - 1)
  const float late_sat = late * (float)nsat / (float)(L > 1 ? L : 1);
  const float has_late = (s >= 1 && L >= 1) ? 1.f : 0.f;
  const float swing10 = 40.f - nst_sum * (10.f / (float)N);
  float z = -9.2251f;
  z += 1.0399f * (float)(lead < 6 ? lead : 6);
  z += 1.0684f * fminf(dmax, 2.f);
  z += 0.14989f * late;
  z += 0.11830f * late_sat;
  z += 1.1557f * hvmax;
  z += 2.2787f * has_late;
  z += -0.013650f * swing10;
  if (bad || !std::isfinite(z)) return 0;
  return (int)fminf(fmaxf((z + 9.5f) * 2.f, 0.f), (float)(ORDER_BUCKETS - 1));
}

}  // namespace
