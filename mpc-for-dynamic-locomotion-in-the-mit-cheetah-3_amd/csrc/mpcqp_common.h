// mpcqp_common.h -- what the engines share besides mpcqp_device.h: the operator-tuple descriptor, packed-fp32 helpers, the solver
// policy constants, the element arithmetic of the tuple expansions, and the dispatch-order pre-pass (dearest-expected-first order of a batch that oversubscribes the device).
#pragma once
#include "mpcqp_device.h"
#include "mpcqp_order.h"   // the dispatch-order score: plain C++, also compiled on the host

namespace {

// Packed pairs: a register tile declared in f2 keeps each pair in an aligned register pair, and the rank-1 updates / mat-vecs map
// 1:1 onto v_pk_fma_f32.
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 mk2(float a, float b) { f2 t = {a, b}; return t; }   // NB: (f2)(a, b) would be a cast of a comma expression
__device__ __forceinline__ f2 splat2(float v) { return mk2(v, v); }

// Inputs of one solve: the operator tuple (x0, r, contact, xdes, mu).  The descriptor fields belong to the gait entry point,
// whose expansion kernel (mpcqp_elementwise.h) turns them into a tuple in the engine's workspace before the solve.
template <typename TIO>
struct FastIn {
  const TIO* x0; const TIO* r; const uint8_t* contact; const TIO* xdes; const TIO* mu;             // tuple form
  const TIO* ref; const TIO* feet0; const TIO* footholds; const int32_t* gait; const uint8_t* feet_id;   // gait form
  const TIO* u_init;   // MPCQP_FLAG_WARM_START: primal initial guess [B,N,12] (aliases the output buffer), else null
  float* y_state;      // ... and the engine's per-slot record of the previous solve's multipliers [cap][40][5] (read, then rewritten)
  int shift;           // MPCQP_FLAG_WARM_SHIFT: the guess and the record are one control tick old: use stage k + 1 for stage k
};

// Element arithmetic of an expansion into the operator tuple, shared by the expand kernels of mpcqp_elementwise.h and mpcqp_gaits.h.
// Element c of x_des[k].  rf: the reference row [roll, pitch, yaw, com (3), v (3), w]; g: the state's gravity entry; gate: 0 where the
// references are zeroed (roll-out, last plan step), else 1.
template <typename TIO>
__device__ __forceinline__ double xdes_elem(const TIO* rf, const TIO g, const int k, const int c, const double d, const double gate) {
  if (c < 2) return (double)rf[c];
  if (c == 2) return (double)rf[2] + (double)k * d * gate * (double)rf[9];
  if (c < 6) return (double)rf[c] + (double)k * d * gate * (double)rf[6 + (c - 3)];
  if (c < 8) return 0.0;
  if (c == 8) return gate * (double)rf[9];
  if (c < 12) return gate * (double)rf[6 + (c - 9)];
  return (double)g;
}

// Component a of a lever arm r[k][l] = foot - com: the measured com at stage 0, the reference's from stage 1 on.  (TF: the foot as
// stored, or in fp64 where a rule has just computed it)
template <typename TF, typename TIO>
__device__ __forceinline__ double lever_elem(const TF foot, const TIO* rf, const TIO* x, const int k, const int a, const double d,
                                             const double gate) {
  const double com = k == 0 ? (double)x[3 + a] : (double)rf[3 + a] + (double)k * d * gate * (double)rf[6 + a];
  return (double)foot - com;
}

// A model row as the engine keeps it (DevCfg::model, mpcqp_model.h): 1 / m, 1 / Ixx, 1 / Iyy, 1 / Izz, f_min, f_max.  An invalid
// row is six NaNs.
constexpr int MODEL_ROW = 6;


#ifndef MPCQP_HARD_ITER_FACTOR
#define MPCQP_HARD_ITER_FACTOR 2
#endif
constexpr int ADAPT_AT = 25;             // iteration of the single early rho check of a cold solve's first ADMM block (both engines)
constexpr float ADAPT_RHO_MAX = 30.f;    // cap of the penalty a QP that triggers it goes on with
constexpr double ALPHA_EASY = 1e-2;      // regulariser at which the active-set search is done (continuation start)
constexpr int HARD_ITER_FACTOR = MPCQP_HARD_ITER_FACTOR;      // ADMM block length of the QPs that trigger it (x check_every)
constexpr int HARD_POLISH_FACTOR = 2;    // ... and their polish-step budget (x polish_max)
#ifndef MPCQP_WARM_POLISH
#define MPCQP_WARM_POLISH 2
#endif
constexpr int WARM_POLISH = MPCQP_WARM_POLISH;   // polish steps tried on a warm-start guess before the first ADMM block
#ifndef MPCQP_WARM_K
#define MPCQP_WARM_K 60
#endif
constexpr int WARM_K = MPCQP_WARM_K;             // length of the first ADMM block when it starts from remembered (u, y)
#ifndef MPCQP_WARM_FRAC10
#define MPCQP_WARM_FRAC10 4
#endif
constexpr int WARM_FRAC10 = MPCQP_WARM_FRAC10;   // ... in tenths of a cold solve's first block (at most WARM_K): 24 iterations at horizon 10
                                                 // (roll-out of 4096 robots x 100 ticks: 2 / 3 / 4 / 6 / 8 / 10 tenths -> 12.9 / 13.5 / 15.0 / 14.3 / 14.0 / 13.4 M
                                                 //  robot-ticks/s, cold solves 13.4 M; profiles/r03f_rollout_warm.txt)
constexpr float WARM_KKT_TOL = 1e-3f;            // (u0, y0) counts as a KKT point when its stationarity residual is below this x |g|

// ------------------------------------------------------------------------------------------------------ dispatch order
// Workgroups are handed out in blockIdx order, and the solve time of a QP varies by 7x (one early rho check, up to four
// ADMM blocks, 1-8 polish steps): with 4096 QPs on 2048 workgroup slots the two-round QPs that start in the second fill set
// the time of the launch (measured 0.32-0.33 ms against 0.25-0.26 ms for the same QPs dispatched dearest-first by their realised
// cost, profiles/r30_order_predictor.txt).  A pre-pass therefore sorts the QPs into ORDER_BUCKETS classes of expected cost and
// the solve kernel takes the dearest class first.  The score and its fit live in mpcqp_order.h (plain C++, checked on the
// host): the log-odds of a second ADMM round from the shape of the support schedule (a horizon that BEGINS in a run of
// friction-saturated two-legged stages; a four-legged start that goes to two legs early), the friction demand and the commanded
// horizontal velocity correction over mu.  Order only: results are per QP.
struct OrderBuf { int* cnt; int* list; int cap; int* head; int* zero; };   // cnt[ORDER_BUCKETS], list[ORDER_BUCKETS][cap], queue head;
                                                                           // zero: the OTHER call's 32 header ints, cleared by this call's pre-pass
static_assert(ORDER_BUCKETS + 1 <= 32, "class counters and the queue head share a header set of 32 ints");

// 16 lanes per QP, one stage per lane (horizons beyond 16: a lane takes stages k0, k0 + 16): the loads of a QP go out together,
// ballots collect the rows' two-legged / saturated stage masks, DPP row reductions the maxima and the stance count, lane 0 of the
// row classes the QP.  The first wave then files the workgroup's 64 QPs: a ballot per class gives each QP its position among
// the workgroup's QPs of its class IN BATCH ORDER (a prefix count, no atomic) and the class its count, the class counters are
// bumped once per workgroup (a global atomic per QP on a handful of addresses serialises) -- so the order inside a class is
// that of the batch within a workgroup, and the workgroups' arrival across them.
template <typename TIO, int N>
__global__ void __launch_bounds__(1024)
mpcqp_order_kernel(const FastIn<TIO> in, const int B, const OrderBuf ob) {
  static_assert(N <= 32, "one mask bit per stage");
  __shared__ int lcls[64];
  // Two sets of class counters + queue head alternate between calls: this pre-pass counts into one (cleared by the previous call's
  // pre-pass, whose solve has finished with it: one stream per handle) and clears the other for the next call -- no memset launch.
  if (blockIdx.x == 0 && threadIdx.x < 32 && ob.zero) ob.zero[threadIdx.x] = 0;
  const int q = threadIdx.x >> 4, b = blockIdx.x * 64 + q, k0 = threadIdx.x & 15, row = 16 * (q & 3);
  const bool live = b < B;
  float inv_mu = 0.f, vx = 0.f, vy = 0.f;
  bool bad = false;
  if (live) {
    const float mu = (float)in.mu[b];
    bad = !isfinite(mu);
    inv_mu = 1.f / fmaxf(fabsf(mu), 1e-3f);
    vx = (float)in.x0[(size_t)b * 13 + 9]; vy = (float)in.x0[(size_t)b * 13 + 10];
  }
  uint32_t two = 0, sat = 0;
  float dmax = 0.f, hvmax = 0.f, cnt = 0.f;
#pragma unroll
  for (int p = 0; p < (N + 15) / 16; ++p) {
    const int k = k0 + 16 * p;
    OrderStage s = {0.f, 0.f, 0.f, false, false, false};
    if (live && k < N) {
      float r[12]; bool ct[4];
      const TIO* rp = in.r + ((size_t)b * N + k) * 12;
#pragma unroll
      for (int i = 0; i < 12; ++i) r[i] = (float)rp[i];
#pragma unroll
      for (int l = 0; l < 4; ++l) ct[l] = in.contact[((size_t)b * N + k) * 4 + l] != 0;
      const TIO* xk = in.xdes + ((size_t)b * (N + 1) + k + 1) * 13;   // stage k steers towards x_des[k + 1]
      s = order_stage(r, ct, vx - (float)xk[9], vy - (float)xk[10], inv_mu);
    }
    // (all lanes of the wave are here: the ballots and the DPP moves below see every row)
    const unsigned long long m2 = __ballot(s.two), ms = __ballot(s.sat), mb = __ballot(s.bad);
    two |= (uint32_t)((m2 >> row) & 0xffffu) << (16 * p);
    sat |= (uint32_t)((ms >> row) & 0xffffu) << (16 * p);
    bad = bad || ((mb >> row) & 0xffffu) != 0;
    dmax = fmaxf(dmax, s.demand); hvmax = fmaxf(hvmax, s.hv); cnt += s.nst;   // (fmaxf drops a NaN: `bad` has it)
  }
  dmax = fmaxf(dmax, dpp_mov<0xB1>(dmax));    // max / sum over the row of 16 lanes
  dmax = fmaxf(dmax, dpp_mov<0x4E>(dmax));
  dmax = fmaxf(dmax, dpp_mov<0x141>(dmax));
  dmax = fmaxf(dmax, dpp_mov<0x140>(dmax));
  hvmax = fmaxf(hvmax, dpp_mov<0xB1>(hvmax));
  hvmax = fmaxf(hvmax, dpp_mov<0x4E>(hvmax));
  hvmax = fmaxf(hvmax, dpp_mov<0x141>(hvmax));
  hvmax = fmaxf(hvmax, dpp_mov<0x140>(hvmax));
  cnt += dpp_mov<0xB1>(cnt);
  cnt += dpp_mov<0x4E>(cnt);
  cnt += dpp_mov<0x141>(cnt);
  cnt += dpp_mov<0x140>(cnt);
  if (k0 == 0) lcls[q] = live ? cost_class(N, two, sat, cnt, dmax, hvmax, bad) : -1;
  __syncthreads();
  if (threadIdx.x < 64) {   // the first wave: lane = QP of the workgroup
    const int lane = threadIdx.x, cls = lcls[lane];
    int pos = 0, mine = 0;
#pragma unroll
    for (int c = 0; c < ORDER_BUCKETS; ++c) {
      const unsigned long long m = __ballot(cls == c);
      if (cls == c) pos = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == c) mine = __popcll(m);
    }
    int base = 0;
    if (lane < ORDER_BUCKETS && mine) base = atomicAdd(&ob.cnt[lane], mine);
    base = __shfl(base, cls < 0 ? 0 : cls);   // cls is cost_class's clamped integer, or -1 past the end of the batch
    if (cls >= 0) ob.list[(size_t)cls * ob.cap + base + pos] = blockIdx.x * 64 + lane;
  }
}

}  // namespace
