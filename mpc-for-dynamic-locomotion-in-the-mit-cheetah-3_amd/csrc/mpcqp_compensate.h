// mpcqp_compensate.h -- the wrench observer and the disturbance table update inside the tick loop of mpcqp_rollout_observe (the C-ABI is
// include/mpcqp_compensate.h, which has the rule; the entry point lives in mpcqp_kernels.hip).  One kernel per tick, behind the estimator's
// predict and the legs step and in front of the advance: the tick's operands are still the live buffers (or the estimator's side buffers, which
// the predict kernel does not write), the observer's row is dist_observer_row of mpcqp_disturb.h -- the row of mpcqp_disturb_track_kernel,
// written once -- and on an update tick the same lane writes the robot's row of the handle's table, which the shift kernel of the next
// tick's solve reads.  A second, one-off kernel converts dist_state[:,0:6] into the table when the call begins, by the same rule.
//
// One lane per robot, the layout of the log pass.  What a lane moves is its robot's 40 state doubles in and out, 36 I/O elements of
// operands, 7 of the body row and up to 18 of outputs: the 64 robots of a wave own one contiguous span of each buffer (64 x 320 bytes of
// state), so every cache line the wave fetches is used in full by that wave, as the shift kernel's comment in mpcqp_disturb.h argues for
// its rows.  The arithmetic is some 150 fp64 operations per robot and a sine / cosine pair; what bounds the launch is the state it moves:
// 640 bytes in and out per robot, 0.8 KB with the operands, 55 MB at 65 536 robots, measured at +17 us per tick there and +10 to +12 us
// at 4096 (tools/rollout_compensate_rate.py, profiles/r31_compensate.txt) against ticks of 4.1 and 0.42 ms.  Four lanes per robot with a
// quad reduction for the leg sums -- whose order (0 + 1) + (2 + 3) it would have to keep -- moves the same bytes and adds the exchanges:
// it was not built.  No LDS, no scratch (every index is a constant after unrolling); masks and poison are selects.
#pragma once
#include "mpcqp_disturb.h"
#include "../../include/mpcqp_compensate.h"

namespace {

// A table row as mpcqp_disturb_rows_kernel converts it: a non-finite entry makes six NaNs.
__device__ __forceinline__ void dist_table_row(const double (&v)[DIST_ROW], double* __restrict__ row) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < DIST_ROW; ++i) ok = ok && isfinite(v[i]);
#pragma unroll
  for (int i = 0; i < DIST_ROW; ++i) row[i] = ok ? v[i] : __builtin_nan("");
}

// The table a call begins with: row b = state[b, 0:6] as the I/O type holds it -- what the update tick behind that state wrote, so that a
// call cut at a multiple of `hold` goes on under the uncut call's table --, one thread per robot.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_compensate_enter_kernel(const double* __restrict__ state, double* __restrict__ table, const int64_t B) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double v[DIST_ROW];
#pragma unroll
  for (int i = 0; i < DIST_ROW; ++i) v[i] = (double)(TIO)state[b * DIST_STATE + i];
  dist_table_row(v, table + b * DIST_ROW);
}

// Tick `it` of mpcqp_rollout_observe_compensated: lane b runs one row of the observer on robot b's state.  x [B,13] (12 are read),
// f robot b's forces at f + b fstride, feet [B,4,3]: the live state, the applied forces and the live feet (MPCQP_WRENCH_TRUTH), or the
// estimator's x^, the solve's stage-0 forces and f^eet (MPCQP_WRENCH_SENSED).  est: null, or the estimator's state [B,EST_STATE] behind
// its predict step, whose NaN marks a robot whose `est` row of this tick is NaN (the predict poisons the log row, not the side buffer).
// body [B,7] or null: the body the observer believes.  dist / resid [B,T,6] or null.  update: write robot b's row of `table`, d^ as the
// I/O type holds it.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_compensate_tick_kernel(const TIO* __restrict__ x, const TIO* __restrict__ f, const int64_t fstride, const TIO* __restrict__ feet,
                             const double* __restrict__ est, const TIO* __restrict__ body, const PlantModel model, const DistPar par,
                             double* state, double* __restrict__ table, TIO* __restrict__ dist, TIO* __restrict__ resid, const int64_t B,
                             const int T, const int it, const bool update) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double* const sb = state + b * DIST_STATE;
  double bd[7], Ii[6];
  plant_body_row(body, model, b, bd);
  const double Ib[6] = {bd[1], bd[2], bd[3], bd[4], bd[5], bd[6]};
  DistLane s;
  dist_state_load(sb, plant_inertia(bd[0], Ib, Ii), s);
  if (est) s.ok = s.ok && isfinite(est[b * EST_STATE + EST_LIVE]);
  double res[6], row[DIST_ROW];
  dist_observer_row(x + 13 * b, f + b * fstride, feet + 12 * b, bd[0], Ib, par, s, res);
  const int64_t o = 6 * (b * T + it);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const TIO dv = est_out<TIO>(s.ok, s.dh[i]);
    row[i] = (double)dv;
    if (dist) dist[o + i] = dv;
    if (resid) resid[o + i] = est_out<TIO>(s.ok, res[i]);
  }
  if (update) dist_table_row(row, table + b * DIST_ROW);
  dist_state_store(sb, s);
}

}  // namespace
