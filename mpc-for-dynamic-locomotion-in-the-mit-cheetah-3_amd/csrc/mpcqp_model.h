// mpcqp_model.h -- per-robot model rows (include/mpcqp_model.h): the conversion of the caller's table into the engine's.
#pragma once
#include "mpcqp_common.h"
#include "../../include/mpcqp_model.h"

namespace {

// One thread per row: (m, Ixx, Iyy, Izz, f_min, f_max) -> (1 / m, 1 / Ixx, 1 / Iyy, 1 / Izz, f_min, f_max) (MODEL_ROW,
// mpcqp_common.h), and the table's address into the device configuration, where the solve kernels find it.  Plain fp64
// divisions, so a row made of the configuration's values gives what mpcqp_create computed from them (1.0 / m) and a
// configuration with exactly invertible values is reproduced bit for bit.  An invalid row (a non-finite entry, m <= 0, an inertia <= 0, f_min < 0, f_max < f_min) becomes six NaNs: the solve
// kernels' non-finite check then reports MPCQP_STATUS_NONFINITE for that QP alone.
__global__ void __launch_bounds__(256)
mpcqp_model_rows_kernel(const double* __restrict__ model, double* __restrict__ table, const int64_t B, DevCfg* __restrict__ dcfg) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b == 0) dcfg->model = table;
  if (b >= B) return;
  double v[MODEL_ROW];
#pragma unroll
  for (int i = 0; i < MODEL_ROW; ++i) v[i] = model[b * MODEL_ROW + i];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < MODEL_ROW; ++i) ok = ok && isfinite(v[i]);
  ok = ok && v[0] > 0.0 && v[1] > 0.0 && v[2] > 0.0 && v[3] > 0.0 && v[4] >= 0.0 && v[5] >= v[4];
  const double nan = __builtin_nan("");
#pragma unroll
  for (int i = 0; i < 4; ++i) table[b * MODEL_ROW + i] = ok ? 1.0 / v[i] : nan;
  table[b * MODEL_ROW + 4] = ok ? v[4] : nan;
  table[b * MODEL_ROW + 5] = ok ? v[5] : nan;
}

// mpcqp_clear_models: back to the configuration's row.
__global__ void mpcqp_model_clear_kernel(DevCfg* __restrict__ dcfg) { dcfg->model = nullptr; }

}  // namespace
