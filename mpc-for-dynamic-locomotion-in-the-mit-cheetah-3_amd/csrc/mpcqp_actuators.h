// mpcqp_actuators.h -- per-robot actuator rows with a torque-speed curve (the C-ABI is include/mpcqp_actuators.h, which has the
// envelope and the rules; the entry points live in mpcqp_kernels.hip): the conversion of the caller's table into the engine's and the
// one clamp that the swing control periods (mpcqp_legsim.h, mpcqp_legroll.h), the stance rule (mpcqp_drive.h) and the limit byte of
// mpcqp_leg_effort (mpcqp_legdyn.h) share in their ACT instantiations.
//
// A row is act[b] = (tau_max[3], qd_knee[3], qd_free[3]) in fp64 whatever the I/O type.  The kernels read it from the table, nine
// loads per lane where it is used, never as a by-value argument: the by-value rows of those kernels are at the size at which their
// first promotion round still runs (mpcqp_legdyn.h), and the legs step, at 256 VGPRs, is not given nine more doubles to hold across
// its control periods (act_row_here).  The envelope runs without contraction and its masks are selects.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace {

constexpr int ACT_ROW = 9;   // tau_max, qd_knee, qd_free of HipX, HipY, Knee

struct ActLim { double lo, hi; };

// The torque a joint can deliver at rate r: the full tau_max up to |r| = knee, falling linearly to 0 at |r| = fre on the motoring
// side (the side of r's sign); the braking side keeps tau_max.  knee = +inf never takes the falling branch: the flat box.
__device__ __forceinline__ ActLim act_limits(const double r, const double tmax, const double knee, const double fre) {
#pragma clang fp contract(off)
  const double a = fabs(r), d = fre - a;
  // (the falling part is formed first and then selected: written inside the conditional, its division is kept under a branch, and a
  //  branch in the middle of a control period splits the block whose multiply-adds the parent kernels fuse as one)
  const double fall = tmax * ((d > 0.0 ? d : 0.0) / (fre - knee));
  const double avail = a > knee ? fall : tmax;
  return {r < 0.0 ? -avail : -tmax, r > 0.0 ? avail : tmax};
}

// Joint j of the row at `row`: the commanded torque t at rate r -> the applied one.  With knee = +inf this is clamp_sym(t, tau_max)
// bit for bit (a NaN t stays); a row the conversion kernel found invalid is NaN and gives NaN.
__device__ __forceinline__ double act_clamp(const double* __restrict__ row, const int j, const double t, const double r) {
  const double tmax = row[j];
  const ActLim m = act_limits(r, tmax, row[3 + j], row[6 + j]);
  const double app = t > m.hi ? m.hi : (t < m.lo ? m.lo : t);
  return tmax == tmax ? app : __builtin_nan("");
}

// True when t lies outside the envelope at rate r (mpcqp_leg_effort's limit bit 4); false for an invalid row, which the caller poisons.
__device__ __forceinline__ bool act_beyond(const double* __restrict__ row, const int j, const double t, const double r) {
  const ActLim m = act_limits(r, row[j], row[3 + j], row[6 + j]);
  return t > m.hi || t < m.lo;
}

// The row with its address made opaque: a load through it is not moved out of the loop it stands in.
__device__ __forceinline__ const double* act_row_here(const double* row) {
  asm volatile("" : "+v"(row));
  return row;
}

// The table of a kernel whose last template argument is the pack ACTROW: nothing (no table: null), or double (one table [B,9], the
// kernel's last parameter `const ACTROW* __restrict__... actp`).  A pack and not a bool plus a struct that holds the pointer: an
// empty struct still takes 8 bytes of the kernel's argument block and moves the hidden arguments, and a pointer inside a struct
// loses its no-alias marking, which schedules the table kernel differently.
__device__ __forceinline__ const double* act_rows() { return nullptr; }
__device__ __forceinline__ const double* act_rows(const double* act) { return act; }

// mpcqp_set_actuators: one thread per row.  A row is valid when every tau_max is finite and >= 0, every qd_knee >= 0 and each joint
// has either qd_knee = +inf (any qd_free) or finite qd_knee < qd_free < inf; an invalid row is stored as nine NaN.
__global__ void __launch_bounds__(256)
mpcqp_actuator_rows_kernel(const double* __restrict__ in, double* __restrict__ out, const int64_t B) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double r[ACT_ROW];
#pragma unroll
  for (int e = 0; e < ACT_ROW; ++e) r[e] = in[ACT_ROW * b + e];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double tm = r[j], kn = r[3 + j], fr = r[6 + j];
    const bool flat = kn > 0.0 && isinf(kn);
    ok = ok && isfinite(tm) && tm >= 0.0 && kn >= 0.0 && (flat || (isfinite(kn) && isfinite(fr) && fr > kn));
  }
  const double nan = __builtin_nan("");
#pragma unroll
  for (int e = 0; e < ACT_ROW; ++e) out[ACT_ROW * b + e] = ok ? r[e] : nan;
}

}  // namespace
