// mpcqp_slip.h -- stance feet that slide: the stance drive's rule with slip kinematics behind it (the C-ABI is mpcqp_stance_slip and
// mpcqp_rollout_slip in include/mpcqp_slip.h, which has the rule; the entry points live in mpcqp_kernels.hip).  Two kernels:
//   mpcqp_stance_slip_kernel   the rule for one (robot, leg).  mpcqp_stance_slip runs it on the caller's rows; mpcqp_rollout_slip runs the
//                              SAME instantiation per tick on the live buffers where mpcqp_rollout_drive runs mpcqp_stance_drive_kernel,
//                              with the same side buffers plus one: the displacement [B,4,2] in the I/O type.  The slip state is read
//                              and written in place; the row's s0 goes to slip_log.
//   mpcqp_slip_finish_kernel   after the landing of a tick, one launch for what the drive's log kernel does and the foot move: on stance
//                              rows tau_log becomes the rule's torque and flag_log gains the bits 2 / 16 / 32 / 128; a leg that was in
//                              stance on the row's tick and does not touch down on the new one has its foot moved by the displacement; a
//                              leg that touches down has its slip entry zeroed.  Seven launches per tick with or without logs.
// One kernel for both entry points is what makes the roll-out's logs replay bit for bit through mpcqp_stance_slip.
//
// Layout and conventions are mpcqp_drive.h's: one thread per (robot, leg), fp64, no LDS, geometry and limits by value, the rule's own
// arithmetic without contraction, masks as selects.  The rule is mpcqp_drive.h's device functions -- stance mask, steps 2, 3 and 5,
// common stores, log step --; this file has what a sliding foot adds: step 4 (slip_slide), the slip kernel's own operands, poison
// test and stores, and the foot move.  The row (R, pw, q, tau_cmd, J) is the drive kernel's lines, in both kernels (see there).
// Not built: a reach stop, static versus kinetic friction, anisotropic foot inertia, a landing foot's residual velocity, the legs'
// reaction on the torso; the stance rows of the q / qd logs still assume the held foot at rest (include/mpcqp_slip.h).
#pragma once
#include "../../include/mpcqp_slip.h"
#include "mpcqp_drive.h"

namespace {

constexpr unsigned SLIP_SLIDING = 128u;                   // MPCQP_DRIVE_SLIDING (include/mpcqp_slip.h)
constexpr unsigned SLIP_BITS = DRIVE_BITS | SLIP_SLIDING;   // what the rule adds to a stance row's flag

// Step 4 for a sliding foot, in the place of drive_cone: the slide of one foot over a tick and the force the ground returned.  f1 the
// force the leg delivers, s0 the foot's velocity, mu the ground's friction, me the foot's effective mass, n substeps of h = delta / n.
// s and d are the end velocity and the displacement.
// Returns f2, the applied force (a pull: 0; a sliding leg: the tick average; any other leg: f1 by value, the caller selects).
__device__ __forceinline__ V3 slip_slide(const V3 f1, const double s0x, const double s0y, const double mu, const double me, const int n,
                                         const double h, const double delta, double& sx, double& sy, double& dx, double& dy, bool& sliding) {
#pragma clang fp contract(off)
  const bool pull = f1.z <= 0.0;
  const double fn = pull ? 0.0 : f1.z, hm = h / me;
  const double cap = (mu * fn) * hm, vx = -f1.x * hm, vy = -f1.y * hm;
  sx = s0x; sy = s0y; dx = 0.0; dy = 0.0;
  for (int k = 0; k < n; ++k) {
    const double tx = sx + vx, ty = sy + vy;
    const double nrm = sqrt(tx * tx + ty * ty);
    const bool stick = nrm <= cap;   // (|s*| = 0 sticks whatever cap >= 0 is: the quotient below is then never selected)
    const double keep = 1.0 - cap / nrm;
    sx = stick ? 0.0 : tx * keep;
    sy = stick ? 0.0 : ty * keep;
    dx += h * sx;
    dy += h * sy;
  }
  sliding = s0x != 0.0 || s0y != 0.0 || sx != 0.0 || sy != 0.0;
  const double med = me / delta;
  return {pull ? 0.0 : (sliding ? f1.x + med * (sx - s0x) : f1.x), pull ? 0.0 : (sliding ? f1.y + med * (sy - s0y) : f1.y), pull ? 0.0 : f1.z};
}

// i = 4 b + leg.  The operands of mpcqp_stance_drive_kernel with the same meaning (x, f / fstride, feet, contact or the gait clock, ground,
// geo, lim, drive, f_out, tau, flag, cmd / cstride), and: foot_mass [B]; slip_in double [B,4,2]; n, h = delta / n, delta; slip_out double
// [B,4,2] or null (may be slip_in: a lane reads its own two values before it writes them); disp [B,4,2] or null; slog or null: the
// row's s0 as read, robot b's at slog + b sstride.
// ACTROW as in mpcqp_stance_drive_kernel; the envelope's rates are those of a foot moving at s0: (s0, 0) - v - omega x (foot - c).
template <typename TIO, typename... ACTROW>
__global__ void __launch_bounds__(256)
mpcqp_stance_slip_kernel(const TIO* __restrict__ x, const TIO* f, const int64_t fstride, const TIO* __restrict__ feet,
                         const uint8_t* __restrict__ contact, const int32_t* __restrict__ gait, const int32_t* __restrict__ tick,
                         const TIO* __restrict__ ground, const TIO* __restrict__ foot_mass, const double* slip_in, const LegGeoDev geo,
                         const LegLimDev lim, const int drive, const int n, const double h, const double delta, TIO* f_out,
                         TIO* __restrict__ tau, uint8_t* __restrict__ flag, TIO* __restrict__ cmd, const int64_t cstride, double* slip_out,
                         TIO* __restrict__ disp, double* __restrict__ slog, const int64_t sstride, const int64_t B,
                         const ACTROW* __restrict__... actp) {
  constexpr bool ACT = sizeof...(ACTROW) != 0;
  const double* const act = act_rows(actp...);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  const TIO* xb = x + 13 * b;
  const TIO* fb = f + b * fstride + 3 * l;
  const TIO fr[3] = {fb[0], fb[1], fb[2]};
  const double s0x = slip_in[2 * i], s0y = slip_in[2 * i + 1];
  const bool stance = stance_mask(contact, gait, tick, i, b, l);
  // the drive's row: R from the rotation vector, the foot seen from the CoM, q and tau_cmd (in the kernel: see mpcqp_stance_drive_kernel)
  double qt[4], pw[3], fl[3], ql[3], tl[3];
  plant_rotvec_to_quat((double)xb[0], (double)xb[1], (double)xb[2], qt);
  const double qw = qt[0], qx = qt[1], qy = qt[2], qz = qt[3];
  const double R[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                       2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                       2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    pw[a] = (double)feet[3 * i + a] - (double)xb[3 + a];
    fl[a] = (double)fr[a];
  }
  bool reach;
  V3 rate = {0.0, 0.0, 0.0};
  if constexpr (ACT) {
    const double om[3] = {(double)xb[6], (double)xb[7], (double)xb[8]};
    const double sv[3] = {s0x, s0y, 0.0};
    double wxr[3], vr[3], qr[4];
    cross3(om, pw, wxr);
#pragma unroll
    for (int a = 0; a < 3; ++a) vr[a] = (sv[a] - (double)xb[9 + a]) - wxr[a];
    reach = leg_joints<true, true>(geo, l, R, pw, fl, ql, tl, vr, qr);
    rate = {qr[0], qr[1], qr[2]};
  } else {
    reach = leg_joints<true>(geo, l, R, pw, fl, ql, tl);
  }
  double pf[3], J[9];
  leg_fk_jac(geo, l, ql, pf, J);
  const V3 fv = {fl[0], fl[1], fl[2]}, tc = {tl[0], tl[1], tl[2]}, q = {ql[0], ql[1], ql[2]}, zero = {0.0, 0.0, 0.0};
  const double mu = (double)ground[b], me = (double)foot_mass[b];
  V3 ta, f1;
  unsigned bits = drive_force<ACT>(R, J, reach, fv, tc, lim, drive == DRIVE_LIMITED, ta, f1, ACT ? act + ACT_ROW * b : nullptr, rate);
  double sx, sy, dx, dy;
  bool sliding;
  const V3 f2 = slip_slide(f1, s0x, s0y, mu, me, n, h, delta, sx, sy, dx, dy, sliding);
  const bool changed = f2.x != f1.x || f2.y != f1.y || f2.z != f1.z;   // the ground changed the force
  const V3 fo = sel3(changed, f2, f1);   // (a select: an untouched force keeps its bits, a -0 included)
  const V3 to = drive_torque(R, J, f2, changed, ta);
  bits |= (changed ? 32u : 0u) | (sliding ? SLIP_SLIDING : 0u) | swing_limits(lim, q, zero);   // 4: q outside its limits
  // the robot's x, ground and foot-mass rows poison its four legs, a leg's own operands that leg (in the kernel: see mpcqp_stance_drive_kernel)
  bool robot = isfinite(mu) && mu >= 0.0 && isfinite(me) && me > 0.0;
#pragma unroll
  for (int a = 0; a < 12; ++a) robot = robot && isfinite((double)xb[a]);
  const bool own = fin3(fv) && isfinite(pw[0]) && isfinite(pw[1]) && isfinite(pw[2]) && isfinite(s0x) && isfinite(s0y) && fin3(fo) &&
                   fin3(to) && isfinite(sx) && isfinite(sy) && isfinite(dx) && isfinite(dy);
  const bool good = robot && (!stance || own);
  if (slog) {
    double* sw = slog + b * sstride + 2 * l;
    sw[0] = s0x; sw[1] = s0y;
  }
  drive_store(i, b, l, fr, good, stance, fo, to, bits, f_out, tau, flag, cmd, cstride);
  // a swing leg's foot is in the air, at rest for the rule
  const double nan = __builtin_nan("");
  if (slip_out) {
    slip_out[2 * i] = good ? (stance ? sx : 0.0) : nan;
    slip_out[2 * i + 1] = good ? (stance ? sy : 0.0) : nan;
  }
  if (disp) {
    disp[2 * i] = good ? (TIO)(stance ? dx : 0.0) : (TIO)nan;
    disp[2 * i + 1] = good ? (TIO)(stance ? dy : 0.0) : (TIO)nan;
  }
}

// After the landing of tick `it` (tick is the new one): i = 4 b + leg.  rtau [B,4,3], rflag [B,4] and rdisp [B,4,2] are what
// mpcqp_stance_slip_kernel left for this tick.  The log step is drive_log_step (mpcqp_drive.h) with bit 128 in its mask: a swing row
// keeps what the legs step logged, and so does a stance row the legs step poisoned.  Then the feet: a leg in stance on the row's tick
// that does not touch down on the new one moves by the displacement as the I/O type holds it (z is never touched); a leg that touches
// down is at rest.
template <typename TIO>
__global__ void __launch_bounds__(256)
mpcqp_slip_finish_kernel(const int32_t* __restrict__ gait, const int32_t* __restrict__ tick, const TIO* __restrict__ rtau,
                         const uint8_t* __restrict__ rflag, const TIO* __restrict__ rdisp, const int64_t B, const int T, const int it,
                         TIO* __restrict__ feet, double* __restrict__ slip, TIO* __restrict__ tau_log, uint8_t* __restrict__ flag_log,
                         TIO* __restrict__ disp_log) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * B) return;
  const int64_t b = i / 4;
  const int l = (int)(i % 4);
  // the clock the advance landed on, as mpcqp_legs_land_kernel reads it, and the row's: one tick back, clamped at 0
  const int32_t tn = tick[b];
  const uint32_t tc = (tn > 0 || tn == INT32_MIN) ? (uint32_t)tn : 0u;
  const uint32_t tr = tc > 0u ? tc - 1u : 0u;
  const GaitLeg gc = gait_leg(gait + b * GAIT_ROW, l);
  const bool stance = gait_phase(gc, tr) < gc.st;
  const bool td = gait_steps(gc) && gait_phase(gc, tc) == 0;
  const int64_t il = 4 * (b * T + it) + l;
  if (stance) drive_log_step(i, il, rtau, rflag, SLIP_BITS, false, tau_log, flag_log);
  const bool move = stance && !td;
  const TIO dx = rdisp[2 * i], dy = rdisp[2 * i + 1];
  if (move) {
    feet[3 * i] = (TIO)((double)feet[3 * i] + (double)dx);
    feet[3 * i + 1] = (TIO)((double)feet[3 * i + 1] + (double)dy);
  }
  if (td) { slip[2 * i] = 0.0; slip[2 * i + 1] = 0.0; }
  if (disp_log) {
    disp_log[2 * il] = move ? dx : (TIO)0.0;
    disp_log[2 * il + 1] = move ? dy : (TIO)0.0;
  }
}

}  // namespace
