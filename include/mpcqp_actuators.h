/*
 * mpcqp_actuators.h -- extension of include/mpcqp_joints.h and mpcqp_sim.h: per-robot actuator rows with a torque-speed curve.
 *
 * Every joint-torque clamp of the leg roll-outs reads the one tau_max of the call's MpcQpLegInertia row, a flat box whatever the
 * joint's rate.  An actuator table gives robot b its own standstill torque and, per joint, a rate up to which that torque is
 * available and a no-load rate at which the motoring torque has fallen to zero: a strength sweep, or a batch of different motors, in
 * one call, and a swing leg that runs out of torque where a real one does -- at speed.
 *
 * The symbols declared here are exported by the product library libmpcqp.so ONLY; the CPU checker library under oracle/ does not
 * have them (the host-side counterpart is the `actuators` argument of lite3_model.swing_track_host / stance_drive_host /
 * leg_effort_host and gaits.rollout_legs_host / rollout_drive_host in the Python package; actuators.py has the row helpers).
 * Return codes and mpcqp_last_error() as in mpcqp.h.
 *
 * Row layout: act[b] = (tau_max[3], qd_knee[3], qd_free[3]) for HipX, HipY, Knee, nine doubles, fp64 WHATEVER the handle's I/O
 * dtype, for the reason mpcqp_model.h gives: the table is small and set once, and fp64 lets a row reproduce the inertia row's
 * tau_max exactly.  tau_max [N m] is the torque at standstill, qd_knee [rad/s] the rate up to which the full torque is available,
 * qd_free [rad/s] the no-load rate.
 *
 * The envelope, for one joint with commanded torque t and rate r, a = |r|:
 *
 *   avail = a > qd_knee ? tau_max * (max(qd_free - a, 0) / (qd_free - qd_knee)) : tau_max
 *   hi    = r > 0 ?  avail :  tau_max
 *   lo    = r < 0 ? -avail : -tau_max
 *   app   = t > hi ? hi : (t < lo ? lo : t)          (a NaN stays)
 *
 * in fp64, in this order, without contraction; the masks are selects.  A braking joint (t r < 0) keeps the full tau_max, only the
 * motoring side falls off.  qd_knee = +inf with any qd_free is the flat box: it gives, bit for bit, the clamp at +-tau_max that the
 * calls apply without a table, so a table of such rows with the inertia row's tau_max is no table.
 *
 * A row is valid when every tau_max is finite and >= 0, every qd_knee >= 0, and each joint has either qd_knee = +inf or a finite
 * qd_knee and a finite qd_free > qd_knee.  An invalid row is kept as NaN and poisons what reads it; no other robot changes (the
 * `body` rule of mpcqp_sim.h): the robot's swing rows log NaN and flag 0xff (and the landing row that ends such a swing), its stance
 * legs under MPCQP_DRIVE_LIMITED get NaN applied forces and torques and flag 0xff -- in a roll-out the plant then carries the NaN
 * into x, and the robot's solves report MPCQP_STATUS_NONFINITE from the next tick on --, and mpcqp_leg_effort writes limit = 0xff.
 *
 * The invalid row inside a roll-out, by entry point and landing (tests/test_gpu_actuator_rows.py holds each clause against the run with
 * the row mended; "a leg log" is q_log, qd_log, tau_log, foot_log, err_log):
 *   mpcqp_rollout_legs, and mpcqp_rollout_drive under MPCQP_DRIVE_IDEAL (with ground = NULL), MPCQP_LAND_RULE
 *                          the legs feed nothing back: x, ref, feet, tick, the six logs of mpcqp_rollout_phase, swing_log and solved
 *                          are the mended run's, bit for bit.  flag_log is 0xff and every leg log NaN on the robot's swing rows and
 *                          on the stance row that follows a swing row of the same leg, the landing row, and on no other row; the
 *                          other rows keep the mended run's values.  miss_log is NaN on its landings.
 *   the same two, MPCQP_LAND_ACTUAL
 *                          up to the first landing as above.  That landing writes a NaN foot into feet; the solve of the landing
 *                          tick reports MPCQP_STATUS_NONFINITE, its row is 0xff / NaN on all four legs, and the plant carries the NaN
 *                          into x: from the tick after it `actual` is non-finite and every row is 0xff / NaN.  solved counts the
 *                          ticks before the first landing.
 *   mpcqp_rollout_drive under MPCQP_DRIVE_LIMITED (the test runs it with MPCQP_LAND_ACTUAL)
 *                          the stance rule poisons the first tick: every row, stance and swing, is 0xff / NaN from tick 0, cmd of
 *                          tick 0 is finite, `actual` is non-finite from tick 1 and solved is 1.
 * In every one of them every other robot's state and logs are the mended run's, bit for bit.
 *
 * Which rate enters the envelope:
 *   swing control period   (mpcqp_swing_track; the legs step of mpcqp_rollout_legs / mpcqp_rollout_drive) the leg state's qd at the
 *                          start of that control period, the one the commanded torque was formed from
 *   stance rule            (mpcqp_stance_drive, and inside mpcqp_rollout_drive; step 2 of the rule in mpcqp_sim.h) mpcqp_joint_rates'
 *                          rate with the foot at rest in the world, J^-1 R^T (-v - omega x (foot - c)) from x[6..11] as stored; out
 *                          of reach or det J = 0 gives a rate of 0 and with it the full tau_max.  MPCQP_DRIVE_IDEAL skips step 2 and
 *                          does not read the table.
 *   mpcqp_leg_effort       limit bit 4 is set when tau_j > hi_j or tau_j < lo_j at the row's qd_j
 * The flag bits keep their meaning: bit 2 is set when app != cmd on any joint.  q_min, q_max, qd_max and the bits they decide stay
 * the inertia row's.  Not built: per-robot joint stops and rate limits, regenerative or thermal limits.  The MPC is not told: a
 * controller that should know lowers f_max through mpcqp_set_models.
 */
#ifndef MPCQP_ACTUATORS_H_
#define MPCQP_ACTUATORS_H_

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Sets the handle's actuator table to the B rows at `act` (device memory on the handle's GPU, fp64 [B,9]).  One conversion kernel
 * validates and copies the rows on `stream` into a table the engine owns (grown as mpcqp_set_models grows its own: a call at a larger
 * B than any before allocates, which synchronises the device); the caller's buffer is free again once that kernel has run, and calls
 * enqueued on the same stream afterwards see the new rows.  A call on ANOTHER stream must be ordered after `stream` by the caller.
 *
 * While a table is set, mpcqp_swing_track, mpcqp_leg_effort (mpcqp_joints.h), mpcqp_stance_drive, mpcqp_rollout_legs and
 * mpcqp_rollout_drive (mpcqp_sim.h) read row b for robot b, and the tau_max of their `inr` argument is ignored.  A call of one of
 * them with a B other than the table's returns MPCQP_EINVAL (the message names the entry point and both sizes).  The B of
 * mpcqp_stance_drive is its row count: on the B T logged rows of a roll-out it needs the table tiled, row b repeated T times.
 *
 * MPCQP_EINVAL for B <= 0 or a null `act`, MPCQP_ENOMEM when the table cannot be grown; the table set before, if any, then stays.
 */
int mpcqp_set_actuators(mpcqp_handle h, int64_t B, const double* act, void* stream);

/*
 * Back to the inertia row's tau_max for every clamp.  The allocation is kept.  The call has no stream: it waits for the device (the
 * calls enqueued so far finish with the table), then every later one runs without it.
 */
int mpcqp_clear_actuators(mpcqp_handle h);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_ACTUATORS_H_ */
