/*
 * mpcqp_sim.h -- extension of include/mpcqp.h: a rigid-body plant for the device roll-out.
 *
 * mpcqp_rollout advances each robot by the MPC's own prediction (x <- X[:,1]), so its closed loop never meets an error the
 * controller did not predict.  The plant here is the single rigid body with massless legs that the MPC assumes, without the
 * MPC's simplifications (rotation linearised about yaw, no gyroscopic term, lever arms frozen per stage, one forward-Euler step
 * over delta), with per-robot mass and inertia that may differ from the model and with external pushes.
 *
 * The symbols declared here are exported by the product library libmpcqp.so ONLY; the CPU checker library under oracle/ does
 * not have them (the host-side counterpart is plant.srb_step / plant.rollout_plant_host in the Python package).  Pointers are
 * device memory on the handle's GPU, T is the handle's I/O dtype (MpcQpConfig.dtype), work is enqueued on `stream` and nothing is
 * synchronised.  The arithmetic is fp64 whatever T is: fp32 outputs are the fp64 results rounded once.  Return codes and
 * mpcqp_last_error() as in mpcqp.h: sizes, null pointers and `substeps` are checked on the host (MPCQP_EINVAL).
 *
 * Conventions:
 *   state    x = [theta (3), p (3), omega (3), v (3), g]: theta the torso rotation vector (|theta| <= pi), p the CoM, omega the
 *            angular velocity in world coordinates, v the CoM velocity, g = x[12] the gravity (negative), carried unchanged and
 *            used as the plant's gravity.
 *   body     body[b] = (m, Ixx, Iyy, Izz, Ixy, Ixz, Iyz): mass and inertia in the torso frame about the CoM.  NULL means the
 *            handle's model: MpcQpConfig.m and diag(1 / Ibody_inv).  A row with a non-finite entry, m <= 0 or an inertia that is
 *            not positive definite (Sylvester: Ixx > 0, Ixx Iyy - Ixy^2 > 0, det > 0) writes NaN into x[0..11] of that robot
 *            (x[12] is kept); inside mpcqp_rollout_plant the solve then reports MPCQP_STATUS_NONFINITE for it from the next tick
 *            on.  Other robots are unaffected.
 *   dynamics over one tick of length MpcQpConfig.delta, forces held (zero-order hold), stance legs only (contact != 0; a swing
 *            leg's force and foot are ignored):
 *              m v'     = sum f_l + m g e_z + F_push                     p' = v
 *              I_w w'   = sum (foot_l - p) x f_l + tau_push - w x (I_w w),  I_w = R I_b R^T
 *              R'       = [w]x R
 *   integration  unit quaternion q = (w, x, y, z), q' = 1/2 (0, omega) (x) q, classical RK4 with h = delta / substeps, q
 *            renormalised after every substep.  theta -> q at the start of the tick, q -> theta (w >= 0, so |theta| <= pi) at
 *            the end; both conversions use a series below an angle of 1e-3 (exact in the limit 0) and atan2 near pi.
 *            substeps = 0 means 10; substeps < 0 or > 1000 is MPCQP_EINVAL.
 *   wrench   push / wrench rows are (F_x, F_y, F_z, tau_x, tau_y, tau_z): a world-frame force (N) at the CoM and a world-frame
 *            torque about the CoM (N m).
 */
#ifndef MPCQP_SIM_H_
#define MPCQP_SIM_H_

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * One control period of the plant for B robots.
 *   x        T  [B,13]   state
 *   f        T  [B,12]   foot forces FL, FR, HL, HR (world frame, N), held over the tick
 *   feet     T  [B,4,3]  foot positions (world), fixed over the tick
 *   contact  u8 [B,4]    nonzero = stance
 *   body     T  [B,7]    or NULL (the handle's model)
 *   wrench   T  [B,6]    or NULL (no push)
 *   x_out    T  [B,13]   out; may equal x
 */
int mpcqp_plant_step(mpcqp_handle h, int64_t B, const void* x, const void* f, const void* feet, const uint8_t* contact,
                     const void* body, const void* wrench, int32_t substeps, void* x_out, void* stream);

/*
 * mpcqp_rollout with the world step replaced by the plant.  Every other argument, log row and in / out rule is as in
 * mpcqp_rollout: per tick the expand kernel and the solve (warm-started when the handle has the warm-start flags) run unchanged,
 * then one advance launch logs actual / desired / forces / solved, steps the plant, rolls `ref` forward and advances `tick`.
 * No host synchronisation happens inside the T ticks.
 *   feet        stance feet stand at plan_pos[step] of the robot's current step and stay fixed over the tick; stance / swing is
 *               the expand kernel's rule for stage 0 (tin < ss ? plan_feet_id : 1; past the plan, the last step, all stance)
 *   forces      the stage-0 forces of the solve, applied as returned whatever the status
 *   body        T  [B,7] or NULL, as in mpcqp_plant_step
 *   push        T  [B,6] or NULL: the wrench of robot b acts on the ticks push_ticks[b][0] <= tick[b] < push_ticks[b][1],
 *               counted on the robot's own tick
 *   push_ticks  i32[B,2]; required when push is given (MPCQP_EINVAL otherwise), ignored when push is NULL
 */
int mpcqp_rollout_plant(mpcqp_handle h, int64_t B, int32_t T, int32_t S, void* x, void* ref, const void* plan_pos,
                        const uint8_t* plan_feet_id, const int32_t* plan_meta, int32_t* tick, const void* mu, const void* body,
                        const void* push, const int32_t* push_ticks, int32_t substeps, void* actual, void* desired, void* forces,
                        int32_t* solved, void* stream);

/*
 * mpcqp_rollout_plant with the plan table replaced by a per-leg gait clock and each robot's feet carried as state (gait row, clock and
 * foothold rule: include/mpcqp_plan.h, mpcqp_phase_expand).  Per tick: the phase expand, the unchanged solve and one advance launch;
 * three launches, no host synchronisation and no allocation after mpcqp_reserve.  The advance, per robot and in this order:
 *   1. logs actual / desired / forces / solved as mpcqp_rollout does (desired is never gated: a gait has no last step)
 *   2. logs feet_log and contact_log: the feet and the stance mask the plant uses this tick
 *   3. steps the plant under the stage-0 forces with the held feet and the clock's stance mask (no stance leg: a ballistic tick)
 *   4. rolls `ref` forward (com += v_ref delta, yaw += theta_dot delta) and advances `tick`
 *   5. for every leg that touches down at the NEW tick writes feet[b][l] from the foothold rule at the MEASURED post-step state as it
 *      is stored in x: c the CoM, v the velocity, psi = atan2(R10, R00) of the rotation the plant's rotation-vector conversion gives.
 *      Every other foot is left bit-for-bit alone.
 *   feet         T  [B,4,3]   in / out: the feet each robot holds (world).  A swing leg's entry is its lift-off foot until it lands.
 *   gait         i32[B,9]     stand  T [B,4,3]     gain  T [B] or NULL
 *   feet_log     T  [B,T,4,3] out, may be NULL.  A swing leg's row is its lift-off foot (contact_log tells which legs swing):
 *                             mpcqp_phase_swing (mpcqp_plan.h) turns these logs into swing trajectories, and its feet_des, not
 *                             feet_log, is the operand mpcqp_joint_log and mpcqp_joint_rates want.
 *   contact_log  u8 [B,T,4]   out, may be NULL
 *   x, ref, tick, mu, body, push, push_ticks, substeps, actual, desired, forces, solved   as in mpcqp_rollout_plant
 * What is reactive: where a foot lands (step 5 reads the measured state).  What is not: when it lands (the clock is open-loop), the
 * footholds the horizon previews for later touchdowns (reference pose, measured velocity) and the height of the ground.
 * A non-finite feet, stand or gain row: that robot's solves report MPCQP_STATUS_NONFINITE; no other robot changes.
 * MPCQP_EINVAL: B or T negative, B * T > 2^31 - 1, substeps outside [0, 1000], push without push_ticks, a null required buffer.
 * B = 0 or T = 0 is a no-op.
 */
int mpcqp_rollout_phase(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, const int32_t* gait, const void* stand,
                        const void* gain, int32_t* tick, const void* mu, const void* body, const void* push, const int32_t* push_ticks,
                        int32_t substeps, void* actual, void* desired, void* forces, void* feet_log, uint8_t* contact_log,
                        int32_t* solved, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_SIM_H_ */
