/*
 * mpcqp_plan.h -- extension of include/mpcqp.h: footstep plans and swing-foot trajectories on the device.
 *
 * These are the pieces of the per-tick glue that sit around the QP.  Two are the reference's: the footstep planner
 * (FootstepPlanner.__init__, src/footstep_planner.py:29-177) and the swing-foot trajectory generator
 * (FootTrajectoryGenerator.generate_feet_trajectories_at_time, src/foot_trajectory_generator.py:27-96), batched over B robots.
 * mpcqp_plan_footsteps writes the plan tables that mpcqp_rollout reads, so a batch of roll-outs is set up without a host loop.
 *
 * The symbols declared here are exported by the product library libmpcqp.so ONLY; the CPU checker library under oracle/ does
 * not have them (its host-side counterparts are footstep_planner.plan_tables / foot_trajectory_generator.swing_tables in the
 * Python package).  Pointers are device memory on the handle's GPU, T is the handle's I/O dtype (MpcQpConfig.dtype), work is
 * enqueued on `stream` and nothing is synchronised.  Both calls carry their arithmetic in fp64 whatever T is: fp32 outputs are
 * the fp64 results rounded once.  A handle serves one stream at a time (include/mpcqp.h): mpcqp_plan_footsteps uses an
 * engine-owned workspace of B * S * 40 bytes, allocated by the first call at a given size and reused afterwards.
 * Return codes and mpcqp_last_error() as in mpcqp.h: sizes and null pointers are checked on the host (MPCQP_EINVAL).
 */
#ifndef MPCQP_PLAN_H_
#define MPCQP_PLAN_H_

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Footstep plan of src/footstep_planner.py:29-177 for B robots, in the table form mpcqp_rollout reads.
 *   feet0        T  [B,4,3]   initial foot positions FL, FR, HL, HR (initial_configuration[leg])
 *   cmd          T  [B,5]     yaw0, v_com_ref x, v_com_ref y, theta_dot, h
 *   gait         i32[B,4]     total_steps, ss_duration, ds_duration, first_swing as a bit mask (bit k = leg k stays down in step 1)
 *   plan_pos     T  [B,S,4,3] out: plan[step]['pos'] of the four feet
 *   plan_feet_id u8 [B,S,4]   out: plan[step]['feet_id'] (1 = stance)
 *   plan_meta    i32[B,4]     out: min(steps, S), ss, ds, 0 (steps = total_steps, or the 100 standing steps when total_steps <= 0)
 *   plan_ang     T  [B,S]     out, may be NULL: yaw of each step
 *   plan_hip     T  [B,S,3]   out, may be NULL: the planner's 'hip' row (x/y NaN for a standing plan, as the host)
 * The tick length is MpcQpConfig.delta (the reference's world_time_step).  The planner's rules: step 0 is all stance; the
 * unicycle (theta += theta_dot dt, centre += R(theta) v dt, ss + ds ticks per step) moves from the second step on; the feet that
 * stay down keep their previous row, the others land on the fresh placement around the centre; first_swing alternates with its
 * complement from step to step.  Rows s >= min(steps, S) repeat the last planned row.  The gait row lives in device memory and
 * is clamped, never trusted: total_steps < 0 means the standing plan, ss and ds are clamped into [0, 65535].
 */
int mpcqp_plan_footsteps(mpcqp_handle h, int64_t B, int32_t S, const void* feet0, const void* cmd, const int32_t* gait,
                         void* plan_pos, uint8_t* plan_feet_id, int32_t* plan_meta, void* plan_ang, void* plan_hip, void* stream);

/*
 * FootTrajectoryGenerator.generate_feet_trajectories_at_time for every leg at ticks tick[b] + j, j = 0..K-1.
 *   plan_pos / plan_feet_id / plan_meta / plan_ang   as written by mpcqp_plan_footsteps ([B,S,...]; plan_ang is required)
 *   tick        i32[B]          first tick of each robot (clamped at >= 0)
 *   step_height T  [B]
 *   traj        T  [B,K,4,3,6]  out: pos / vel / acc 6-vectors (angle xyz, position xyz) of each leg
 *   feet_des    T  [B,K,4,3]    out, may be NULL: the desired foot position of the reference's closed-loop log
 *                               (FEET POS des, src/main.py:152-167)
 * Step of tick tau: s = min(tau / (ss + ds), S_b - 1), t = tau - s (ss + ds); the target past the last row is the start; step 0
 * stands; the swing lands at 0.8 ss (cubic in x / y / angle, quartic bump of step_height in z); velocity and acceleration are
 * divided by delta and delta^2.  plan_meta is clamped as in mpcqp_rollout (1 <= S_b <= S, ss, ds >= 0, ss + ds >= 1).
 *
 * The host generator marks a step all-stance (plan[step]['feet_id'] = 1) when it is queried in double support
 * (src/foot_trajectory_generator.py:53-54).  These functions never write the plan; feet_des is the pure rule that reproduces
 * what that side effect does to the log of a closed loop that has queried every tick from 0:
 *   stance leg (plan_feet_id[s] == 1)                   plan_pos[s]
 *   swing leg, single support (t < ss)                  trajectory position, z clamped at >= 0
 *   swing leg, first double-support tick (t == ss)      the target plan_pos[s + 1] (past the plan: plan_pos[s]), z clamped at >= 0
 *   swing leg, later double-support ticks (t > ss)      plan_pos[s]
 * (Step 0 returns before the side effect in the host generator: a swing leg there, which only a hand-made table can have, keeps
 * the trajectory position, i.e. the start, at every tick.)  Stance is any nonzero plan_feet_id.
 */
int mpcqp_swing_trajectories(mpcqp_handle h, int64_t B, int32_t K, int32_t S, const void* plan_pos, const uint8_t* plan_feet_id,
                             const int32_t* plan_meta, const void* plan_ang, const int32_t* tick, const void* step_height,
                             void* traj, void* feet_des, void* stream);

/*
 * Per-leg periodic gaits with reactive footholds: a phase clock per leg in place of a plan table.
 *
 * Gait row   gait i32[B,9] = (P, offset[4], stance[4]) in ticks, legs FL, FR, HL, HR.  Leg l is in stance at tick t >= 0 when
 *            phi_l(t) = (t + offset_l) mod P < stance_l, and touches down at t exactly when 0 < stance_l < P and phi_l(t) = 0.
 *            stance = P is a leg that never lifts, stance = 0 one that never lands; neither has a touchdown.  The row lives in device
 *            memory and is clamped, never trusted: P into [1, 65535], offset reduced into [0, P) (a negative one to its non-negative
 *            residue), stance into [0, P], a negative tick to 0; t + offset is formed in unsigned 32 bits, which it cannot overflow.
 * Foothold   of a touchdown of leg l, from a CoM c, a yaw psi, a velocity v, the reference velocity v_ref = ref[6..8] and the stance
 *            time Ts = stance_l delta:
 *              p_xy = c_xy + Rz(psi) stand_xy[l] + (Ts / 2) v_ref_xy + gain (v_xy - v_ref_xy),    p_z = stand_z[l]
 *   stand    T  [B,4,3]  nominal foot of each leg relative to the CoM in the yaw frame (x, y); the third entry is the WORLD z of the
 *                        ground under that foot
 *   gain     T  [B]      velocity feedback in seconds, or NULL for 0
 * All arithmetic is fp64 whatever T is; fp32 outputs are the fp64 results rounded once.
 *
 * mpcqp_phase_expand turns (x0, ref, feet, gait, tick, stand, gain) into a caller-owned operator tuple:
 *   x0       T  [B,13]     measured state                     ref   T  [B,10]  roll, pitch, yaw, com (3), v_ref (3), theta_dot
 *   feet     T  [B,4,3]    the feet the robot holds (world)   tick  i32[B]     tick of stage 0
 *   r        T  [B,N,4,3]  out                                contact u8[B,N,4] out     xdes  T [B,N+1,13]  out
 * xdes is that of mpcqp_solve_batch_gait (never gated); contact[k][l] is the clock at tick + k.  The foothold of (k, l) belongs to the
 * leg's last touchdown, at stage j = k - phi_l(tick + k): if 0 < stance_l < P and j >= 1 it is the rule at the REFERENCE pose of
 * stage j (c = ref com + j delta v_ref, psi = ref yaw + j delta theta_dot) with the measured velocity v = x0[9..11]; otherwise it is
 * the held foot feet[b][l].  The lever arm is foothold - com with the measured com at stage 0 and the reference's from stage 1 on.
 * A swing leg gets the same rule (its force is pinned to 0 by the solve).  A non-finite stand or gain row makes the stage-0
 * lever arms of that robot non-finite whatever its clock, and a non-finite held foot its own lever arms, so the robot's solve reports
 * MPCQP_STATUS_NONFINITE; no other robot changes.
 */
int mpcqp_phase_expand(mpcqp_handle h, int64_t B, const void* x0, const void* ref, const void* feet, const int32_t* gait,
                       const int32_t* tick, const void* stand, const void* gain, void* r, uint8_t* contact, void* xdes, void* stream);

/*
 * mpcqp_phase_expand into the engine's tuple workspace, then the solve exactly as mpcqp_solve_batch does it on that tuple: outputs,
 * warm-start flags, model rows and mpcqp_last_kernel_ms (expand + solve) as there.  Any horizon, both engines.
 */
int mpcqp_solve_batch_phase(mpcqp_handle h, int64_t B, const void* x0, const void* ref, const void* feet, const int32_t* gait,
                            const int32_t* tick, const void* stand, const void* gain, const void* mu, void* u_out, void* X_out,
                            int32_t* status, int32_t* iters, float* res, void* stream);

/*
 * Swing-foot trajectories of a roll-out on a gait clock, from its logs: what mpcqp_swing_trajectories is to the plan table.
 *   actual      T  [B,T,12]     as mpcqp_rollout_phase logs it: rotation vector, CoM, omega, v
 *   desired     T  [B,T,12]     as it logs it; read: [8] the reference yaw rate, [9..11] v_ref
 *   feet_log    T  [B,T,4,3]    as it logs it: the feet the plant used each tick; a swing leg's row is its lift-off foot
 *   gait        i32[B,9]        the roll-out's gait rows, clamped as above
 *   tick0       i32[B]          the value `tick` had BEFORE the roll-out.  The roll-out advances `tick` in place, so the caller keeps a
 *                               copy.  Row t is tick max(tick0 + t, 0), as the roll-out's advance clamps it (a negative start tick holds
 *                               the clock at 0); the sum saturates at 2^31 - 1.
 *   stand, gain                 the roll-out's rows (gain may be NULL)
 *   step_height T  [B]          apex of the swing above the straight line from lift-off to target
 *   swing       T  [B,T,4,4,3]  out: per (robot, row, leg) the four 3-vectors pos, vel, acc, target
 *   feet_des    T  [B,T,4,3]    out, may be NULL: pos -- the `feet` operand of mpcqp_joint_log / mpcqp_joint_rates
 * A pure function of one log row per (robot, row, leg).  phi = phi_l(tick of the row).  The leg swings when 0 < stance_l < P and
 * phi >= stance_l; then with n = P - stance_l, s = (phi - stance_l) / n in [0, 1), rem = P - phi ticks to touchdown, T_sw = n delta:
 *   p0      = feet_log[b,t,l], the lift-off foot
 *   p1      = the foothold rule at the touchdown predicted from the row: c_xy = com_xy + (rem delta) v_xy,
 *             psi = measured yaw + (rem delta) desired[8], v the measured velocity, v_ref = desired[9..11], Ts = stance_l delta;
 *             p1_z = stand_z.  The measured yaw is atan2(R10, R00) of the plant's rotation-vector conversion, as the roll-out reads it.
 *             With rem = 0 this is, term for term, the foothold the roll-out writes at the landing.
 *   pos     = p0 + b(s) (p1 - p0) + z_b(s) e_z,     b(s) = 3 s^2 - 2 s^3,   z_b(s) = 16 step_height s^2 (1 - s)^2
 *   vel     = [b'(s) (p1 - p0) + z_b'(s) e_z] / T_sw,     acc = [b''(s) (p1 - p0) + z_b''(s) e_z] / T_sw^2
 *   target  = p1
 * The target moves from row to row with the measured state; vel and acc hold it frozen (they are the derivatives of the row's own
 * curve, not differences between rows).  A stance leg, and a leg without touchdowns (stance = 0 or stance = P), has
 * pos = target = its feet_log row bit for bit and vel = acc = 0.  A non-finite stand, gain or step_height row makes every output of
 * that robot NaN, a non-finite actual row or desired[8..10] every output of that (robot, row), a non-finite foot its own leg's; no
 * other robot, row or leg changes.  B = 0 or T = 0 is a no-op; B or T negative, B T > 0x7fffffff or a null required buffer is
 * MPCQP_EINVAL.
 */
int mpcqp_phase_swing(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* desired, const void* feet_log,
                      const int32_t* gait, const int32_t* tick0, const void* stand, const void* gain, const void* step_height,
                      void* swing, void* feet_des, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_PLAN_H_ */
