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
 *            torque about the CoM (N m).  The plant's push is not told to the MPC; rows of the same layout that are, and an observer
 *            that estimates them from a roll-out's logs, are mpcqp_disturb.h.
 */
#ifndef MPCQP_SIM_H_
#define MPCQP_SIM_H_

#include "mpcqp.h"
#include "mpcqp_joints.h"   /* MpcQpLegInertia, for mpcqp_rollout_legs */

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

/*
 * mpcqp_rollout_phase with the swing legs integrated inside the roll-out, tick by tick: a leg state per (robot, leg) is carried next to
 * x, ref, feet and tick, and a foot that touches down may land where its leg put it instead of on the foothold rule.  Every argument of
 * mpcqp_rollout_phase keeps its meaning.  (A product library built before this call has the header's other three; the Python binding
 * tells the two apart.)
 *   legs         double [B,4,7]  in / out, required: per leg q (3), qd (3) and live, in the layout and with the `live` semantics of
 *                                mpcqp_swing_track's `state` (include/mpcqp_joints.h).  fp64 whatever the I/O dtype: a state that passes
 *                                through memory every tick must not be rounded to float32 on the way (mpcqp_set_models' rows are doubles
 *                                for the same reason).  All zeros: every leg starts from its row.
 *   step_height  T [B]           as for mpcqp_phase_swing
 *   gains        T [B,2] or NULL, leg_substeps, geo, inr   as `gains`, `substeps`, `geo`, `inr` of mpcqp_swing_track: leg_substeps = 0
 *                                means control periods of 2 ms, a value below 0 or above 1000 is MPCQP_EINVAL
 *   land         MPCQP_LAND_RULE or MPCQP_LAND_ACTUAL; anything else is MPCQP_EINVAL
 *   logs, each may be NULL:
 *   swing_log    T  [B,T,4,4,3]  pos / vel / acc / target, as mpcqp_phase_swing's `swing`
 *   q_log, qd_log, tau_log, foot_log   T [B,T,4,3],  err_log T [B,T,4],  flag_log u8 [B,T,4]: mpcqp_swing_track's outputs, with its
 *                                per-row meaning and flag bits
 *   miss_log     T  [B,T,4]      the landing miss of a leg that touches down at the tick after row t; 0 for every other leg
 * Per tick, in this order:
 *   1. the phase expand and the solve, unchanged
 *   2. the legs step, one lane per (robot, leg).  It forms the row mpcqp_swing_track would read at this tick from the live buffers:
 *      actual = x[0..11], forces = the solve's stage-0 forces, the held foot = feet, the stance mask from the gait clock at
 *      max(tick, 0), swing = mpcqp_phase_swing's rule at this row with desired[8] = ref[9] and desired[9..11] = ref[6..8], as the I/O
 *      dtype holds it.  Then exactly what mpcqp_swing_track does with a row -- landing / lift-off re-initialisation, the per-row
 *      outputs, the leg_substeps control periods on a swing row -- and the state goes back to `legs`.  The torso's acceleration over
 *      the tick is the plant's right-hand side at the row WITH the robot's push where its window is open:
 *        a = (sum f + F_push) / m + g e_z,   alpha = I_w^-1 (sum r x f + tau_push - omega x I_w omega)
 *      (the roll-out knows the push; mpcqp_swing_track has to be told through base_acc), formed in fp64 and, like the swing row, held
 *      as the I/O dtype would hold it in a base_acc row: with float32 I/O mpcqp_swing_track on the logs, given this right-hand side,
 *      starts every row from the same operands.
 *   3. the advance of mpcqp_rollout_phase, bit for bit: logs, plant step, ref, tick, rule footholds.  Then, for every leg that touches
 *      down at the new tick: p_act = c + R p_foot(q) with q from `legs` and c, R from the post-step state as stored (what
 *      mpcqp_swing_track's landing row calls the miss); miss_log[b,it,l] = |p_act - rule foothold| in 3-D; and with MPCQP_LAND_ACTUAL
 *      feet[b][l] = (p_act.x, p_act.y, stand_z) instead of the rule's xy.
 * Five launches per tick, no host synchronisation, copy or allocation inside the T ticks.
 * Non-finite operands: a non-finite leg state at a landing with MPCQP_LAND_ACTUAL writes a NaN foot; that robot's solves then report
 * MPCQP_STATUS_NONFINITE and no other robot changes.  A bad gains or step_height row poisons its robot's legs the same way (leg logs NaN,
 * flag 0xff).  With MPCQP_LAND_RULE a poisoned leg never reaches x or feet: x, ref, feet, tick and the six logs of mpcqp_rollout_phase
 * are then bit for bit what mpcqp_rollout_phase gives.
 * MPCQP_EINVAL: as mpcqp_rollout_phase, and a null legs or step_height, leg_substeps or land out of range, an invalid geo / inr row.
 * Not built: the legs' reaction on the torso (the body's mass already contains the legs: hip forces added naively would count their
 * weight twice), joint stops, swing-foot ground contact and early / late touchdown (the clock stays open-loop), a variant on plan
 * tables.
 */
#define MPCQP_LAND_RULE 0
#define MPCQP_LAND_ACTUAL 1
int mpcqp_rollout_legs(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                       const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                       const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains, int32_t leg_substeps,
                       const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, void* actual, void* desired, void* forces,
                       void* feet_log, uint8_t* contact_log, int32_t* solved, void* swing_log, void* q_log, void* qd_log, void* tau_log,
                       void* foot_log, void* err_log, uint8_t* flag_log, void* miss_log, void* stream);

/*
 * The score row of a roll-out: one HIP reduction over the logs of mpcqp_rollout / _plant / _phase / _legs into MPCQP_SCORE_FIELDS doubles
 * per robot -- did it fall, how well did it track, what did it cost, how often did its actuators saturate, how far did its feet miss.
 * (A product library built before this call has the header's other four; the Python binding tells the two apart.)
 *   actual, desired, forces   T  [B,T,12]   required, as the roll-outs write them
 *   contact_log               u8 [B,T,4]    required; nonzero = stance (mpcqp_rollout and mpcqp_rollout_plant write none: the caller
 *                                           supplies the mask the plan gave)
 *   tau, qd                   T  [B,T,4,3], flag u8 [B,T,4]   the leg group, mpcqp_swing_track's rows: all three or none
 *   miss                      T  [B,T,4]    or NULL; needs nothing else
 *   rule                      host pointer, NULL = the defaults below
 *   score                     double [B, MPCQP_SCORE_FIELDS], fp64 whatever the I/O dtype: it passes through memory between pieces (the
 *                             reason `legs` is fp64).  accumulate = 0: written fresh, whatever it held.  accumulate != 0: the row in
 *                             `score` is combined with this piece (sums and counts add, maxima take the larger, fall_row keeps the
 *                             first), and this piece's first row has the global index rows + bad_rows of the incoming row: a long
 *                             roll-out is scored piece by piece and its logs need the memory of one piece.
 * A row t of robot b is FALLEN when p_z < z_frac * p_z_des or sqrt(theta_x^2 + theta_y^2) > tilt_max (actual[5], desired[5],
 * actual[0..1]).  The defaults, z_frac = 0.5 and tilt_max = 0.7 rad, are a CONVENTION of this header -- half the commanded height, 40
 * degrees off the vertical -- not a property of the robot or of the plant, which lets a torso sink through the ground; pass the rule a
 * study means.  A fallen row is scored like any other.  A rule that is not finite and positive, or whose size is not the struct's, is
 * MPCQP_EINVAL.
 * A row with a non-finite entry among its 36 values of actual, desired and forces is a BAD row: it counts in bad_rows, it may be the
 * fall_row, and nothing else of it is read -- not its leg rows or misses either -- so a score stays finite.
 * Fields, in this order (all arithmetic fp64; float32 logs convert exactly; maxima and counts start at 0; sums are per row, the time
 * step goes in on the host):
 *   body    ROWS rows scored; BAD_ROWS; FALL_ROW the global index of the first fallen or bad row, -1 if none; Z_SQ sum (p_z - p_z_des)^2,
 *           Z_MAX max |p_z - p_z_des|; VEL_SQ sum |v_xy - v_xy_des|^2, VEL_MAX max |v_xy - v_xy_des|; ANG_SQ sum |theta - theta_des|^2,
 *           ANG_MAX max |theta - theta_des|; TILT_MAX max sqrt(theta_x^2 + theta_y^2); VX_SUM, VY_SUM sum v_x, sum v_y
 *   forces  legs with contact != 0 only.  FZ_MAX max f_z; FRIC_MAX max of max(|f_x|, |f_y|) / f_z over stance legs with f_z > 0: the
 *           pyramid's use, to be read against mu; F_SQ sum |f|^2; STANCE_ROWS + l the stance rows of leg l; FLIGHT_ROWS rows with no
 *           stance leg
 *   legs    0 without the group.  A leg-row whose flag is 0xff (or that holds a non-finite tau or qd, which the roll-outs write only
 *           under that flag) counts in POISONED_ROWS only.  TAU_MAX max |tau_j|; TAU_SQ sum tau_j^2; WORK_POS sum over leg-rows of
 *           max(tau . qd, 0); WORK_ABS sum |tau . qd|; SWING_ROWS, CLAMP_ROWS, QLIM_ROWS, RATE_ROWS, SINGULAR_ROWS leg-rows with flag bit
 *           1, 2, 4, 8, 16
 *   miss    0 without it.  LANDINGS entries with miss != 0; MISS_MAX max miss; MISS_SQ sum miss^2.  A non-finite miss is a landing and is
 *           left out of MISS_MAX and MISS_SQ.
 * One wave per robot, one fixed reduction order: a robot's row does not depend on B, on its slot in the batch or on anything but its
 * own T rows, and the same call gives the same bits.  Nothing is synchronised or allocated.
 * MPCQP_EINVAL: B or T negative, B * T > 2^31 - 1, a null required buffer (B > 0 and T > 0) or a null score (B > 0), a leg group given in
 * part, a float buffer that is not 16-byte aligned or a u8 buffer that is not 4-byte aligned (the rows are read as vectors), a bad rule.
 * B = 0 is a no-op; T = 0 writes the identity row (zeros, FALL_ROW -1) with accumulate = 0 and leaves `score` alone otherwise.
 */
typedef struct MpcQpScoreRule {
  uint32_t size;    /* sizeof(MpcQpScoreRule) */
  double z_frac;    /* fallen: p_z < z_frac * p_z_des; default 0.5 */
  double tilt_max;  /* fallen: sqrt(theta_x^2 + theta_y^2) > tilt_max [rad]; default 0.7 */
} MpcQpScoreRule;
#define MPCQP_SCORE_RULE_Z_FRAC 0.5
#define MPCQP_SCORE_RULE_TILT_MAX 0.7
#define MPCQP_SCORE_ROWS 0
#define MPCQP_SCORE_BAD_ROWS 1
#define MPCQP_SCORE_FALL_ROW 2
#define MPCQP_SCORE_Z_SQ 3
#define MPCQP_SCORE_Z_MAX 4
#define MPCQP_SCORE_VEL_SQ 5
#define MPCQP_SCORE_VEL_MAX 6
#define MPCQP_SCORE_ANG_SQ 7
#define MPCQP_SCORE_ANG_MAX 8
#define MPCQP_SCORE_TILT_MAX 9
#define MPCQP_SCORE_VX_SUM 10
#define MPCQP_SCORE_VY_SUM 11
#define MPCQP_SCORE_FZ_MAX 12
#define MPCQP_SCORE_FRIC_MAX 13
#define MPCQP_SCORE_F_SQ 14
#define MPCQP_SCORE_STANCE_ROWS 15   /* + leg: 15 .. 18 */
#define MPCQP_SCORE_FLIGHT_ROWS 19
#define MPCQP_SCORE_TAU_MAX 20
#define MPCQP_SCORE_TAU_SQ 21
#define MPCQP_SCORE_WORK_POS 22
#define MPCQP_SCORE_WORK_ABS 23
#define MPCQP_SCORE_SWING_ROWS 24
#define MPCQP_SCORE_CLAMP_ROWS 25
#define MPCQP_SCORE_QLIM_ROWS 26
#define MPCQP_SCORE_RATE_ROWS 27
#define MPCQP_SCORE_SINGULAR_ROWS 28
#define MPCQP_SCORE_POISONED_ROWS 29
#define MPCQP_SCORE_LANDINGS 30
#define MPCQP_SCORE_MISS_MAX 31
#define MPCQP_SCORE_MISS_SQ 32
#define MPCQP_SCORE_FIELDS 33
int mpcqp_rollout_score(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* desired, const void* forces,
                        const uint8_t* contact_log, const void* tau, const void* qd, const uint8_t* flag, const void* miss,
                        const MpcQpScoreRule* rule, int32_t accumulate, double* score, void* stream);

/*
 * What a stance leg delivers.  The roll-outs above apply the solve's stage-0 forces as returned: the legs are ideal force sources and
 * the ground transmits anything.  The rule here puts the actuators' torque limit and the ground between the commanded force and the
 * plant; mpcqp_stance_drive is the rule for B robots (it is to the drive what mpcqp_plant_step is to the plant), mpcqp_rollout_drive the
 * roll-out with the rule in its loop.  (A product library built before these two has the header's other five; the Python binding tells
 * them apart.)
 * The rule, for one stance leg (contact != 0) with commanded force f (world), held foot, state x as stored:
 *   1. R from the rotation vector exactly as mpcqp_joint_log forms it; (q, reach) the closed-form IK with rot = R, origin = CoM;
 *      A = (R J(q))^T; tau_cmd = A (-f) -- mpcqp_joint_log's stance torque, from the same device functions.
 *   2. tau_app = tau_cmd clamped per joint into [-tau_max, tau_max] (the inertia row's); the leg is CLAMPED when any joint differs.
 *   3. not clamped: f1 = f (a select: the bits of f are kept).  Clamped, reach = 1 and det J != 0: f1 = -A^-1 tau_app = -R (J^-T tau_app),
 *      J^T solved by cofactors and determinant in the order the rates solve J.  Clamped but out of reach or singular: f1 = f, bit 16.
 *   4. the ground.  f1_z <= 0: f2 = 0, the foot cannot pull.  Otherwise, with a friction row mu_g, if sqrt(f1_x^2 + f1_y^2) > mu_g f1_z the
 *      tangential part is scaled by mu_g f1_z / sqrt(f1_x^2 + f1_y^2): onto the circular Coulomb cone, direction kept.  Otherwise f2 = f1.
 *      Bit 32 is set exactly when f2 != f1.  THE FOOT DOES NOT MOVE under this rule: f2 is the force a sliding foot transmits, but the
 *      held foot stays where it is until the leg lifts off.  Feet that slide are include/mpcqp_slip.h: mpcqp_stance_slip and
 *      mpcqp_rollout_slip put slip kinematics behind steps 1 to 3.
 *   5. f_out = f2; tau = tau_app where bit 32 is clear, else (R J)^T (-f2); flag bits 2 clamped, 4 q outside [q_min, q_max], 16 the leg
 *      cannot be resolved, 32 the ground limited the force.
 *   6. a swing leg (contact == 0): f_out = f bit for bit, tau = 0, flag 0.
 * A stance leg with a non-finite operand (its force or foot) writes NaN into its own f_out and tau and flag 0xff; so do all four legs of
 * a robot whose x[0..11] or mu_g is not finite or whose mu_g < 0.  No other robot changes.
 * Arithmetic is fp64 without contraction, float32 outputs are rounded once.  Neither limit is told to the MPC: a controller that should
 * know lowers f_max through mpcqp_set_models (include/mpcqp_model.h) or mu.
 *   x        T  [B,13]   f  T [B,12]   feet  T [B,4,3]   contact  u8 [B,4]   as in mpcqp_plant_step
 *   ground   T  [B]      or NULL: no friction limit (the foot still cannot pull)
 *   geo, inr             as in mpcqp_leg_effort: tau_max, q_min, q_max are read (one row per call)
 *   f_out    T  [B,12]   out; may equal f
 *   tau      T  [B,4,3]  out, may be NULL        flag  u8 [B,4]  out, may be NULL
 * MPCQP_EINVAL: B negative or above 2^29 - 1, a null x, f, feet, contact or f_out (B > 0), an invalid geo / inr row.  B = 0 is a no-op.
 */
int mpcqp_stance_drive(mpcqp_handle h, int64_t B, const void* x, const void* f, const void* feet, const uint8_t* contact, const void* ground,
                       const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, void* f_out, void* tau, uint8_t* flag, void* stream);

/*
 * mpcqp_rollout_legs with the stance drive in its loop.  Every argument of mpcqp_rollout_legs keeps its meaning.
 *   drive     MPCQP_DRIVE_IDEAL: step 2 of the rule is skipped (no torque limit); MPCQP_DRIVE_LIMITED: the whole rule with inr's
 *             tau_max -- the row the swing legs are clamped by.  Anything else is MPCQP_EINVAL.
 *   ground    T [B] or NULL, as in mpcqp_stance_drive
 *   cmd_log   T [B,T,12] out, may be NULL: the COMMANDED stage-0 forces of the solve
 * Per tick, after the unchanged expand and solve, the rule runs on the live buffers: x, feet, the stance mask of the gait clock that the
 * advance uses, the solve's stage-0 forces.  Then:
 *   - the legs step's torso acceleration, the plant step and the `forces` log use the APPLIED forces
 *   - on stance rows tau_log is the rule's tau and flag_log the row's bits OR the rule's 2 / 16 / 32 (0xff for a poisoned leg); a stance
 *     row the legs step itself poisons (tau NaN, flag 0xff) stays so
 *   - the solver's own buffers are not altered: the next solve warm-starts from what it returned, not from what was delivered
 * MPCQP_DRIVE_IDEAL with ground = NULL leaves every force with f_z > 0 alone: x, ref, feet, legs, tick and every log are then
 * mpcqp_rollout_legs' bit for bit, and cmd_log == forces.  (In that mode a stance row the rule leaves alone keeps the torque
 * mpcqp_rollout_legs logs, which is the rule's tau_cmd up to the last place in fp64; in every other mode all stance rows hold the
 * rule's tau, so that mpcqp_stance_drive on the logged rows -- x = actual, f = cmd_log, feet_log, contact_log -- reproduces forces,
 * the stance rows of tau_log and the bits 2 / 16 / 32 of flag_log bit for bit.)
 * Six launches per tick, seven with tau_log or flag_log; no host synchronisation, copy or allocation inside the T ticks (the side
 * buffers are part of the roll-out's reserve).  A non-finite or negative ground row: that robot's applied forces are NaN, its solves
 * report MPCQP_STATUS_NONFINITE from the next tick with a stance leg on, and no other robot changes.
 * A tau_max per robot and a torque-speed curve are include/mpcqp_actuators.h: while mpcqp_set_actuators has set a table, step 2 clamps at
 * robot b's envelope at the joint rates with the foot at rest in the world, and the tau_max of `inr` is not read.
 * Not built: per-robot joint limits, a variant on plan tables.  (Slip kinematics: include/mpcqp_slip.h.)
 */
#define MPCQP_DRIVE_IDEAL 0
#define MPCQP_DRIVE_LIMITED 1
int mpcqp_rollout_drive(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                        const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                        const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains, int32_t leg_substeps,
                        const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, int32_t drive, const void* ground,
                        void* actual, void* desired, void* forces, void* feet_log, uint8_t* contact_log, int32_t* solved, void* swing_log,
                        void* q_log, void* qd_log, void* tau_log, void* foot_log, void* err_log, uint8_t* flag_log, void* miss_log,
                        void* cmd_log, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_SIM_H_ */
