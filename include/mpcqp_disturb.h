/*
 * mpcqp_disturb.h -- extension of include/mpcqp.h: per-robot disturbance wrench rows for the MPC, and a wrench observer over the
 * logs of a roll-out.
 *
 * The plant can push a robot (`push`, `push_ticks` of mpcqp_sim.h) and can carry a body the controller does not know (`body` against
 * mpcqp_set_models).  A disturbance table tells the MPC: batch slot b plans under a constant world-frame force F at its CoM and a
 * constant world-frame torque tau about it.  mpcqp_disturbance_track estimates such a wrench from what a roll-out logged.
 *
 * The symbols declared here are exported by the product library libmpcqp.so ONLY; the CPU checker library under oracle/ does not
 * have them (the host-side counterparts are disturbance.shift_host, disturbance.DisturbedEngine -- a wrapper of a checker handle --
 * and disturbance.disturbance_track_host in the Python package).  Return codes and mpcqp_last_error() as in mpcqp.h.
 *
 * The rule.  The QP's dynamics are X[k+1] = Ad X[k] + Bd_k U[k] with Ad a function of the yaw of x0 alone.  A
 * constant wrench adds an affine term Cd to every stage.  With s[0] = 0, s[k+1] = Ad s[k] + Cd the disturbed states are X = X~ + s,
 * where X~ obeys the undisturbed dynamics under the same U; the cost |X - xdes| is |X~ - (xdes - s)|; the constraints touch only U
 * and X[12], and s[12] = 0.  So the disturbed QP is the undisturbed one with xdes replaced by xdes - s, and its predicted states are
 * the solver's plus s.  No solve kernel knows of the table: one element-wise kernel runs in front of the solve, one behind it.
 *
 *   c  = (0_3, 0_3, Rz diag(1 / I) Rz^T tau, F / m, 0), Rz from x0[2]; 1 / m and 1 / I of row b of the model table when one is set
 *        (mpcqp_model.h), else the configuration's (1 / MpcQpConfig.m, Ibody_inv)
 *   Cd = delta c for MPCQP_DISC_EULER, (delta I + delta^2 / 2 A) c for MPCQP_DISC_ZOH (what the discretisation does to B)
 *   s[k] = (delta^2 (k (k - 1) / 2 + theta k) Rz alpha,  delta^2 (k (k - 1) / 2 + theta k) a,  k delta alpha,  k delta a,  0)
 *        with alpha = c[6..8], a = c[9..11], theta = 0 (EULER) or 1 / 2 (ZOH): the recursion in closed form, A being nilpotent.
 * Arithmetic is fp64; xdes - s and X + s are rounded once into the handle's I/O dtype.
 *
 * Row layout: rows[b] = (F_x, F_y, F_z, tau_x, tau_y, tau_z), fp64 WHATEVER the handle's I/O dtype: the layout of a `push` row.
 * A row with a non-finite entry is kept as NaN: that robot's shifted xdes is NaN, its solve reports MPCQP_STATUS_NONFINITE with zero
 * outputs (nothing is added to its X_out), and no other QP changes.  So does a robot whose x0[2] or whose model row is not finite.
 *
 * The observer inside a roll-out's tick loop, with the table updated on the device every few ticks, is mpcqp_compensate.h.
 * Not built: a disturbance-aware foothold rule; a wrench that varies over the horizon; telling the plant.
 */
#ifndef MPCQP_DISTURB_H_
#define MPCQP_DISTURB_H_

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCQP_DIST_STATE 40   /* doubles per robot of the observer's state */

/*
 * Sets the handle's disturbance table to the B rows at `rows` (device memory on the handle's GPU, fp64 [B,6]).  Mechanics, lifetime,
 * size check and stream rules are those of mpcqp_set_models (mpcqp_model.h): one conversion kernel is enqueued on `stream` into a table
 * the engine owns (grown like the mpcqp_reserve workspace: a call at a larger B than any before allocates, which synchronises the
 * device), the caller's buffer is free again once that kernel has run, solves enqueued on the same stream afterwards see the new
 * rows, and a solve on ANOTHER stream must be ordered after `stream` by the caller.  With the table the engine grows a buffer of
 * [B,N+1,13] I/O elements for the shifted xdes; a handle that never had a table has neither.
 *
 * While a table is set, every entry point that solves reads row b for batch slot b -- mpcqp_solve_batch, mpcqp_solve_batch_gait,
 * mpcqp_solve_batch_gait_steps, mpcqp_solve_batch_phase and, on every tick, every roll-out of mpcqp.h, mpcqp_sim.h, mpcqp_slip.h,
 * mpcqp_observe.h, mpcqp_gate.h and mpcqp_attitude.h -- through one hook around the solve they share: the shift kernel writes
 * xdes - s into the engine's buffer before anything reads xdes (the dispatch-order pre-pass included), the solve reads that buffer, and
 * where X_out is non-null a second kernel adds s to it.  The caller's xdes, or the workspace xdes an expansion kernel wrote, is
 * never written.  That is two launches per solve more than without a table; without one, a solve launches exactly what it did.
 * A call of one of them with a B other than the table's returns MPCQP_EINVAL (the message names the entry point and both sizes).
 * X_out is then the prediction under the wrench, and so is the next state of mpcqp_rollout (x <- X[:,1]).
 *
 * The row is what the MPC is told and nothing else: the plant's push stays `push`, the observer below reads no table.
 *
 * MPCQP_EINVAL for B <= 0 or a null `rows`, MPCQP_ENOMEM when the table or the buffer cannot be grown; the table set before, if
 * any, then stays.
 */
int mpcqp_set_disturbance(mpcqp_handle h, int64_t B, const double* rows, void* stream);

/*
 * Back to no disturbance for every QP.  The allocations are kept.  The call has no stream: it waits for the device (the solves
 * enqueued so far finish with the table), then every later solve runs without it -- the launches of a handle that never had one.
 */
int mpcqp_clear_disturbance(mpcqp_handle h);

/*
 * The shift kernel alone, for tests (what mpcqp_phase_expand is to mpcqp_solve_batch_phase): out [B,N+1,13] = xdes - s for x0 [B,13]
 * and xdes [B,N+1,13] in the handle's I/O dtype, with the table that is set (and the model table, if one is).  `out` may be xdes.
 * MPCQP_EINVAL without a table, for a B other than the table's, or for a null buffer.
 */
int mpcqp_disturbance_shift(mpcqp_handle h, int64_t B, const void* x0, const void* xdes, void* out, void* stream);

/*
 * The observer's parameters.  The defaults are inputs, not measurements.  f_lim and t_lim clamp every component of the estimate's
 * force and torque (infinity: no clamp).
 */
typedef struct MpcQpWrenchObserver {
  uint32_t size;     /* sizeof(MpcQpWrenchObserver) */
  double gravity;    /* -9.81: the z acceleration the plant adds (its x[12]) */
  double kappa;      /* 0.2: the gain of the first-order filter, in [0, 1] */
  double f_lim;      /* infinity, N */
  double t_lim;      /* infinity, N m */
} MpcQpWrenchObserver;

int mpcqp_default_wrench_observer(MpcQpWrenchObserver* par);

/*
 * A momentum observer over the rows of a roll-out's logs: one lane per robot, serial in T.
 *
 *   actual, forces  T [B,T,12]   the torso rows (rotation vector, CoM, omega, v) and the foot forces applied over each row's tick.
 *                                Either the plant's truth (the `actual` and `forces` logs of a roll-out) or what a robot has: `est`
 *                                of mpcqp_rollout_observe (mpcqp_observe.h), which has the layout of `actual`, and its `cmd` log.
 *   feet            T [B,T,4,3]  the `feet_log` of the roll-out
 *   body            T [B,7]      (m, Ixx, Iyy, Izz, Ixy, Ixz, Iyz) as in mpcqp_sim.h, or NULL for the configuration's model.  An
 *                                invalid row (its rule there) poisons the robot, as in mpcqp_leg_effort (mpcqp_joints.h).
 *   par                          NULL: the defaults
 *   state           double [B,MPCQP_DIST_STATE], in / out, may be NULL: d^ (6), then the previous row's L (3), v (3), p (3),
 *                                f (12), feet (12), then `live` (0: there is no previous row yet).  Zeros start an observer.
 *   dist, resid     T [B,T,6]    outputs, each may be NULL, at least one is required
 *
 * Per row t: R from the row's rotation vector as the plant converts it (through the quaternion), L = R I_b R^T omega, v, p.  If
 * the state is live, with `prev` the row before:
 *   res_F   = m (v - v_prev) / delta - ((f0 + f1) + (f2 + f3))_prev - m g e_z
 *   res_tau = (L - L_prev) / delta - sum_l (feet_prev_l - (p_prev + p) / 2) x f_prev_l     (the legs in the force sum's order)
 *   d^      = clamp(d^ + kappa (res - d^))
 * otherwise res = 0 and d^ stays.  Then the row becomes `prev` and live = 1.  dist[b,t] = d^, resid[b,t] = res.  The plant holds
 * the forces over a tick, so res_F is the push up to rounding; the lever arms move during the tick, and res_tau with the arms at the
 * midpoint of the two CoMs carries an error of that order (DESIGN.md has the figures).
 * A leg whose three force entries are all zero is left out of both sums by a select, and its foot is then not read: a NaN foot of a
 * swing leg does not poison the row (the state keeps a zero in its place).
 * Arithmetic is fp64 and not contracted; a call split into pieces through `state` reproduces the unsplit call bit for bit.
 *
 * Poison is mpcqp_estimate_track's (mpcqp_estimate.h): a non-finite operand of row t (a foot of a leg that is left out excepted) makes
 * the outputs of that robot NaN from row t on, a non-finite state or an invalid body row from the first row on, and the robot's
 * returned state is NaN.  No other robot changes.
 *
 * MPCQP_EINVAL: a size out of range (B T beyond 2^29), both outputs NULL, a NULL actual / forces / feet with B T > 0, a struct
 * size mismatch, a gravity that is not finite and negative, a kappa outside [0, 1], a negative or NaN f_lim / t_lim.
 */
int mpcqp_disturbance_track(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet, const void* body,
                            const MpcQpWrenchObserver* par, double* state, void* dist, void* resid, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_DISTURB_H_ */
