/*
 * mpcqp_model.h -- extension of include/mpcqp.h: per-robot model rows.
 *
 * Every QP of a batch is built from the handle's one MpcQpConfig.m, Ibody_inv, f_min and f_max.  A model table gives batch slot b
 * its own mass, principal inertias and f_z box instead: the controller of a robot that carries a payload, or whose model is
 * deliberately wrong (estimation-error studies), in the same launch as all the others.  The mass and the inertia enter only the
 * per-leg blocks T_jl = [Rz I^-1 [r_l]x ; c_l / m I_3] of the wrench-space form and the box only the bounds of the f_z rows
 * (DESIGN.md section 4), so everything the handle precomputes from the horizon, the tick and the weights stays shared.
 *
 * The symbols declared here are exported by the product library libmpcqp.so ONLY; the CPU checker library under oracle/ does
 * not have them (the host-side counterpart is models.grouped_host in the Python package, one checker handle per distinct row,
 * behind models.solve_batch_models_host and models.rollout_models_host / rollout_plant_models_host / rollout_phase_models_host /
 * rollout_legs_models_host / rollout_drive_models_host).  Return codes and mpcqp_last_error() as in mpcqp.h.
 *
 * Row layout: model[b] = (m, Ixx, Iyy, Izz, f_min, f_max), fp64 WHATEVER the handle's I/O dtype -- the table is small and set
 * once, not per tick, and fp64 lets a row reproduce the configuration exactly.  The first four entries are the first four of a
 * `body` row of include/mpcqp_sim.h; the inertias are the principal ones in the torso frame (the MPC's model is diagonal, as
 * MpcQpConfig.Ibody_inv is).  The engine keeps (1 / m, 1 / Ixx, 1 / Iyy, 1 / Izz, f_min, f_max), plain fp64 divisions: a row
 * (cfg.m, 1 / cfg.Ibody_inv[i], cfg.f_min, cfg.f_max) whose divisions are exact gives bit for bit the results of no table.
 *
 * Invalid rows: a non-finite entry, m <= 0, an inertia <= 0, f_min < 0 or f_max < f_min.  Such a row is kept as NaN and every
 * solve reports MPCQP_STATUS_NONFINITE with zero outputs for that QP; no other QP changes (the `body` rule of mpcqp_sim.h).
 * (A constant external wrench per robot, which the shift rule of mpcqp_disturb.h scales by this row's 1 / m and 1 / I, is set there.)
 */
#ifndef MPCQP_MODEL_H_
#define MPCQP_MODEL_H_

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Sets the handle's model table to the B rows at `model` (device memory on the handle's GPU, fp64 [B,6]).  One conversion kernel
 * is enqueued on `stream` into a table the engine owns (grown like the mpcqp_reserve workspace: a call at a larger B than any
 * before allocates, which synchronises the device); the caller's buffer is free again once that kernel has run, and solves
 * enqueued on the same stream afterwards see the new rows.
 *
 * Other streams: the host side of the handle counts the table as set from this call on, the device side from the moment the
 * conversion kernel has run.  A solve on ANOTHER stream must be ordered after `stream` by the caller (an event, or a
 * synchronisation); one that is not may run before the kernel and then reports MPCQP_STATUS_NONFINITE for every QP (no table
 * on the device yet) or reads the rows of the table set before.
 *
 * While a table is set, every entry point that solves reads row b for batch slot b: mpcqp_solve_batch, mpcqp_solve_batch_gait,
 * mpcqp_solve_batch_gait_steps and mpcqp_solve_batch_phase (mpcqp_plan.h), and, on every tick, the roll-outs mpcqp_rollout,
 * mpcqp_rollout_plant, mpcqp_rollout_phase, mpcqp_rollout_legs and mpcqp_rollout_drive (mpcqp_sim.h).  A call of one of them with
 * a B other than the table's returns MPCQP_EINVAL (the message names the entry point and both sizes).  X_out is then the
 * prediction under the robot's own row, and so is the next state of mpcqp_rollout (x <- X[:,1]).
 *
 * The row is the MPC's model and nothing else.  The plant of mpcqp_rollout_plant / _phase / _legs / _drive and of mpcqp_plant_step,
 * the legs step of mpcqp_rollout_legs / _drive (its torso acceleration is the plant's right-hand side) and mpcqp_leg_effort /
 * mpcqp_swing_track (mpcqp_joints.h) take their body from `body`; with body = NULL they use the CONFIGURATION's model
 * (MpcQpConfig.m, 1 / Ibody_inv), whatever the table says.  A robot whose plant is to be the body of its row passes
 * body[b] = (m, Ixx, Iyy, Izz, 0, 0, 0).  The stance drive (mpcqp_stance_drive, and inside mpcqp_rollout_drive) reads neither.
 *
 * MPCQP_EINVAL for B <= 0 or a null `model`, MPCQP_ENOMEM when the table cannot be grown; the table set before, if any, then stays.
 */
int mpcqp_set_models(mpcqp_handle h, int64_t B, const double* model, void* stream);

/*
 * Back to the configuration's m, Ibody_inv, f_min, f_max for every QP.  The allocation is kept.  The call has no stream: it waits
 * for the device (the solves enqueued so far finish with the table), then every later solve runs without it.
 */
int mpcqp_clear_models(mpcqp_handle h);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_MODEL_H_ */
