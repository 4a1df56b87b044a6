/*
 * mpcqp_compensate.h -- extension of include/mpcqp_attitude.h and include/mpcqp_disturb.h: the wrench observer and the disturbance table
 * update inside the tick loop of mpcqp_rollout_observe.
 *
 * mpcqp_disturb.h gives the MPC a per-robot wrench table and estimates such a wrench from a roll-out's logs; between the two the loop
 * closes on the host (disturbance.compensated_rollout in the Python package: a roll-out call, an observer call and a table call per
 * piece).  Here one roll-out call does it on the device: every tick runs one row of mpcqp_disturbance_track's observer on a carried
 * state, and every `hold` ticks the estimate becomes the robot's row of the handle's table, which the next tick's solve plans under.
 * The operands are the plant's truth or what a robot has -- the state estimate, the commanded forces and the estimated feet of
 * mpcqp_rollout_observe --, so that a push or a payload nobody told the controller about is estimated from IMU, encoders and commanded
 * forces and reaches the next solve without the host in between.
 *
 * The symbols declared here are exported by the product library libmpcqp.so ONLY (the host-side counterpart is
 * disturbance.rollout_compensated_host in the Python package).  Pointers, T, `stream`, return codes and mpcqp_last_error() as in
 * mpcqp_observe.h.  The observer's arithmetic is fp64 and not contracted: it is the row of mpcqp_disturbance_track, written once.
 *
 * The rule.  The tick is mpcqp_rollout_observe's (or _gated's or _aided's: MpcQpCompensate.flags) with one more step.  Per tick `it` of
 * the call, after the slip rule has produced the applied forces and the estimator's predict has run, BEFORE the advance moves x and
 * before the slip finish moves the feet, one row of mpcqp_disturbance_track's rule (mpcqp_disturb.h) runs on robot b's row of
 * dist_state.  Every operand is read as the I/O type holds it, so the logs replay:
 *   MPCQP_WRENCH_TRUTH    the live x[0..11], the applied forces and the live feet: the `actual`, `forces` and `feet_log` rows of tick it
 *   MPCQP_WRENCH_SENSED   the estimator's x^ and f^eet of tick it (the side buffers its update step fills, whichever `feed` is) and the
 *                         solve's stage-0 forces: the `est_log`, `cmd_log` and `feet_est_log` rows of tick it, which may be NULL.  A
 *                         robot whose predict step poisons its est_log row (mpcqp_observe.h) counts as a NaN operand.
 * The body row is obs_body's: the body the OBSERVER believes, NULL = the configuration's model.  It is not the plant's `body`: a payload
 * of dm kg that the plant carries and the observer is not told of shows up as a residual of -dm |g| in F_z.
 * d^ and res go to dist_log[b,it] and resid_log[b,it], rounded to the I/O type, NaN for a poisoned robot.
 * On an update tick -- (it + 1) % hold == 0, or it == T - 1 -- the same kernel writes robot b's row of the handle's disturbance table:
 * d^ AS THE I/O TYPE HOLDS IT (the dist_log entry), widened to fp64, under mpcqp_set_disturbance's conversion: a non-finite entry makes
 * six NaNs.  The shift and add-back kernels around the solve of tick it + 1 read it.  `it` is the call's own tick index: a call cut
 * into pieces through the carried states reproduces the uncut call bit for bit when every piece's T is a multiple of `hold`.
 * The whole is disturbance.compensated_rollout at piece = hold composed of mpcqp_set_disturbance, mpcqp_rollout_observe and
 * mpcqp_disturbance_track, as values.
 *
 * The table.  At entry the call sets the handle's table to B rows as mpcqp_set_disturbance does -- it grows the table and the shifted
 * xdes buffer at a B larger than any before, which synchronises the device -- with rows dist_state[:,0:6] through the same conversion
 * (as the I/O type holds them, widened to fp64, six NaNs for a non-finite entry): what the update tick that left that state wrote, and
 * for a fresh (zero) state a table that tells the MPC nothing.  A table of another size set before is replaced.  The table
 * STAYS SET when the call returns: later solves of the handle read it until mpcqp_clear_disturbance or mpcqp_set_disturbance.
 * Ten launches per tick: the nine of mpcqp_rollout_observe under a table (shift and add-back included) and the observer's.
 *
 * Poison.  A robot whose observer row is not finite (a non-finite operand, state or obs_body row) gets NaN rows in dist_log and
 * resid_log from that tick on and a NaN dist_state; on the next update tick its table row is NaN, so its QPs report
 * MPCQP_STATUS_NONFINITE from the tick after it (and with zero forces the plant takes it where it takes any unsolved robot).  No other
 * robot changes.
 *
 * Not built: a disturbance-aware foothold rule; a wrench that varies over the horizon; telling the plant.
 */
#ifndef MPCQP_COMPENSATE_H_
#define MPCQP_COMPENSATE_H_

#include "mpcqp_attitude.h"
#include "mpcqp_disturb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCQP_WRENCH_TRUTH 0       /* source: the observer reads the plant's truth */
#define MPCQP_WRENCH_SENSED 1      /* source: the observer reads the state estimate, the commanded forces and the estimated feet */
#define MPCQP_COMP_GATED 1         /* flags: the estimator is mpcqp_rollout_observe_gated's */
#define MPCQP_COMP_AIDED 2         /* flags: the estimator is mpcqp_rollout_observe_aided's */

typedef struct MpcQpCompensate {
  uint32_t size;                   /* sizeof(MpcQpCompensate) */
  uint32_t flags;                  /* 0: which estimator runs, see below */
  int32_t source;                  /* MPCQP_WRENCH_TRUTH */
  int32_t hold;                    /* 1: ticks between two updates of the table, >= 1 */
  MpcQpWrenchObserver observer;    /* the observer's parameters (mpcqp_default_wrench_observer) */
} MpcQpCompensate;

/* Fills *comp with the defaults above.  MPCQP_EINVAL for a null pointer. */
int mpcqp_default_compensate(MpcQpCompensate* comp);

/*
 * mpcqp_rollout_observe with the observer and the table update inside the tick.  Every argument up to bias_log is
 * mpcqp_rollout_observe_aided's, in its order and with its meaning; which of the estimator's arguments are read is comp->flags':
 *   0                                    mpcqp_rollout_observe: gate, trust_log, flags, att, att_state and bias_log are not read
 *   MPCQP_COMP_GATED                     mpcqp_rollout_observe_gated: gate and trust_log are read as well
 *   MPCQP_COMP_AIDED                     mpcqp_rollout_observe_aided: all of them, the gate as `flags` says (MPCQP_AIDED_GATE)
 *   MPCQP_COMP_AIDED | MPCQP_COMP_GATED  mpcqp_rollout_observe_aided with the gate, whatever `flags` says of it
 * Then:
 *   comp                      host pointer, NULL = the defaults
 *   obs_body     T [B,7]      the body the observer believes, as `body` of mpcqp_disturbance_track, or NULL
 *   dist_state   double [B,MPCQP_DIST_STATE]  in / out, required: the `state` of mpcqp_disturbance_track.  Zeros start an observer.
 *   dist_log     T [B,T,6]    out, may be NULL: d^ after each tick's row
 *   resid_log    T [B,T,6]    out, may be NULL: the residual of each tick's row
 * With comp->observer.kappa = 0 and a zero dist_state the call is the estimator's call under a table of zero rows, as values.
 * MPCQP_EINVAL as in the estimator's call, and: a source other than the two, hold < 1, a flag bit other than the two, a struct size
 * mismatch (comp's or its observer's), an observer field as mpcqp_disturbance_track refuses it, a null dist_state with B > 0.
 * MPCQP_ENOMEM when the table cannot be grown (the table set before then stays).  B = 0 or T = 0 is a no-op: no table is set.
 */
int mpcqp_rollout_observe_compensated(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                                      const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                                      const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains,
                                      int32_t leg_substeps, const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, int32_t drive,
                                      const void* ground, const void* foot_mass, double* slip, void* actual, void* desired, void* forces,
                                      void* feet_log, uint8_t* contact_log, int32_t* solved, void* swing_log, void* q_log, void* qd_log,
                                      void* tau_log, void* foot_log, void* err_log, uint8_t* flag_log, void* miss_log, void* cmd_log,
                                      double* slip_log, void* disp_log, int32_t feed, double* est_state, const void* est_init, const void* height,
                                      const void* bias, const void* noise, const void* enc_noise, const MpcQpEstimator* par, void* imu_log,
                                      void* q_enc_log, void* qd_enc_log, void* est_log, void* feet_est_log, void* sigma_log, void* nis_log,
                                      const MpcQpTrustGate* gate, void* trust_log, int32_t flags, const MpcQpAttitude* att, double* att_state,
                                      void* bias_log, const MpcQpCompensate* comp, const void* obs_body, double* dist_state, void* dist_log,
                                      void* resid_log, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_COMPENSATE_H_ */
