/*
 * mpcqp_attitude.h -- extension of include/mpcqp_gate.h: velocity-aided attitude and gyro-bias states for the state estimator.
 *
 * mpcqp_estimate_track pulls its orientation towards the accelerometer's direction, so it takes every horizontal acceleration of a
 * moving torso for tilt; with the pull off (kappa = 0) the orientation is the gyro's integral and drifts linearly under any gyro
 * bias.  The leg-kinematic velocity update knows better: a tilt error delta makes the predicted acceleration wrong by |g| delta, and
 * step 2 of the row corrects the velocity by that much every row.  The aided rule feeds that correction back as a PI term: its
 * proportional part is a tilt reference that does not confuse acceleration with gravity, its integral is a gyro-bias state.
 *
 * The symbols declared here are exported by the product library libmpcqp.so ONLY (the host-side counterparts are
 * estimator.estimate_track_host and gaits.rollout_observe_host with attitude=, in the Python package).  Pointers, T, `stream`, return
 * codes and mpcqp_last_error() as in mpcqp_estimate.h.  All arithmetic is fp64 and not contracted, like the rest of the filter.
 *
 * The per-robot attitude state, att_state, is double [B,MPCQP_ATT_STATE] whatever the handle's I/O type, in / out:
 *   [0,3)  b^, the gyro bias estimate in the torso's axes
 *   [3,6)  e_b, the error signal of the last row: the update writes it, the predict reads it
 *   [6,8)  reserved, written 0
 * It is read where est_state's live is 1 (only b^ is read from outside a row); a fresh robot starts from b^ = 0.
 *
 * The rule.  The row is mpcqp_estimate_track's, with g' = gyro - b^ (b^ as the row finds it) and these changes:
 *   1. step 1 uses g' wherever it uses gyro:  rhod_l = R^ (g' x p_foot + J qd)
 *   2. before step 2 (and the gate's step 1g) v_pred[a] is kept: the velocity entry of xi[a], a = x, y; on a fresh row init's v
 *   3. after step 2, with v_post[a] the same entries:
 *        dv[a] = v_post[a] - v_pred[a]
 *        e_w   = (-dv[y] / (delta |g|), dv[x] / (delta |g|), 0)          (delta |g| is formed once)
 *        e_b   = R^T e_w, with the R^ of step 1; e_b goes to att_state[3..5]
 *   4. step 3: est's omega is R^ g'; bias_log is b^ as the row found it
 *   5. step 4, the orientation update:
 *        w^ = R^ ((g' + (k_s kap) (s^ x u)) + k_v e_b)                   per component, in this order
 *        b^ <- clamp(b^ - (k_b delta) e_b, +-b_max) per component        (k_b delta is formed once)
 *        q^ as in mpcqp_estimate_track; the position and covariance predict are unchanged.
 * With k_s = 1, k_v = 0, k_b = 0 and b^ = 0 the row is mpcqp_estimate_track's as values (a sum with +0.0 may change the sign of a
 * zero and nothing else).  k_s = k_v = k_b = 0 is the gyro-only orientation.
 *
 * What the rule is: a fixed-gain stand-in for the tilt-velocity cross-covariance of the full error-state filter, which would feed
 * the velocity innovation into the attitude through P.  It needs no stance detection of its own: an untrusted leg's inflated noise
 * (k_swing) makes its share of dv small, so flight rows barely correct.  The gate's w (mpcqp_gate.h) feeds it through the same
 * updates.  The world-z component of e_w is zero: yaw and the yaw-rate bias stay unobservable, and b^'s component along the world's
 * vertical is never driven.  A horizontal accelerometer bias is indistinguishable from tilt here as in any filter without a bias
 * state for it: 0.3 m/s^2 reads as about 43 mrad.
 *
 * Not built: accelerometer bias states; the full 27-state error-state filter; adaptive gains.
 */
#ifndef MPCQP_ATTITUDE_H_
#define MPCQP_ATTITUDE_H_

#include "mpcqp_gate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCQP_ATT_STATE 8          /* doubles per robot of att_state */
#define MPCQP_AIDED_GATE 1         /* flags: run the trust gate of mpcqp_gate.h (step 1g) */

/* The rule's gains.  The defaults are inputs, like the estimator's noise figures and the gate's thresholds: they are supported by a
 * host study on the eight named gaits only, not by a measurement on a robot. */
typedef struct MpcQpAttitude {
  uint32_t size;                /* sizeof(MpcQpAttitude) */
  double k_s;                   /* 0: the share of the accelerometer pull kappa that is kept */
  double k_v;                   /* 2.0 1/s: the proportional gain on e_b */
  double k_b;                   /* 5.0 1/s^2: the integral gain, into b^ */
  double b_max;                 /* 0.1 rad/s: the bound on each component of b^ */
} MpcQpAttitude;

/* Fills *att with the defaults above.  MPCQP_EINVAL for a null pointer. */
int mpcqp_default_attitude(MpcQpAttitude* att);

/*
 * `att` of the two calls below is a host pointer, NULL = the defaults.  MPCQP_EINVAL for a wrong `size`, a non-finite field or a
 * negative field, and for a bit of `flags` other than MPCQP_AIDED_GATE.
 */

/*
 * mpcqp_estimate_track with the aided rule.  Every argument up to trust_out is mpcqp_estimate_track_gated's, in its order and with
 * its meaning.
 *   flags                     MPCQP_AIDED_GATE: run the gate; without it `gate` is ignored and trust_out is c
 *   att                       the gains
 *   att_state    double [B,8] in / out, may be NULL: start from b^ = 0, nothing written back
 *   bias_log     T [B,T,3]    out, may be NULL: b^ as each row found it.  It counts as an output: at least one of est, feet_est,
 *                             sigma, nis, trust_out, bias_log.
 * `state` has mpcqp_estimate_track's layout.  A log cut in pieces through `state` and att_state gives the one call's outputs bit for bit.
 * Poison as in mpcqp_estimate_track: a non-finite b^ that is read, or a non-finite operand, makes the robot's outputs NaN from that
 * row on, bias_log included, and its `state` and att_state rows NaN.  No other robot changes.
 * MPCQP_EINVAL as in mpcqp_estimate_track_gated (all six outputs NULL), and bad gains or flags.  B = 0 or T = 0 is a no-op.
 */
int mpcqp_estimate_track_aided(mpcqp_handle h, int64_t B, int32_t T, const void* imu, const void* q, const void* qd,
                               const uint8_t* contact_log, const void* trust, const void* height, const void* init,
                               const MpcQpEstimator* par, const MpcQpLegGeometry* geo, double* state, void* est, void* feet_est, void* sigma,
                               void* nis, const MpcQpTrustGate* gate, void* trust_out, int32_t flags, const MpcQpAttitude* att,
                               double* att_state, void* bias_log, void* stream);

/*
 * mpcqp_rollout_observe with the aided rule inside the tick.  Every argument up to trust_log is mpcqp_rollout_observe_gated's, in
 * its order and with its meaning.
 *   flags, att                as above; without MPCQP_AIDED_GATE trust_log is the clock's c
 *   att_state    double [B,8] in / out, required (like est_state)
 *   bias_log     T [B,T,3]    out, may be NULL: b^ as each tick found it
 * Step 1 of the tick (sense and update) does items 1 to 4 of the rule and stores e_b; step 4 (predict) reads b^ and e_b back from
 * att_state, as it reads the trust from its side buffer.  The same nine launches per tick and the same reserve.  With
 * MPCQP_FEED_TRUTH the call is mpcqp_rollout_slip bit for bit.  With MPCQP_FEED_ESTIMATE the controller reads the aided estimate,
 * omega = R^ g' included.  mpcqp_estimate_track_aided on imu_log, q_enc_log, qd_enc_log and contact_log with the same flags, gate and
 * gains gives est_log, feet_est_log, sigma_log, nis_log, trust_log, bias_log, est_state and att_state bit for bit.
 * Poison as in mpcqp_rollout_observe_gated; bias_log follows est_log (a row whose accelerometer is not finite is NaN).
 * MPCQP_EINVAL as in mpcqp_rollout_observe_gated, a null att_state, and bad gains or flags.  B = 0 or T = 0 is a no-op.
 */
int mpcqp_rollout_observe_aided(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
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
                                void* bias_log, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_ATTITUDE_H_ */
