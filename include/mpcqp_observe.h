/*
 * mpcqp_observe.h -- extension of include/mpcqp_slip.h and mpcqp_estimate.h: the slip roll-out with sensors and the state estimator
 * inside its tick loop, and a switch for what the MPC reads.
 *
 * Every other roll-out hands the MPC the plant's true state.  mpcqp_rollout_observe is mpcqp_rollout_slip with, per tick, the row of
 * encoder and IMU readings a robot would have, one row of mpcqp_estimate_track on them, and -- with MPCQP_FEED_ESTIMATE -- the phase
 * expand and the solve reading that estimate in place of the plant's state.  With MPCQP_FEED_TRUTH the estimator only shadows the loop
 * and the call is mpcqp_rollout_slip bit for bit.
 *
 * The symbol declared here is exported by the product library libmpcqp.so ONLY (the host-side counterpart is
 * gaits.rollout_observe_host in the Python package).  Pointers are device memory on the handle's GPU, T is the handle's I/O dtype, work
 * is enqueued on `stream`, nothing is synchronised.  All arithmetic is fp64; the filter's own arithmetic is not contracted; every sensor
 * value is used as the I/O type holds it (rounded through T once), so the logs replay.  Return codes and mpcqp_last_error() as in mpcqp.h.
 *
 * The tick, with x, feet, legs, slip, gait and tick the live buffers:
 *   1. Sense and update, before the expand.
 *      Encoders of leg l: where the leg is in swing on the clock and its `legs` row is live, the carried (q, qd).  Otherwise the
 *      on-trajectory joint state the legs step will form for this row -- its swing row followed by the closed-form inverse and the rates
 *      with the same operands in the same order -- with one difference: the foot velocity of a stance leg is (slip[b,l], 0), not zero
 *      (the slip entry as T holds it, like the rest of the swing row: the foot_vel row mpcqp_joint_rates would be handed).
 *      With a zero slip entry that is the row's q_log / qd_log bit for bit; with a sliding foot the encoder rate contains the slide.
 *      enc_noise is added where given; the result, rounded to T, goes to q_enc_log / qd_enc_log.
 *      Gyro: R^T omega + bias_g + noise_g, R from x's rotation vector as mpcqp_imu_log forms it, rounded to T.
 *      Trust: contact != 0 on the clock.
 *      Steps 1 to 3 of mpcqp_estimate_track's row on est_state: the fresh start from est_init where live == 0, the four legs' scalar
 *      updates in their fixed order, the outputs.  The posterior xi, P and live = 1 go back to est_state, the est, feet_est, sigma and
 *      nis rows to their logs, and x^ [B,13] = (est row, x[12]) and f^eet [B,4,3] = the feet_est row to side buffers, in T.
 *   2. Expand and solve.  With MPCQP_FEED_ESTIMATE the phase expand and the solve's x0 read x^ and f^eet in place of x and feet; with
 *      MPCQP_FEED_TRUTH they read x and feet.  The same kernels and the same workspace either way.
 *   3. The slip rule, as in mpcqp_rollout_slip, on the true x and feet.
 *   4. Predict, before the legs step.  The specific force is R^T ((sum f_applied + F_push) / m + g e_z - g e_z) + bias_a + noise_a with
 *      the leg sum (0 + 1) + (2 + 3) and the body row as mpcqp_imu_log forms them, F_push where the robot's push window is open,
 *      g = par->gravity; a flight tick reads an exact zero.  Rounded to T; imu_log = (the gyro of step 1, the specific force).  Then step
 *      4 of mpcqp_estimate_track's row on est_state, with the R^ of the q^ that step 1 read and the gyro and the trust of step 1.
 *   5. Legs step, advance, landing and slip finish as in mpcqp_rollout_slip.  They read the true x and feet, and actual, forces,
 *      feet_log and every other log of mpcqp_rollout_slip stay the plant's truth.
 * After T ticks est_state is the predicted state for row T: mpcqp_estimate_track on imu_log, q_enc_log, qd_enc_log and contact_log with
 * init = est_init (or actual[:,0]) and the same height gives est_log, feet_est_log, sigma_log, nis_log and that state bit for bit.  On
 * rows without an open push window imu_log is mpcqp_imu_log on the call's logs bit for bit.
 *
 * Poison follows mpcqp_estimate_track: a non-finite sensor operand (x's rotation vector or omega, an encoder, bias, the row's noise or
 * enc_noise, the applied forces, the push or the body row), est_init or height row, or a live state that is not finite makes that
 * robot's estimator outputs NaN from that row on and its est_state NaN.  With MPCQP_FEED_ESTIMATE its QPs then report
 * MPCQP_STATUS_NONFINITE and `solved` stops counting.  No other robot changes.
 * What only step 4 reads -- the applied forces, the push, the body row -- is known after the row's solve: where one of them is the
 * first operand that is not finite, the row's estimator logs are overwritten with NaN in step 4, as mpcqp_estimate_track would give
 * them, but the expand and the solve of that one row have read the finite estimate, and the feed sees the poison from the next row on.
 *
 * Nine launches per tick (mpcqp_rollout_slip: seven); no host synchronisation, copy or allocation inside the T ticks: the side buffers
 * are part of the roll-out's reserve.
 *
 * Not built: the foothold rule at touchdown and the swing-leg controller still read the true state (they live inside the advance and
 * the legs step, which are mpcqp_rollout_slip's); contact detection from forces (trust is the clock; gating it on the legs' velocity
 * innovations is mpcqp_rollout_observe_gated, mpcqp_gate.h); accelerometer bias states (the gyro-bias state is
 * mpcqp_rollout_observe_aided, mpcqp_attitude.h); an IMU off the CoM; a host checker with model tables.
 */
#ifndef MPCQP_OBSERVE_H_
#define MPCQP_OBSERVE_H_

#include "mpcqp_estimate.h"
#include "mpcqp_slip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCQP_FEED_TRUTH 0      /* the MPC reads the plant's state: the estimator only shadows the loop */
#define MPCQP_FEED_ESTIMATE 1   /* the MPC reads the estimate */

/*
 * Every argument up to disp_log is mpcqp_rollout_slip's, in its order and with its meaning.
 *   feed          MPCQP_FEED_TRUTH or MPCQP_FEED_ESTIMATE
 *   est_state     double [B,131]  in / out, required: mpcqp_estimate_track's state.  live == 0 starts the robot's filter.
 *   est_init      T [B,12]        or NULL; read where live == 0.  NULL: the robot's x[0..11] at the call's first tick, as stored.
 *   height        T [B,4]         or NULL, as in mpcqp_estimate_track
 *   bias          T [B,6]         or NULL, as in mpcqp_imu_log
 *   noise         T [B,T,6]       or NULL, as in mpcqp_imu_log
 *   enc_noise     T [B,T,4,6]     or NULL: (q, qd) noise per leg, added as given
 *   par                           host pointer, NULL = the defaults; checked as in mpcqp_estimate.h
 *   imu_log       T [B,T,6]       out, may be NULL
 *   q_enc_log, qd_enc_log  T [B,T,4,3]  out, may be NULL
 *   est_log       T [B,T,12]      out, may be NULL, in the layout of `actual`
 *   feet_est_log  T [B,T,4,3]     out, may be NULL
 *   sigma_log     T [B,T,6]       out, may be NULL
 *   nis_log       T [B,T]         out, may be NULL
 * MPCQP_EINVAL: as mpcqp_rollout_slip, and a null est_state (B > 0), a feed that is neither value, a bad par.  B = 0 or T = 0 is a
 * no-op.
 */
int mpcqp_rollout_observe(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                          const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                          const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains, int32_t leg_substeps,
                          const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, int32_t drive, const void* ground,
                          const void* foot_mass, double* slip, void* actual, void* desired, void* forces, void* feet_log, uint8_t* contact_log,
                          int32_t* solved, void* swing_log, void* q_log, void* qd_log, void* tau_log, void* foot_log, void* err_log,
                          uint8_t* flag_log, void* miss_log, void* cmd_log, double* slip_log, void* disp_log, int32_t feed, double* est_state,
                          const void* est_init, const void* height, const void* bias, const void* noise, const void* enc_noise,
                          const MpcQpEstimator* par, void* imu_log, void* q_enc_log, void* qd_enc_log, void* est_log, void* feet_est_log,
                          void* sigma_log, void* nis_log, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_OBSERVE_H_ */
