/*
 * mpcqp_gate.h -- extension of include/mpcqp_estimate.h and mpcqp_observe.h: the estimator's trust gated per leg on the leg's own
 * velocity innovation.
 *
 * mpcqp_estimate_track and mpcqp_rollout_observe take a leg's trust from the gait clock (or from the caller): "a stance foot stands
 * still".  On a ground that lets feet slide that premise is false on exactly the rows that matter, and the filter takes the slide for
 * the torso's velocity.  The gate asks the filter itself: before a row's updates it compares what the leg's encoders say the torso's
 * horizontal velocity is with what the filter predicts, in units of the innovation's own variance, and takes the trust away from a leg
 * whose reading the prediction does not support.  It is one more step in the row of mpcqp_estimate_track, between its steps 1 and 2.
 *
 * The symbols declared here are exported by the product library libmpcqp.so ONLY (the host-side counterparts are
 * estimator.estimate_track_host and gaits.rollout_observe_host with gate=, in the Python package).  Pointers, T, `stream`, return
 * codes and mpcqp_last_error() as in mpcqp_estimate.h.  All arithmetic is fp64 and not contracted, like the rest of the filter.
 *
 * The rule, step 1g of the row.  It reads the predicted state -- xi and P as the row finds them, before any of its updates; on a fresh
 * row init's v and p0_v -- and the x and y filters only.  For leg l, with c_l the trust the row has without the gate (trust[b,t,l], or
 * contact != 0), v[a] the velocity entry of xi[a] and P_vv[a] its diagonal entry of P[a]:
 *   1. for a in {x, y}:  e = (-rhod_l[a]) - v[a],  S = P_vv[a] + r_v,  m_la = (e e) / S
 *   2. d_l = m_lx + m_ly
 *   3. g_l = 1 if d_l <= d_lo;  (d_hi - d_l) / (d_hi - d_lo) if d_lo < d_l < d_hi;  0 otherwise (d_l >= d_hi, and a d_l that is not a
 *      number: 0 / 0 where e and S are both zero)
 *   4. w_l = c_l g_l, rounded through T once, like every sensor value in mpcqp_observe.h.  g_l = 1 leaves c_l's bits.
 * Steps 2 and 4 of the row then use w_l wherever they use trust_l: in s_l = 1 + (1 - w_l) k_swing, which scales the leg's three
 * measurement variances, and in the foot's process noise q_f s_l.  w is also an output: mpcqp_estimate_track on the same operands with
 * trust = w gives the gated call's outputs and state bit for bit.
 * d_l is the leg's share of the row's nis along x and y had its velocity rows been the first updates of the row, with the unscaled r_v.
 * The thresholds are in those units, with two degrees of freedom: under a consistent filter a held foot's d_l has the mean
 * 2 P_vv / (P_vv + r_v) with exact encoders (its innovation is the velocity error, whose variance is P_vv) and 2 with encoder noise of
 * variance r_v; a foot that slides at 0.5 m/s along one axis under a filter with sigma_v = 0.1 m/s has d_l = 0.25 / 0.11 = 2.3.
 * The z axis is left out on purpose: the slip rule moves feet in xy, and the vertical innovation is where flight and landing show.
 *
 * Not built: hysteresis (a leg's gate has no memory: it opens again on the first row whose innovation is small); a force cue (the
 * commanded or applied force against the friction cone); a gate on z; telling the MPC (the solve still plans with the clock's contact).
 * (What the gated updates do to the orientation -- the velocity-aided attitude and gyro-bias states -- is mpcqp_attitude.h.)
 */
#ifndef MPCQP_GATE_H_
#define MPCQP_GATE_H_

#include "mpcqp_observe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gate's thresholds.  The defaults are inputs, like the estimator's noise figures: they are supported by a host study on the eight
 * named gaits only, not by a measurement on a robot. */
typedef struct MpcQpTrustGate {
  uint32_t size;                /* sizeof(MpcQpTrustGate) */
  double d_lo, d_hi;            /* 1.0, 4.0: full trust up to d_lo, none from d_hi on, linear in between */
} MpcQpTrustGate;

/* Fills *gate with the defaults above.  MPCQP_EINVAL for a null pointer. */
int mpcqp_default_trust_gate(MpcQpTrustGate* gate);

/*
 * `gate` of the two calls below is a host pointer, NULL = the defaults.  MPCQP_EINVAL for a wrong `size`, a non-finite field,
 * d_lo < 0 or d_hi <= d_lo.
 */

/*
 * mpcqp_estimate_track with the gate.  Every argument up to nis is mpcqp_estimate_track's, in its order and with its meaning.
 *   gate                      the thresholds
 *   trust_out    T [B,T,4]    out, may be NULL: w.  It counts as an output: at least one of est, feet_est, sigma, nis, trust_out.
 * `state` has mpcqp_estimate_track's layout and the two calls may be mixed on one state.  With thresholds no d_l reaches (d_lo =
 * 1e300) every output and the state are mpcqp_estimate_track's bit for bit and trust_out is c.
 * Poison as in mpcqp_estimate_track; a poisoned robot's trust_out is NaN from the poisoned row on.
 * MPCQP_EINVAL as in mpcqp_estimate_track (all of the five outputs NULL), and a bad gate.  B = 0 or T = 0 is a no-op.
 */
int mpcqp_estimate_track_gated(mpcqp_handle h, int64_t B, int32_t T, const void* imu, const void* q, const void* qd,
                               const uint8_t* contact_log, const void* trust, const void* height, const void* init,
                               const MpcQpEstimator* par, const MpcQpLegGeometry* geo, double* state, void* est, void* feet_est, void* sigma,
                               void* nis, const MpcQpTrustGate* gate, void* trust_out, void* stream);

/*
 * mpcqp_rollout_observe with the gate inside the tick's update.  Every argument up to nis_log is mpcqp_rollout_observe's, in its
 * order and with its meaning.
 *   gate                      the thresholds
 *   trust_log    T [B,T,4]    out, may be NULL: w of every tick
 * Step 1 of the tick forms c from the clock, then w, and steps 1 and 4 use w: the predict step reads it back from the side buffer
 * that already carries "the trust of step 1".  The same nine launches per tick and the same reserve.  With MPCQP_FEED_TRUTH the call
 * is mpcqp_rollout_slip bit for bit, as mpcqp_rollout_observe is.  mpcqp_estimate_track_gated on imu_log, q_enc_log, qd_enc_log and
 * contact_log with the same gate gives est_log, feet_est_log, sigma_log, nis_log, trust_log and est_state bit for bit.
 * Poison as in mpcqp_rollout_observe; a poisoned robot's trust_log is NaN from the poisoned row on.  Where the first operand that is
 * not finite is one only step 4 reads, the row's trust_log keeps the finite w that steps 1 to 3 used (the other estimator logs of
 * that row are overwritten with NaN), and trust_log is NaN from the next row on.
 * MPCQP_EINVAL as in mpcqp_rollout_observe, and a bad gate.  B = 0 or T = 0 is a no-op.
 */
int mpcqp_rollout_observe_gated(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                                const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                                const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains,
                                int32_t leg_substeps, const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, int32_t drive,
                                const void* ground, const void* foot_mass, double* slip, void* actual, void* desired, void* forces,
                                void* feet_log, uint8_t* contact_log, int32_t* solved, void* swing_log, void* q_log, void* qd_log,
                                void* tau_log, void* foot_log, void* err_log, uint8_t* flag_log, void* miss_log, void* cmd_log,
                                double* slip_log, void* disp_log, int32_t feed, double* est_state, const void* est_init, const void* height,
                                const void* bias, const void* noise, const void* enc_noise, const MpcQpEstimator* par, void* imu_log,
                                void* q_enc_log, void* qd_enc_log, void* est_log, void* feet_est_log, void* sigma_log, void* nis_log,
                                const MpcQpTrustGate* gate, void* trust_log, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_GATE_H_ */
