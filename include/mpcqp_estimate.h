/*
 * mpcqp_estimate.h -- extension of include/mpcqp_sim.h and mpcqp_joints.h: the torso state estimated from an IMU and leg kinematics.
 *
 * Every roll-out hands the MPC the plant's true state.  The MIT Cheetah 3 controller reads an estimate instead: an orientation filter
 * on gyro and accelerometer, and a Kalman filter that fuses the accelerometer with leg kinematics under the assumption that stance
 * feet stand still.  This header has both as passes over a roll-out's logs: mpcqp_imu_log computes what an IMU at the CoM reads on
 * every row, mpcqp_estimate_track runs the filter over the rows, one filter per robot, with its state in / out so that a log can be
 * processed in pieces (and, later, one row per tick inside a roll-out).
 *
 * The symbols declared here are exported by the product library libmpcqp.so ONLY (the host-side counterparts are estimator.imu_log_host,
 * estimator.estimate_track_host and, as an independent 18-state form, estimator.estimate_joint_host in the Python package).  Pointers
 * are device memory on the handle's GPU, T is the handle's I/O dtype, work is enqueued on `stream`, nothing is synchronised or
 * allocated.  All arithmetic is fp64; the filter's own arithmetic (everything below but the leg's forward map) is not contracted;
 * float32 outputs are rounded once.  Return codes and mpcqp_last_error() as in mpcqp.h.
 *
 * Not built: accelerometer bias states (a given bias is read as it is; a gyro-bias state and an orientation steered by the velocity
 * update are mpcqp_attitude.h), contact detection from forces (trust is given;
 * gating it on the legs' velocity innovations is mpcqp_gate.h), an IMU off the CoM, telling the MPC the estimate's covariance.  (The
 * estimate inside a roll-out's tick loop is mpcqp_observe.h; an external wrench estimated from a roll-out's logs is mpcqp_disturb.h.)
 */
#ifndef MPCQP_ESTIMATE_H_
#define MPCQP_ESTIMATE_H_

#include "mpcqp_joints.h"
#include "mpcqp_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The filter's parameters.  The defaults are inputs, not measurements: the noise figures of the open MIT controller as remembered. */
typedef struct MpcQpEstimator {
  uint32_t size;                /* sizeof(MpcQpEstimator) */
  double gravity;               /* -9.81 */
  double kappa;                 /* 2.0 1/s: gain of the accelerometer's tilt correction */
  double q_p, q_v, q_f;         /* process noise densities of p, v, a trusted foot: 0.02, 0.02, 0.002 */
  double r_p, r_v, r_z;         /* measurement variances of relative foot position, relative foot velocity, foot height: 0.001, 0.1, 0.001 */
  double k_swing;               /* 100: how much an untrusted leg's noises are inflated */
  double p0_p, p0_v, p0_f;      /* initial variances: 0.01, 1.0, 0.01 */
} MpcQpEstimator;

/* Fills *par with the defaults above.  MPCQP_EINVAL for a null pointer. */
int mpcqp_default_estimator(MpcQpEstimator* par);

/*
 * `par` of the two calls below is a host pointer, NULL = the defaults.  MPCQP_EINVAL for a wrong `size`, a non-finite field, a
 * non-negative gravity, or a negative kappa, noise (q_*, r_*, p0_*) or k_swing.
 */

/*
 * What an IMU at the CoM reads on every row of a log, one lane per (robot, row).
 *   actual, forces  T [B,T,12]   as mpcqp_leg_effort takes them (actual = rotation vector, CoM, omega, v)
 *   feet            T [B,T,4,3]  as mpcqp_leg_effort takes it; required, and not read: an IMU at the CoM does not feel alpha
 *   base_acc        T [B,T,6]    (alpha, a) of the torso / CoM in world axes, or NULL: a is the unpushed plant's right-hand side at the
 *                                row, (sum f_l) / m + g e_z with the sum and the body row as mpcqp_leg_effort forms them
 *   body            T [B,7]      read only without base_acc; NULL = the handle's model.  An invalid row makes the robot's rows NaN.
 *   bias            T [B,6]      gyro and accelerometer bias, or NULL; added as given
 *   noise           T [B,T,6]    or NULL; added as given (the caller draws it; there is no device RNG)
 *   imu             T [B,T,6]    out: (R^T omega + bias_g + n_g, R^T (a - g e_z) + bias_a + n_a), R from the row's rotation vector as
 *                                mpcqp_joint_log forms it, g = par->gravity
 * A flight row (forces zero) reads zero specific force, exactly.  A non-finite operand of a row that is read (rotation vector, omega,
 * the base_acc row or the forces and the body row, bias, noise) makes that row NaN and touches nothing else.
 * MPCQP_EINVAL: B or T negative, B T > 0x1fffffff, a null actual, forces, feet or imu (B, T > 0), a bad par.  B = 0 or T = 0 is a no-op.
 */
int mpcqp_imu_log(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet, const void* base_acc,
                  const void* body, const void* bias, const void* noise, const MpcQpEstimator* par, void* imu, void* stream);

/*
 * The filter state of one robot, fp64 whatever the I/O dtype, for the reason `legs` is (mpcqp_sim.h):
 *   [0,4)     the orientation quaternion (w, x, y, z)
 *   [4,22)    xi[a][6], axis a = x, y, z: (p, v, c_FL, c_FR, c_HL, c_HR) -- CoM, velocity and the four feet along that axis
 *   [22,130)  P[a][6][6], the covariance of xi[a], stored in full; read from its upper triangle (row <= column)
 *   [130]     live: 0 = the robot starts from `init`
 */
#define MPCQP_EST_STATE 131

/*
 * The filter over the T rows of B robots; four lanes per robot, serial in T.
 *   imu          T [B,T,6]     (gyro, specific force) in the torso's axes: mpcqp_imu_log's output
 *   q, qd        T [B,T,4,3]   the encoders: the q_log / qd_log of mpcqp_rollout_legs, _drive and _slip, or mpcqp_joint_rates' q, qd
 *   contact_log  u8 [B,T,4]    read only without trust
 *   trust        T [B,T,4]     in [0,1], or NULL: contact != 0 ? 1 : 0
 *   height       T [B,4]       the ground height under each foot, or NULL: no height rows
 *   init         T [B,12]      required, in the layout of an `actual` row; theta, p and v are read
 *   state        double [B,131] in / out, may be NULL.  live == 0 or NULL: the robot starts from init, and nothing is written back for
 *                              NULL.  On return: the predicted state for row T, live = 1.
 *   est          T [B,T,12]    out, in the layout of `actual`: (theta, p, omega, v)
 *   feet_est     T [B,T,4,3]   out
 *   sigma        T [B,T,6]     out: sqrt of P's p diagonal entry along x, y, z, then of its v entry
 *   nis          T [B,T]       out: the row's normalised innovation squared, summed over its scalar measurements
 * Each output may be NULL; at least one is required.
 *
 * Start (live == 0): q^ from init[0..2] (the plant's rotation-vector conversion), p = init[3..5], v = init[9..11],
 * c_l = p + R^ p_foot(q[b,0,l]), P[a] = diag(p0_p, p0_v, p0_f x 4).
 *
 * The row, with d = the handle's delta:
 *   1. R^ from q^.  Per leg l: rho_l = R^ p_foot(q_l), rhod_l = R^ (gyro x p_foot(q_l) + J(q_l) qd_l), p_foot and J as
 *      mpcqp_leg_jacobians forms them; s_l = 1 + (1 - trust_l) k_swing.
 *   2. Each axis a is updated by scalar measurements in the order l = 0..3, each time (i), (ii), (iii):
 *        (i)   z = rho_l[a],     h = e_{c_l} - e_p,  r = r_p s_l
 *        (ii)  z = -rhod_l[a],   h = e_v,            r = r_v s_l
 *        (iii) a = z and height given only:  z = height[b,l],  h = e_{c_l},  r = r_z s_l
 *      One update: w = P h, S = h^T w + r, k = w / S, e = z - h^T xi;  xi += k e;  P[i][j] -= k_i w_j on the upper triangle, mirrored, so
 *      that P stays exactly symmetric;  nis_a += e e / S.  The row's nis is (nis_x + nis_y) + nis_z.
 *   3. Outputs: est = (rotation vector of q^, p^, R^ gyro, v^), feet_est = c^_l, sigma, nis.
 *   4. Predict: a_w = R^ s + g e_z with s = imu[3..5] and the R^ of step 1.  Per axis p = (p + d v) + (d d / 2) a_w[a], v = v + d a_w[a];
 *      P = A P A^T + d diag(q_p, q_v, q_f s_0..3), A the identity with A[p][v] = d:
 *      P_pp = (P_pp + d P_pv) + d (P_pv + d P_vv), then P_pj = P_pj + d P_vj for j = v, c_0..3 (the old P_vj).
 *      Orientation: u = R^^T e_z;  if |s| > 0: s^ = s / |s| and kap = kappa clamp(1 - ||s| - |g|| / |g|, 0, 1), else kap = 0 (a select);
 *      w^ = R^ (gyro + kap (s^ x u));  q^ = normalise(quat(d w^) (x) q^).  A tilt error decays at the rate kappa; yaw is not observable and
 *      stays where init put it.
 * In exact arithmetic the three 6-state filters with scalar updates are the usual filter with 18 states and 28 measurements: all
 * noises are isotropic and every matrix is a Kronecker product with I_3, apart from the height rows.  No matrix inverse.
 *
 * Poison: a non-finite operand of robot b's row (its imu, q, qd, trust, the robot's height or init row, a live state that is not
 * finite) makes that robot's outputs NaN from that row on (height, init and state: from row 0) and every entry of its returned state
 * NaN.  No other robot changes.
 * MPCQP_EINVAL: B or T negative, B T > 0x1fffffff, a null imu, q, qd or init, a null contact_log without trust (B, T > 0), all outputs
 * NULL, a bad par, an invalid geo row.  B = 0 or T = 0 is a no-op.
 */
int mpcqp_estimate_track(mpcqp_handle h, int64_t B, int32_t T, const void* imu, const void* q, const void* qd, const uint8_t* contact_log,
                         const void* trust, const void* height, const void* init, const MpcQpEstimator* par, const MpcQpLegGeometry* geo,
                         double* state, void* est, void* feet_est, void* sigma, void* nis, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_ESTIMATE_H_ */
