/*
 * mpcqp_joints.h -- extension of include/mpcqp.h: closed-form leg inverse kinematics and the joint-space log of a roll-out.
 *
 * The roll-out's logs (actual / desired / forces) stop at the torso.  The reference's controller also logs the twelve joint
 * torques and the feet every tick (CONTROL EFFORT and FEET POS, src/main.py:152-176, torque map src/main.py:212-214); both go
 * through joint angles.  mpcqp_leg_ik is the inverse of the `foot` output of mpcqp_leg_jacobians; mpcqp_joint_log turns the
 * logs of a roll-out and the feet of its plan into per-tick joint angles, joint torques and reach flags in one launch.
 *
 * The symbols declared here are exported by the product library libmpcqp.so ONLY; the CPU checker library under oracle/ does
 * not have them (the host-side counterparts are lite3_model.leg_ik_closed / lite3_model.joint_log_host in the Python package).
 * Pointers are device memory on the handle's GPU, T is the handle's I/O dtype (MpcQpConfig.dtype), work is enqueued on `stream`,
 * nothing is synchronised and nothing is allocated.  The arithmetic is fp64 whatever T is: fp32 outputs are the fp64 results
 * rounded once.  Return codes and mpcqp_last_error() as in mpcqp.h: sizes, null pointers and the geometry are checked on the
 * host (MPCQP_EINVAL).
 *
 * Geometry.  The closed form needs the structure of the Lite3's leg, a HipX joint followed by a planar two-link chain:
 *   axis_x = +-e_x,  axis_y = +-e_y,  hip_y[l] = (0, d_l, 0),  knee = (0, 0, -l1),  foot = (0, 0, -l2),  l1, l2 > 0
 * (hip_x is free).  Any other MpcQpLegGeometry is MPCQP_EINVAL, with the failing field named in mpcqp_last_error().  The signs
 * s_x, s_y of the two axes are read from the geometry: a joint angle q about the axis s e is the angle s q about +e.
 *
 * The inverse, per leg l.  Let p = rot^T (foot - origin) - hip_x[l] and d = d_l.  The foot in the HipX link frame is
 * (p_x, d, z_s) with
 *   z_s   = -sqrt(p_y^2 + p_z^2 - d^2)
 *   HipX  = s_x atan2(d p_z - z_s p_y, d p_y + z_s p_z)           the rotation about e_x that turns (d, z_s) onto (p_y, p_z)
 *   c     = (p_x^2 + z_s^2 - l1^2 - l2^2) / (2 l1 l2),   Knee = acos(c),   s = sqrt((1 - c)(1 + c))
 *   HipY  = s_y atan2(z_s v - p_x u, -(z_s u + p_x v)),   u = l1 + l2 c,  v = s_y l2 s
 * Branch (fixed): the foot lies below the HipX axis in the HipX link frame (z_s <= 0) and the knee angle lies in [0, pi].  This is
 * the branch of the reference's initial configuration (0, -60, 90 degrees).  Joint vectors on it satisfy
 * l1 cos(HipY) + l2 cos(HipY + Knee) >= 0, and for those mpcqp_leg_ik inverts mpcqp_leg_jacobians' foot to rounding; the error
 * of HipY and Knee grows like 1 / (l sin Knee) towards the straight and the folded knee, that of HipX like 1 / |z_s|.
 *
 * Reach.  reach = 1 exactly when p_y^2 + p_z^2 >= d^2 and |l1 - l2| <= sqrt(p_x^2 + z_s^2) <= l1 + l2.  Otherwise the offending
 * quantities are clamped -- the square-root argument at 0, the cosine at +-1 -- so that q is the finite joint vector of the
 * nearest boundary (leg stretched, leg folded, foot on the HipX axis' cylinder of radius |d|), and reach = 0.  A leg with a
 * non-finite input (its foot, or its robot's rot / origin) writes NaN into its own q and 0 into its own reach; no other leg
 * is touched.
 */
#ifndef MPCQP_JOINTS_H_
#define MPCQP_JOINTS_H_

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Joint angles of the four legs from their foot positions, for B robots.
 *   foot    T  [B,4,3]  foot positions FL, FR, HL, HR, world orientation
 *   rot     T  [B,3,3]  torso orientation (world <- torso), row-major; NULL = identity
 *   origin  T  [B,3]    torso origin in the frame of `foot`; NULL = zero.  With rot and origin NULL the call is the exact inverse
 *                       of the `foot` output of mpcqp_leg_jacobians.
 *   geo                 host pointer, NULL = the Lite3 (mpcqp_default_leg_geometry)
 *   q       T  [B,4,3]  out: HipX, HipY, Knee in rad
 *   reach   u8 [B,4]    out, may be NULL
 * B = 0 is a no-op (MPCQP_OK), as for mpcqp_leg_jacobians; B < 0 or B > 0x1fffffff is MPCQP_EINVAL.
 */
int mpcqp_leg_ik(mpcqp_handle h, int64_t B, const void* foot, const void* rot, const void* origin, const MpcQpLegGeometry* geo,
                 void* q, uint8_t* reach, void* stream);

/*
 * Joint-space log of a roll-out: joint angles, joint torques and reach flags of every (robot, tick, leg).
 *   actual  T  [B,T,12]   as mpcqp_rollout / mpcqp_rollout_plant log it: rotation vector, CoM, omega, v
 *   forces  T  [B,T,12]   as they log it: the stage-0 forces FL, FR, HL, HR
 *   feet    T  [B,T,4,3]  world foot positions.  The feet_des output of mpcqp_swing_trajectories with K = T and the roll-out's
 *                         first tick is exactly this operand: stance feet on the plan, swing feet on their trajectory.
 *   geo                   host pointer, NULL = the Lite3
 *   q       T  [B,T,4,3]  out, may be NULL: HipX, HipY, Knee
 *   tau     T  [B,T,4,3]  out, may be NULL: joint torques
 *   reach   u8 [B,T,4]    out, may be NULL
 * At least one output is required (all three NULL: MPCQP_EINVAL).  B = 0 or T = 0 is a no-op; B T > 0x1fffffff is MPCQP_EINVAL.
 * Per (robot, tick, leg): R from the rotation vector (through the unit quaternion, with the plant's series below an angle of
 * 1e-3, include/mpcqp_sim.h); the inverse above with rot = R and origin = CoM -- the CoM stands in for the torso origin, as in
 * the package's kinematic controller model; the world Jacobian R J(q) of mpcqp_leg_jacobians; tau = (R J)^T (-f)
 * (src/main.py:212-214).  A swing leg's force is an exact zero of the solve, so its torque is a zero: no contact mask is needed.
 * The torque is computed from the clamped q also where reach = 0.  Non-finite rows as above (q and tau NaN, reach 0).
 */
int mpcqp_joint_log(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet,
                    const MpcQpLegGeometry* geo, void* q, void* tau, uint8_t* reach, void* stream);

/*
 * mpcqp_joint_log plus joint rates and joint power.
 *   actual, forces, feet, geo   as for mpcqp_joint_log; of actual also omega = [6..8] and v = [9..11] are read
 *   foot_vel T  [B,T,4,3]  world velocity of each foot, or NULL = the feet are at rest in the world (stance feet; the `vel` of
 *                          mpcqp_phase_swing for a swing leg)
 *   q        T  [B,T,4,3]  out, may be NULL: as mpcqp_joint_log
 *   qd       T  [B,T,4,3]  out, may be NULL: joint rates in rad / s
 *   tau      T  [B,T,4,3]  out, may be NULL: as mpcqp_joint_log
 *   power    T  [B,T,4]    out, may be NULL: sum_j tau_j qd_j per leg, the mechanical power of the leg's joints in W
 *   reach    u8 [B,T,4]    out, may be NULL: as mpcqp_joint_log
 * At least one output is required; sizes as for mpcqp_joint_log.  q, tau and reach are mpcqp_joint_log's, bit for bit.  The foot's
 * world velocity is foot_vel = v + omega x (foot - CoM) + R J(q) qd, hence
 *   qd = J(q)^-1 R^T (foot_vel - v - omega x (foot - CoM)),
 * the 3x3 system solved by adjugate and determinant.  For a foot at rest power summed over the legs is the rate at which the ground
 * forces work on the body, sum_l f_l . (v + omega x (foot_l - CoM)).  Where reach = 0 or det J = 0 (the straight and the folded
 * knee, the foot on the HipX axis), qd and power are 0.  A non-finite leg as for mpcqp_joint_log; a non-finite omega, v or foot_vel
 * makes qd and power of that leg NaN and leaves q, tau and reach alone.
 */
int mpcqp_joint_rates(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet,
                      const void* foot_vel, const MpcQpLegGeometry* geo, void* q, void* qd, void* tau, void* power, uint8_t* reach,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_JOINTS_H_ */
