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

/*
 * ---- Leg dynamics: the rigid-body dynamics of the three-link leg on a moving torso ----------------------------------------------
 *
 * The joint log above prices a leg's motion at zero: tau = (R J)^T (-f) is the torque of the ground force alone, and a swing leg's is
 * a zero.  The calls below add what moving the 1.16 kg of leg costs -- the reference's controller adds the same terms, an operational-
 * space feed-forward plus the leg's Coriolis and gravity forces, to J^T (-f) for a swing leg (src/main.py:225-282).
 *
 * The inertial row.  Per leg the HIP, THIGH and SHANK link: mass, centre of mass in the link's own frame (origin at its joint, axes
 * of the joint's child frame at q = 0, i.e. the torso's axes) and the inertia tensor about the centre of mass in the link's axes
 * (Ixy etc. are the tensor's elements).  A link that hangs on a fixed joint (the Lite3's FOOT) has to be folded into the row of the
 * link it hangs from.  mpcqp_default_leg_inertia fills in the Lite3: the <inertial> blocks and joint <limit> rows of
 * lite3_urdf/urdf/Lite3.urdf, gravity -9.81, and the FOOT link (0.01 kg, inertia 1e-2 kg m^2 about its own centre, at the foot
 * point (0, 0, -0.21) of the shank frame) folded into the SHANK row by the parallel-axis theorem.  That foot inertia is fifteen
 * times the shank's own; it is the description's model and is kept (DESIGN.md has the shank row with and without it).
 * The row is checked on the host: a non-finite entry, a negative mass, q_min > q_max, a negative qd_max / tau_max, or a gravity that
 * is not negative and finite is MPCQP_EINVAL with the field named in mpcqp_last_error().  All-zero masses and inertias are valid
 * (massless legs: the dynamic torque is then an exact zero).
 *
 * The recursion (Newton-Euler over HipX, HipY, Knee, in the torso's axes; link k turns about the axis z_k through its joint origin
 * p_k, its centre of mass is c_k, its mass m_k and inertia I_k):
 *   outwards  w_k  = w_{k-1} + z_k qd_k,   al_k = al_{k-1} + z_k qdd_k + (w_{k-1} x z_k) qd_k,
 *             a(p_{k+1}) = a(p_k) + al_k x (p_{k+1} - p_k) + w_k x (w_k x (p_{k+1} - p_k)),  likewise a(c_k);  p_4 = the foot point
 *             F_k = m_k (a(c_k) - g),   N_k = I_k al_k + w_k x (I_k w_k)
 *   inwards   f_k = F_k + f_{k+1},   n_k = N_k + (c_k - p_k) x F_k + n_{k+1} + (p_{k+1} - p_k) x f_{k+1},   tau_k = z_k . n_k
 * starting from the torso's w_0, al_0 and a(p_1) = a_0 + al_0 x p_1 + w_0 x (w_0 x p_1).  No foot force enters: the ground's share
 * is the (R J)^T (-f) of the joint log.
 *
 * Not in these two calls: the PD terms of the reference's swing-leg controller -- they need a leg state to form a tracking error,
 * which mpcqp_swing_track below carries; the reaction of the legs on the torso -- the plant's legs stay massless;
 * and the reference's op_space_mi = J*M*J.T, an element-wise product on a block of the mass matrix that is not the leg's:
 * what is computed here is the rigid-body answer, not a copy of that expression.
 */
typedef struct MpcQpLegInertia {
  uint32_t size, reserved;
  double mass[4][3];        /* HIP, THIGH, SHANK link of FL, FR, HL, HR, kg; >= 0 */
  double com[4][3][3];      /* centre of mass in the link's own frame (origin at its joint) */
  double inertia[4][3][6];  /* Ixx, Iyy, Izz, Ixy, Ixz, Iyz about the centre of mass, link axes */
  double q_min[3], q_max[3], qd_max[3], tau_max[3];   /* HipX, HipY, Knee */
  double gravity;           /* negative, m/s^2 */
} MpcQpLegInertia;

/* The Lite3's row (sets size); MPCQP_EINVAL for a null pointer. */
int mpcqp_default_leg_inertia(MpcQpLegInertia* inr);

/*
 * The leg's equations of motion for B rows: tau = M(q) qdd + bias(q, qd, torso motion, gravity).
 *   q       T  [B,4,3]    joint angles HipX, HipY, Knee
 *   qd      T  [B,4,3]    joint rates, NULL = 0
 *   qdd     T  [B,4,3]    joint accelerations, NULL = 0
 *   rot     T  [B,3,3]    torso orientation (world <- torso), NULL = identity
 *   base    T  [B,9]      world-frame angular velocity, angular acceleration and linear acceleration of the torso origin; NULL = the
 *                         torso at rest.  Gravity is inr->gravity along world -z.
 *   geo                   host pointer, NULL = the Lite3.  Any geometry mpcqp_leg_jacobians takes (no closed-form structure needed)
 *   inr                   host pointer, NULL = the Lite3 (mpcqp_default_leg_inertia)
 *   tau     T  [B,4,3]    out, may be NULL: the joint torques that produce qdd (no foot force)
 *   mass    T  [B,4,3,3]  out, may be NULL: the joint-space inertia M(q), row-major; column j is the recursion at a unit qdd_j without
 *                         velocity, torso and gravity terms
 *   bias    T  [B,4,3]    out, may be NULL: tau at qdd = 0
 * At least one output is required.  B = 0 is a no-op; B < 0 or B > 0x1fffffff is MPCQP_EINVAL.  A non-finite operand makes the
 * outputs that depend on it NaN in its own leg (q: its leg; rot, base: the four legs of its row; mass depends on q alone).
 */
int mpcqp_leg_dynamics(mpcqp_handle h, int64_t B, const void* q, const void* qd, const void* qdd, const void* rot, const void* base,
                       const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, void* tau, void* mass, void* bias, void* stream);

/*
 * The full joint torques of a roll-out's log, and whether the actuators could deliver them.
 *   actual, forces, feet, foot_vel, geo   exactly the operands of mpcqp_joint_rates (the closed form's geometry)
 *   foot_acc T  [B,T,4,3]  world acceleration of each foot, or NULL = 0 (the `acc` of mpcqp_phase_swing / mpcqp_swing_trajectories)
 *   base_acc T  [B,T,6]    world-frame angular acceleration of the torso and linear acceleration of the CoM, or NULL = the unpushed
 *                          plant's right-hand side at the row: a = sum_l f_l / m + g e_z, alpha = I_w^-1 (sum_l r_l x f_l - omega x I_w
 *                          omega), I_w = R I_b R^T, r_l = foot_l - CoM, g = inr->gravity.  No contact mask is needed: a swing leg's
 *                          force is an exact zero.  A caller that pushes its robots passes its own.
 *   body     T  [B,7]      as for mpcqp_plant_step (m, Ixx, Iyy, Izz, Ixy, Ixz, Iyz), NULL = the handle's model; read only when
 *                          base_acc is NULL.  An invalid row (the plant's check) makes every output of that robot NaN, limit 0xff.
 *   inr                    host pointer, NULL = the Lite3
 *   qdd      T  [B,T,4,3]  out, may be NULL: joint accelerations in rad / s^2
 *   tau_dyn  T  [B,T,4,3]  out, may be NULL: mpcqp_leg_dynamics' tau at (q, qd, qdd)
 *   tau      T  [B,T,4,3]  out, may be NULL: tau_f + tau_dyn, tau_f = (R J)^T (-f) the tau of mpcqp_joint_rates
 *   power    T  [B,T,4]    out, may be NULL: sum_j tau_j qd_j, formed as mpcqp_joint_rates' power (tau_f . qd) plus tau_dyn . qd
 *   limit    u8 [B,T,4]    out, may be NULL: OR over the leg's three joints of  1: q outside [q_min, q_max],  2: |qd| > qd_max,
 *                          4: |tau| > tau_max;  8: the leg is out of reach (reach = 0)
 * At least one output is required; sizes as for mpcqp_joint_log.  Per (robot, tick, leg): q, qd, tau_f and reach are those of
 * mpcqp_joint_rates (the same device function).  With the CoM standing in for the torso origin, as in the joint log, the foot's
 * world acceleration is
 *   a_foot = a + alpha x r + omega x (omega x r) + 2 omega x u + R (Jdot qd) + R J qdd,     r = foot - CoM,  u = R J qd;
 * everything but the last term is the foot point's acceleration in the forward pass of the recursion at qdd = 0 (with r = R p_foot(q),
 * which is foot - CoM for a leg in reach), and qdd = J^-1 R^T (a_foot - that) by adjugate and determinant as for the rates, of the J
 * the recursion's own chain gives (the shared device function of the joint log is left as it is).  With base_acc NULL the row's
 * sum_l f_l and sum_l r_l x f_l are formed across the four legs as (FL + FR) + (HL + HR).  tau_dyn
 * is the recursion at (q, qd, qdd) with rot = R and base = (omega, alpha, a).  Where reach = 0 or det J = 0: qd = qdd = 0, and tau_dyn
 * is the torque that holds the clamped q on the moving torso.  A non-finite value among the leg's inputs (its row of actual, its
 * force, foot, foot_vel, foot_acc, its row of base_acc -- or, with base_acc NULL, any force or foot of its row and its robot's body)
 * or results makes all five outputs of that leg NaN / 0xff; no other leg changes.
 */
int mpcqp_leg_effort(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet,
                     const void* foot_vel, const void* foot_acc, const void* base_acc, const void* body,
                     const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr,
                     void* qdd, void* tau_dyn, void* tau, void* power, uint8_t* limit, void* stream);

/*
 * ---- The swing leg as a controlled plant --------------------------------------------------------------------------------------
 *
 * mpcqp_leg_effort assumes the leg exactly on its desired trajectory.  The two calls below give the leg a state of its own: its
 * forward dynamics, and the swing legs of a roll-out's log integrated under the reference's swing-leg controller with its PD terms
 * (src/main.py:225-282), so that the foot's actual position, the commanded torque with feedback, its saturation and the landing miss
 * can be read off.  The coupling is one-way: the torso moves as the log says.
 *
 * The leg's forward dynamics for B rows: qdd = M(q)^-1 (tau - bias(q, qd, torso motion, gravity)).
 *   q, qd, rot, base, geo, inr   as for mpcqp_leg_dynamics (qd, rot, base may be NULL)
 *   tau     T  [B,4,3]    the applied joint torques (no foot force)
 *   qdd     T  [B,4,3]    out: joint accelerations in rad / s^2
 *   det     T  [B,4]      out, may be NULL: det M(q)
 * M comes column by column from the recursion at unit accelerations without velocity, torso and gravity terms, bias from the recursion
 * at qdd = 0; the 3x3 system is solved by cofactors and determinant, as the rates solve J.  Massless legs (det M = 0) give qdd = 0.  A
 * non-finite operand makes qdd NaN in its own leg (q, qd, tau: its leg; rot, base: the four legs of its row); det depends on q alone.
 * B = 0 is a no-op; B < 0 or B > 0x1fffffff is MPCQP_EINVAL, as are a null q, tau or qdd.
 */
int mpcqp_leg_accel(mpcqp_handle h, int64_t B, const void* q, const void* qd, const void* tau, const void* rot, const void* base,
                    const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, void* qdd, void* det, void* stream);

/*
 * The swing legs of a roll-out as a controlled plant: one leg state per (robot, leg), carried through the T rows of the log.
 *   actual, forces T [B,T,12], feet_log T [B,T,4,3], contact_log u8 [B,T,4]   as mpcqp_rollout_phase logs them
 *   swing    T  [B,T,4,4,3]  as mpcqp_phase_swing writes it; pos, vel and acc are read.  A stance leg's pos is its held foot and its
 *                            vel and acc are 0 (what mpcqp_phase_swing writes)
 *   base_acc T  [B,T,6]      as for mpcqp_leg_effort, or NULL = the unpushed plant's right-hand side at the row, formed as there over
 *                            the row's forces and the feet the plant held (feet_log), with
 *   body     T  [B,7]        as for mpcqp_leg_effort (NULL = the handle's model; read only when base_acc is NULL)
 *   gains    T  [B,2]        (Kp, Kd) of the Cartesian PD in N / m and N s / m, NULL = 250 and 15 (src/main.py:48-49).  The rows are
 *                            device memory: a negative or non-finite row is not an error, it poisons its robot
 *   state    T  [B,4,7]      in / out, may be NULL: per leg q (3), qd (3), live.  live != 0: q, qd are a swing state to be continued;
 *                            0: the leg starts from its row.  NULL = all live = 0, nothing is written back.  On return it holds the
 *                            state after row T - 1 (live = 1 where that row was a swing row), so a long log can be tracked in pieces
 *   substeps                 control periods per tick, h = delta / substeps; 0 = ceil(delta / h0) (below); < 0 or > 1000: MPCQP_EINVAL
 *   geo, inr                 host pointers, NULL = the Lite3 (the closed form's geometry, as for mpcqp_leg_effort)
 *   q, qd, tau, foot T [B,T,4,3], err T [B,T,4], flag u8 [B,T,4]   out, each may be NULL, at least one required
 * Sizes as for mpcqp_leg_effort; B = 0 or T = 0 is a no-op.
 *
 * Per row and leg.  The on-trajectory state of a row is mpcqp_joint_rates' q, qd at feet = pos, foot_vel = vel.
 *   Stance row (contact != 0): if the incoming state is live this is a landing row: err = |c + R p_foot(q carried) - pos|, the miss
 *     between where the simulated leg put the foot and the foothold the plant used, and flag bit 64.  In every case the state becomes
 *     the on-trajectory state, live = 0; q, qd are that state, tau = (R J)^T (-f) (mpcqp_joint_rates' value, not necessarily its bits),
 *     foot = c + R p_foot(q), and err = |pos - foot| where the row is no landing row.
 *   Swing row, state not live (lift-off, or the first row in mid-swing without a given state): the state becomes the on-trajectory
 *     state of the row, live = 1 (at a lift-off pos is the lift-off foot and vel = 0: the leg starts at rest on the ground); then
 *   Swing row: q, qd = the state at the start of the row, foot = c + R p_foot(q), err = |pos - foot|, tau = the applied torque of the
 *     first control period.  Then `substeps` control periods of h; in period k, s = k h:
 *       torso     c(s) = c + s v + s^2 / 2 a,  v(s) = v + s a,  omega(s) = omega + s alpha  (alpha, a: base_acc); its orientation starts
 *                 from the row's quaternion and takes one Euler step of the plant's quaternion rate at omega(s) per period, renormalised
 *       desired   p_des = pos + s vel + s^2 / 2 acc,  v_des = vel + s acc,  a_des = acc
 *       1  foot = c(s) + R p_foot(q),  foot_vel = v(s) + omega(s) x (R p_foot) + R J qd
 *       2  F = Kp (p_des - foot) + Kd (v_des - foot_vel)
 *       3  bias and the foot point's acceleration af0 from the recursion at (q, qd, qdd = 0) on the torso's (omega(s), alpha, a); M(q)
 *       4  qdd_des = J^-1 (R^T a_des - af0), of the chain's own J; 0 where det J = 0 (flag bit 16)
 *       5  tau_cmd = (R J)^T F + M qdd_des + bias      computed torque: the rigid-body form of the reference's feed-forward
 *       6  tau_app = tau_cmd clamped per joint into [-tau_max, tau_max]  (flag bit 2 where it differs)
 *       7  qdd = M^-1 (tau_app - bias)  (0 where det M = 0)
 *       8  qd += h qdd;  q += h qd       semi-implicit Euler
 *   flag: 1 swing (dynamic) row, 2 some period's torque was clamped, 4 q outside [q_min, q_max] (at the start of some period; on a
 *   stance row: of the logged q), 8 |qd| > qd_max (likewise), 16 det J = 0 in some period or the leg was (re-)initialised out of reach,
 *   64 landing row; 0xff non-finite.
 * A non-finite input of the leg's row (its row of actual, its force, held foot, pos / vel / acc, its row of base_acc -- or, with
 * base_acc NULL, any force or held foot of its row and its robot's body -- its robot's gains, a live state given non-finite) makes
 * that leg's six outputs NaN / 0xff from that row until its next stance row re-initialises it -- the landing row that ends the swing
 * included, whatever the input was: the miss of a poisoned swing is not known; the leg is clean from the row after -- and so does a
 * state that stops being finite; no other leg changes.
 *
 * The clamp is the flat box of the inertia row's tau_max; with an actuator table set (include/mpcqp_actuators.h, mpcqp_set_actuators) it
 * is robot b's torque-speed envelope at the leg state's qd at the start of the control period, and mpcqp_leg_effort's limit bit 4 is
 * tau outside that envelope at the row's qd.
 * Not built: the legs' reaction on the torso, joint-limit stops (a joint beyond its limit is flagged, not stopped) and ground contact
 * of a swing foot (a foot below the ground is not stopped; the landing row's err says where it was).  This call runs after the roll-out,
 * on its logs; mpcqp_rollout_legs (include/mpcqp_sim.h) runs the same row inside the roll-out, tick by tick, and can land a foot where
 * its leg put it.
 *
 * The default control period.  The explicit step is stable only while h lambda < 2, lambda = max eig(M^-1 J^T Kd J).  Measured on the
 * host (lite3_model.swing_gain_lambda) at Kd = 15 over the joint box of the IK and dynamics tests (HipX in [-0.5, 0.5], HipY in
 * [-1.5, -0.2], Knee in [0.5, 2.3], 80 000 legs): lambda = 106.5 / s, so h < 18.8 ms.  h0 is the largest of 2, 1, 0.5, 0.25 ms that is
 * <= 0.5 / lambda = 4.70 ms (the factor 4 is for the Kp term and the torso coupling, which the bound leaves out): h0 = 2 ms, and
 * substeps = 0 means ceil(delta / h0) -- 15 periods at delta = 0.03.  Other gains need their own substeps: lambda scales with Kd.
 */
int mpcqp_swing_track(mpcqp_handle h, int64_t B, int32_t T, const void* actual, const void* forces, const void* feet_log,
                      const uint8_t* contact_log, const void* swing, const void* base_acc, const void* body, const void* gains, void* state,
                      int32_t substeps, const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, void* q, void* qd, void* tau, void* foot,
                      void* err, uint8_t* flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_JOINTS_H_ */
