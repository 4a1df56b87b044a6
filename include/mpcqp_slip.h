/*
 * mpcqp_slip.h -- extension of include/mpcqp_sim.h: stance feet that slide.
 *
 * mpcqp_rollout_drive (mpcqp_sim.h) scales a stance leg's tangential force onto the ground's Coulomb cone and leaves the foot where it
 * is: the transmitted force is right, the stance geometry is not, and a robot on ice never loses its footing.  The rule here gives each
 * held foot a velocity and lets it slide: an implicit Coulomb time-stepping scheme with one state per foot and one parameter per
 * robot, without a stick / slide mode.  mpcqp_stance_slip is the rule for B robots, mpcqp_rollout_slip the roll-out with the rule in
 * the place of the drive's.
 *
 * The symbols declared here are exported by the product library libmpcqp.so ONLY; the CPU checker library under oracle/ does not have
 * them (the host-side counterparts are lite3_model.stance_slip_host and gaits.rollout_slip_host in the Python package).  Pointers are
 * device memory on the handle's GPU, T is the handle's I/O dtype, work is enqueued on `stream` and nothing is synchronised.  Return
 * codes and mpcqp_last_error() as in mpcqp.h.
 *
 * State and parameter:
 *   slip       double [B,4,2]  the world-frame xy velocity of each held foot [m/s].  fp64 whatever the I/O dtype, for the reason `legs`
 *                              is (mpcqp_sim.h): a state that passes through memory every tick is not rounded on the way.  Zeros:
 *                              every foot is at rest.
 *   foot_mass  T [B]           the effective mass m_e a sliding foot presents [kg]: 1 / mean eig((J M^-1 J^T)_xy) of the leg at its
 *                              stance; lite3_model.foot_mass() gives the Lite3's nominal value, about 0.258 kg.
 *
 * The rule, for one stance leg (contact != 0) with commanded force f, held foot, state x as stored and slip entry s0.  Steps 1 to 3 of
 * mpcqp_stance_drive's rule (mpcqp_sim.h) are unchanged and give tau_app and f1; while an actuator table is set (mpcqp_actuators.h) the
 * envelope's joint rates are those of a foot moving at s0, J^-1 R^T ((s0, 0) - v - omega x (foot - c)), which with s0 = 0 is the drive's
 * rate bit for bit.  Then, with n the plant's `substeps` (0 means 10), h = delta / n, f_n = max(f1_z, 0), cap = (mu_g f_n) (h / m_e)
 * and drv = -f1_xy (h / m_e):
 *   1. s = s0, d = 0, and n times:   s* = s + drv;   s = 0 if |s*| <= cap, else s* (1 - cap / |s*|);   d += h s.
 *      A foot at rest that is commanded inside the cone never moves; a sliding foot is braked by kinetic friction against its velocity
 *      and sticks exactly (s = 0.0, not a small number).
 *   2. the leg is SLIDING (flag bit 128) when s0 != 0 or s_end != 0.
 *   3. the applied force: f2 = 0 on a pull (f1_z <= 0; the foot then coasts under drv with cap = 0).  On a sliding leg
 *      f2_xy = f1_xy + (m_e / delta) (s_end - s0), the tick average of the friction the ground returned, and f2_z = f1_z.  On any other
 *      leg f2 = f1, by a select: the bits are kept.  Bit 32 is set exactly when f2 != f1; tau and the other bits follow step 5 of the
 *      drive's rule.
 *   4. a swing leg (contact == 0): f_out = f bit for bit, tau = 0, flag 0, s = 0, d = 0.
 * Arithmetic is fp64 without contraction; float32 outputs are rounded once.
 * Poison: a foot_mass row that is not finite and positive, or a ground row that is not finite and non-negative, poisons the robot's four
 * legs as a bad ground row poisons them in mpcqp_stance_drive (f_out, tau, slip_out, disp NaN, flag 0xff); a stance leg with a non-finite
 * slip entry, force or foot is poisoned alone.  Nobody else changes.
 *
 * Not built: a reach stop (a foot may slide out of reach, where the IK's reach = 0 and bit 16 apply as in the drive), static versus
 * kinetic friction coefficients, anisotropic foot inertia, a landing foot's residual velocity (a foot lands at rest), the legs' reaction
 * on the torso; the stance rows of the q / qd logs still assume the held foot at rest.
 */
#ifndef MPCQP_SLIP_H_
#define MPCQP_SLIP_H_

#include "mpcqp_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCQP_DRIVE_SLIDING 128   /* the flag bit of a sliding stance leg */

/*
 * The rule alone on the caller's rows.
 *   x, f, feet, contact, geo, inr, f_out, tau, flag   as in mpcqp_stance_drive
 *   ground     T [B]            required
 *   foot_mass  T [B]            required
 *   slip_in    double [B,4,2]   required: s0
 *   substeps                    the n of the rule: the `substeps` of the plant whose tick this is; 0 means 10, outside [0, 1000] is
 *                               MPCQP_EINVAL
 *   slip_out   double [B,4,2]   out, may be NULL, may equal slip_in: s_end (0 on a swing leg)
 *   disp       T [B,4,2]        out, may be NULL: d, how far the foot slid over the tick
 * MPCQP_EINVAL: B negative or above 2^29 - 1, a null x, f, feet, contact, ground, foot_mass, slip_in or f_out (B > 0), substeps out of
 * range, an invalid geo / inr row.  B = 0 is a no-op.
 */
int mpcqp_stance_slip(mpcqp_handle h, int64_t B, const void* x, const void* f, const void* feet, const uint8_t* contact, const void* ground,
                      const void* foot_mass, const double* slip_in, int32_t substeps, const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr,
                      void* f_out, void* tau, uint8_t* flag, double* slip_out, void* disp, void* stream);

/*
 * mpcqp_rollout_drive with the slip rule in the place of the drive's rule.  Every argument of mpcqp_rollout_drive keeps its meaning; the
 * rule's n is the call's `substeps`.
 *   ground     T [B]              required
 *   foot_mass  T [B]              required
 *   slip       double [B,4,2]     in / out, required: state next to x, ref, feet, legs and tick
 *   slip_log   double [B,T,4,2]   out, may be NULL: s0 of the row.  fp64, so that a replay through mpcqp_stance_slip is exact.
 *   disp_log   T [B,T,4,2]        out, may be NULL: what was added to the feet after the row
 * Per tick the rule runs between the solve and the legs step on the live buffers, as the drive's does; the legs step, the plant (whose
 * feet stay fixed over the tick while the applied forces are held), the advance and the landing are mpcqp_rollout_drive's.  After the
 * landing one more launch finishes the row: on stance rows tau_log becomes the rule's tau and flag_log gains its bits 2 / 16 / 32 / 128
 * (0xff for a poisoned leg) under mpcqp_rollout_drive's conditions; every leg that was in stance on the row's tick and does not touch
 * down on the new tick gets feet.xy = (T)((double)feet.xy + d), with d as T holds it, and its slip entry keeps s_end; a leg that touches
 * down gets s = 0; z is never touched.  The MPC reads feet: it is told where its feet are, not that they slide, and the next swing
 * starts from the slid lift-off foot.
 * mpcqp_stance_slip on the logged rows -- x = actual, f = cmd_log, feet_log, contact_log, slip_in = slip_log -- reproduces forces, the
 * stance rows of tau_log, the bits 2 / 16 / 32 / 128 of flag_log and disp_log bit for bit, and its slip_out is the next row's slip_log on
 * a leg that stays in stance.  (Bit 16 of flag_log has a second source on a stance row, as in mpcqp_rollout_drive: the legs step sets it
 * where the held foot is out of reach, which a foot that slides without a reach stop can be.)
 * On a ground that never limits (mu_g = 1e3) no foot moves, and x, ref, feet, legs, tick and every log are mpcqp_rollout_drive's on
 * that ground, bit for bit.
 * Seven launches per tick, with or without logs; no host synchronisation, copy or allocation inside the T ticks (the displacement side
 * buffer is part of the roll-out's reserve).
 * MPCQP_EINVAL: as mpcqp_rollout_drive, and a null ground, foot_mass or slip.  B = 0 or T = 0 is a no-op.
 */
int mpcqp_rollout_slip(mpcqp_handle h, int64_t B, int32_t T, void* x, void* ref, void* feet, double* legs, const int32_t* gait,
                       const void* stand, const void* gain, int32_t* tick, const void* mu, const void* body, const void* push,
                       const int32_t* push_ticks, int32_t substeps, const void* step_height, const void* gains, int32_t leg_substeps,
                       const MpcQpLegGeometry* geo, const MpcQpLegInertia* inr, int32_t land, int32_t drive, const void* ground,
                       const void* foot_mass, double* slip, void* actual, void* desired, void* forces, void* feet_log, uint8_t* contact_log,
                       int32_t* solved, void* swing_log, void* q_log, void* qd_log, void* tau_log, void* foot_log, void* err_log,
                       uint8_t* flag_log, void* miss_log, void* cmd_log, double* slip_log, void* disp_log, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_SLIP_H_ */
