"""Analytic leg kinematics of the Lite3 (geometry data read off lite3_urdf/urdf/Lite3.urdf:44-124 of the reference:
joint origins and axes; no code).  Replaces, for the caller-side torque map, what the reference asks DART for
(`getLinearJacobian(...)[:, 6:9]` etc., src/main.py:205-210).  Legs FL, FR, HL, HR; joints HipX, HipY, Knee.
"""
from __future__ import annotations

import numpy as np

LEGS = ("FL_FOOT", "FR_FOOT", "HL_FOOT", "HR_FOOT")
_HIPX = np.array([[0.1745, 0.062, 0.0], [0.1745, -0.062, 0.0], [-0.1745, 0.062, 0.0], [-0.1745, -0.062, 0.0]])
_HIPY = np.array([[0.0, 0.0985, 0.0], [0.0, -0.0985, 0.0], [0.0, 0.0985, 0.0], [0.0, -0.0985, 0.0]])
_KNEE = np.array([0.0, 0.0, -0.20])
_FOOT = np.array([0.0, 0.0, -0.21])
_AX_X = np.array([-1.0, 0.0, 0.0])      # HipX axis
_AX_Y = np.array([0.0, -1.0, 0.0])      # HipY and Knee axes


def _rot(axis, angle):
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def leg_fk_jac(leg: int, q):
    """Foot position and 3x3 linear Jacobian d p / d q in the torso frame, q = (HipX, HipY, Knee) in rad."""
    R1 = _rot(_AX_X, q[0]); R2 = R1 @ _rot(_AX_Y, q[1]); R3 = R2 @ _rot(_AX_Y, q[2])
    p1 = _HIPX[leg]
    p2 = p1 + R1 @ _HIPY[leg]
    p3 = p2 + R2 @ _KNEE
    pf = p3 + R3 @ _FOOT
    J = np.stack([np.cross(R1 @ _AX_X, pf - p1), np.cross(R2 @ _AX_Y, pf - p2), np.cross(R3 @ _AX_Y, pf - p3)], axis=1)
    return pf, J


def leg_ik(leg: int, p_body, q0=(0.0, -1.0, 1.6), iters=30):
    """Newton inverse kinematics (knee-bent branch selected by the start value)."""
    q = np.array(q0, dtype=float)
    for _ in range(iters):
        p, J = leg_fk_jac(leg, q)
        e = np.asarray(p_body, float) - p
        if np.abs(e).max() < 1e-12:
            break
        q = q + np.linalg.solve(J + 1e-9 * np.eye(3), e)
    return q


def leg_ik_closed(p_body, leg=None):
    """Closed-form inverse of `leg_fk_jac` (the host counterpart of mpcqp_leg_ik, include/mpcqp_joints.h): foot positions in the
    torso frame, [...,4,3] for the four legs or [...,3] with a leg index, -> (q [...,3] HipX, HipY, Knee, reach uint8 [...]).

    The leg is a HipX joint followed by a planar 2R chain: with p = p_body - hip_x and d the lateral HipY offset, the foot in the
    HipX link frame is (p_x, d, z_s), z_s = -sqrt(p_y^2 + p_z^2 - d^2); HipX turns (d, z_s) onto (p_y, p_z), HipY and Knee follow from
    the cosine law in (p_x, z_s).  Branch: foot below the HipX axis (z_s <= 0), knee angle in [0, pi].  Out of reach (reach = 0) the
    square-root argument is clamped at 0 and the cosine at +-1: q is the joint vector of the nearest boundary.  A non-finite row
    gives NaN and reach = 0.  No iteration, no seed."""
    p = np.asarray(p_body, dtype=float)
    if leg is None:
        if p.shape[-2:] != (4, 3):
            raise ValueError(f"p_body must be [...,4,3] (or [...,3] with a leg index), got {p.shape}")
        hx, d = _HIPX, _HIPY[:, 1]
    else:
        if p.shape[-1] != 3:
            raise ValueError(f"p_body must be [...,3], got {p.shape}")
        hx, d = _HIPX[leg], _HIPY[leg, 1]
    sx, sy, l1, l2 = _AX_X[0], _AX_Y[1], -_KNEE[2], -_FOOT[2]
    with np.errstate(invalid="ignore", over="ignore"):
        px, py, pz = p[..., 0] - hx[..., 0], p[..., 1] - hx[..., 1], p[..., 2] - hx[..., 2]
        finite = np.isfinite(px) & np.isfinite(py) & np.isfinite(pz)
        w = py * py + pz * pz - d * d
        ok = w >= 0.0
        zs = -np.sqrt(np.where(ok, w, 0.0))
        a0 = np.arctan2(d * pz - zs * py, d * py + zs * pz)
        r2 = px * px + zs * zs
        r = np.sqrt(r2)
        ok &= (r >= abs(l1 - l2)) & (r <= l1 + l2)
        c = (r2 - l1 * l1 - l2 * l2) / (2.0 * l1 * l2)
        c = np.where(c > 1.0, 1.0, np.where(c < -1.0, -1.0, c))
        k = np.arccos(c)
        s = np.sqrt((1.0 - c) * (1.0 + c))
        u, v = l1 + l2 * c, sy * (l2 * s)                  # the foot seen from the HipY joint, along and across the thigh
        a1 = np.arctan2(zs * v - px * u, -(zs * u + px * v))
        q = np.stack([sx * a0, sy * a1, k], axis=-1)       # (a0, a1: angles about +e_x, +e_y; the knee's is sy * k)
        q = np.where(finite[..., None], q, np.nan)
    return q, (ok & finite).astype(np.uint8)


def joint_log_host(actual, forces, feet):
    """Joint-space log of a roll-out (the host counterpart of mpcqp_joint_log, include/mpcqp_joints.h): actual, forces [B,T,12] as
    the roll-out logs them (actual = rotation vector, CoM, omega, v), feet [B,T,4,3] world foot positions -> (q [B,T,4,3],
    tau [B,T,4,3], reach uint8 [B,T,4]).  Per leg: p = R^T (foot - CoM) with R from the rotation vector, q by `leg_ik_closed`,
    tau = (R J(q))^T (-f) (src/main.py:212-214); the torque is computed from the clamped q where reach = 0."""
    from scipy.spatial.transform import Rotation
    actual, forces, feet = (np.asarray(a, dtype=float) for a in (actual, forces, feet))
    B, T = actual.shape[:2]
    R = Rotation.from_rotvec(actual[..., :3].reshape(-1, 3)).as_matrix().reshape(B, T, 3, 3)
    p = np.einsum("btji,btlj->btli", R, feet - actual[:, :, None, 3:6])
    q, reach = leg_ik_closed(p)
    f = forces.reshape(B, T, 4, 3)
    tau = np.empty((B, T, 4, 3))
    for b in range(B):
        for t in range(T):
            for l in range(4):
                if np.isfinite(q[b, t, l]).all():
                    tau[b, t, l] = (R[b, t] @ leg_fk_jac(l, q[b, t, l])[1]).T @ -f[b, t, l]
                else:
                    tau[b, t, l] = np.nan
    return q, tau, reach


def joint_rates_host(actual, forces, feet, foot_vel=None):
    """`joint_log_host` plus joint rates and power (the host counterpart of mpcqp_joint_rates, include/mpcqp_joints.h): foot_vel
    [B,T,4,3] world foot velocities, None = feet at rest in the world -> (q, qd [B,T,4,3], tau, power [B,T,4], reach).  The foot
    moves with foot_vel = v + omega x (foot - CoM) + R J(q) qd, so qd = J^-1 R^T (foot_vel - v - omega x (foot - CoM)), by adjugate and
    determinant in the device's order; power = sum_j tau_j qd_j.  Out of reach or det J = 0: qd = power = 0; non-finite: NaN."""
    from scipy.spatial.transform import Rotation
    q, tau, reach = joint_log_host(actual, forces, feet)
    actual, feet = np.asarray(actual, dtype=float), np.asarray(feet, dtype=float)
    B, T = actual.shape[:2]
    fv = np.zeros((B, T, 4, 3)) if foot_vel is None else np.asarray(foot_vel, dtype=float)
    R = Rotation.from_rotvec(actual[..., :3].reshape(-1, 3)).as_matrix().reshape(B, T, 3, 3)
    pw = feet - actual[:, :, None, 3:6]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        vrel = (fv - actual[:, :, None, 9:12]) - np.cross(actual[:, :, None, 6:9], pw)
        h = np.einsum("btji,btlj->btli", R, vrel)
        J = np.full((B, T, 4, 3, 3), np.nan)
        for b in range(B):
            for t in range(T):
                for l in range(4):
                    if np.isfinite(q[b, t, l]).all():
                        J[b, t, l] = leg_fk_jac(l, q[b, t, l])[1]
        j = [J[..., a // 3, a % 3] for a in range(9)]
        c = [[j[4] * j[8] - j[5] * j[7], j[5] * j[6] - j[3] * j[8], j[3] * j[7] - j[4] * j[6]],
             [j[2] * j[7] - j[1] * j[8], j[0] * j[8] - j[2] * j[6], j[1] * j[6] - j[0] * j[7]],
             [j[1] * j[5] - j[2] * j[4], j[2] * j[3] - j[0] * j[5], j[0] * j[4] - j[1] * j[3]]]
        det = j[0] * c[0][0] + j[1] * c[0][1] + j[2] * c[0][2]
        qd = np.stack([(c[0][k] * h[..., 0] + c[1][k] * h[..., 1] + c[2][k] * h[..., 2]) / det for k in range(3)], axis=-1)
        move = (reach != 0) & (det != 0.0)
        fin = np.isfinite(q).all(axis=-1) & np.isfinite(vrel).all(axis=-1)
        qd = np.where(fin[..., None], np.where(move[..., None], qd, 0.0), np.nan)
        power = (tau[..., 0] * qd[..., 0] + tau[..., 1] * qd[..., 1]) + tau[..., 2] * qd[..., 2]
        power = np.where(fin, np.where(move, power, 0.0), np.nan)
    return q, qd, tau, power, reach


# ---- leg dynamics (the host counterparts of mpcqp_leg_dynamics / mpcqp_leg_effort, include/mpcqp_joints.h) ------------------------
_BODY = np.array([8.885, 0.24, 1.0, 1.0, 0.0, 0.0, 0.0])   # body = None: MpcQpConfig.m and diag(1 / Ibody_inv) of the default handle


def leg_inertia(fold_foot=True):
    """The Lite3's inertial row and actuator limits as a dict of arrays, the numbers of mpcqp_default_leg_inertia (read off the
    <inertial> blocks and joint <limit> rows of lite3_urdf/urdf/Lite3.urdf; data, no code): mass [4,3] kg, com [4,3,3] m, inertia
    [4,3,6] (Ixx, Iyy, Izz, Ixy, Ixz, Iyz about the centre of mass) of the HIP, THIGH, SHANK link of FL, FR, HL, HR; q_min, q_max,
    qd_max, tau_max [3] of HipX, HipY, Knee; gravity.  The FOOT link (0.01 kg, 1e-2 kg m^2, on a fixed joint at the foot point) is
    folded into the SHANK row by the parallel-axis theorem; fold_foot=False gives the shank's own row."""
    mass, com, inertia = np.zeros((4, 3)), np.zeros((4, 3, 3)), np.zeros((4, 3, 6))
    hip_com = [[-0.0047, -0.0091, -0.0018], [-0.0047, 0.0091, -0.0018], [0.0047, -0.0091, -0.0018], [0.0047, 0.0091, -0.0018]]
    hip_prod = [[8.1579e-07, -1.264e-05, 1.3443e-06], [-8.1551e-07, -1.2639e-05, -1.3441e-06],
                [-8.1585e-07, 1.2639e-05, 1.3444e-06], [8.1545e-07, 1.2639e-05, -1.344e-06]]
    foot_m, foot_i, foot_c = 0.01, 1e-2, [0.0, 0.0, -0.21]
    sm, sc = 0.115, [0.00585, -8.732e-07, -0.12]
    si = [6.68e-04, 6.86e-04, 3.155e-05, -1.24e-08, 6.91e-06, 5.65e-09]
    for l in range(4):
        sy = 1.0 if l % 2 == 0 else -1.0
        mass[l, 0] = 0.428
        com[l, 0] = hip_com[l]
        inertia[l, 0] = [0.00014538, 0.00024024, 0.00013038, *hip_prod[l]]
        mass[l, 1] = 0.61
        com[l, 1] = [-0.00523, -0.0216 * sy, -0.0273]
        inertia[l, 1] = [0.001, 0.00116, 2.68e-04, -2.5e-06 * sy, -1.12e-04, 3.75e-07 * sy]
        if not fold_foot:
            mass[l, 2], com[l, 2], inertia[l, 2] = sm, sc, si
            continue
        m = sm + foot_m
        c = [(sm * sc[a] + foot_m * foot_c[a]) / m for a in range(3)]
        I = [si[a] + (foot_i if a < 3 else 0.0) for a in range(6)]
        for mk, ck in ((sm, sc), (foot_m, foot_c)):
            dx, dy, dz = ck[0] - c[0], ck[1] - c[1], ck[2] - c[2]
            I[0] = I[0] + mk * (dy * dy + dz * dz); I[1] = I[1] + mk * (dx * dx + dz * dz); I[2] = I[2] + mk * (dx * dx + dy * dy)
            I[3] = I[3] - mk * (dx * dy); I[4] = I[4] - mk * (dx * dz); I[5] = I[5] - mk * (dy * dz)
        mass[l, 2], com[l, 2], inertia[l, 2] = m, c, I
    return {"mass": mass, "com": com, "inertia": inertia, "q_min": np.array([-0.42, -2.67, 0.6]), "q_max": np.array([0.42, 0.314, 2.72]),
            "qd_max": np.array([26.0, 26.0, 17.0]), "tau_max": np.array([24.0, 24.0, 36.0]), "gravity": -9.81}


def _rodrigues(a, ang):
    s, c = np.sin(ang), np.cos(ang)
    t = 1.0 - c
    R = [c + t * a[0] * a[0], t * a[0] * a[1] - s * a[2], t * a[0] * a[2] + s * a[1],
         t * a[1] * a[0] + s * a[2], c + t * a[1] * a[1], t * a[1] * a[2] - s * a[0],
         t * a[2] * a[0] - s * a[1], t * a[2] * a[1] + s * a[0], c + t * a[2] * a[2]]
    return np.stack(R, axis=-1).reshape(ang.shape + (3, 3))


def _mv(R, v):
    return np.einsum("...ij,...j->...i", R, v)


def _mtv(R, v):
    return np.einsum("...ji,...j->...i", R, v)


def _leg_chain(q):
    """q [...,4,3] -> link orientations Rl[k] [...,4,3,3] (torso <- HIP, THIGH, SHANK), joint axes z[k] [...,4,3], joint origins and
    foot p[0..3] [...,4,3], all in the torso frame, as `leg_fk_jac` composes them."""
    R1 = _rodrigues(_AX_X, q[..., 0])
    R2 = R1 @ _rodrigues(_AX_Y, q[..., 1])
    R3 = R2 @ _rodrigues(_AX_Y, q[..., 2])
    p1 = np.broadcast_to(_HIPX, q.shape)
    p2 = p1 + _mv(R1, _HIPY)
    p3 = p2 + _mv(R2, _KNEE)
    pf = p3 + _mv(R3, _FOOT)
    return (R1, R2, R3), (_mv(R1, _AX_X), _mv(R2, _AX_Y), _mv(R3, _AX_Y)), (p1, p2, p3, pf)


def _leg_rnea(inr, chain, w0, al0, a0, gb, qd, qdd, vel=True):
    """The recursion of include/mpcqp_joints.h on a chain (csrc/mpcqp_legdyn.h, leg_rnea): torso motion w0, al0, a0 and gravity gb
    in the torso's axes [...,1 or 4,3], qd, qdd [...,4,3] -> (tau [...,4,3], foot acceleration [...,4,3]).  vel=False: M(q) qdd."""
    Rl, z, p = chain
    x = np.cross
    if vel:
        w, al = w0 + 0.0 * p[0], al0 + 0.0 * p[0]
        ap = (a0 + x(al0, p[0])) + x(w0, x(w0, p[0]))
    else:
        w = al = ap = np.zeros_like(p[0])
    F, N, rc, d = [], [], [], []
    for k in range(3):
        if vel:
            al = (al + z[k] * qdd[..., k:k + 1]) + x(w, z[k]) * qd[..., k:k + 1]
            w = w + z[k] * qd[..., k:k + 1]
        else:
            al = al + z[k] * qdd[..., k:k + 1]
        S = inr["inertia"][:, k]
        S = np.stack([S[:, 0], S[:, 3], S[:, 4], S[:, 3], S[:, 1], S[:, 5], S[:, 4], S[:, 5], S[:, 2]], axis=-1).reshape(4, 3, 3)
        Iv = lambda v: _mv(Rl[k], _mv(S, _mtv(Rl[k], v)))
        mk = inr["mass"][:, k][:, None]
        rc.append(_mv(Rl[k], inr["com"][:, k]))
        d.append(p[k + 1] - p[k])
        ac, an, Nk = ap + x(al, rc[k]), ap + x(al, d[k]), Iv(al)
        if vel:
            ac = ac + x(w, x(w, rc[k]))
            an = an + x(w, x(w, d[k]))
            Nk = Nk + x(w, Iv(w))
            F.append(mk * (ac - gb))
        else:
            F.append(mk * ac)
        N.append(Nk)
        ap = an
    f, n, tau = np.zeros_like(ap), np.zeros_like(ap), [None] * 3
    for k in (2, 1, 0):
        n = ((N[k] + x(rc[k], F[k])) + n) + x(d[k], f)
        f = F[k] + f
        tau[k] = (z[k][..., 0] * n[..., 0] + z[k][..., 1] * n[..., 1]) + z[k][..., 2] * n[..., 2]
    return np.stack(tau, axis=-1), ap


def _inertia_arrays(inertia):
    inr = leg_inertia() if inertia is None else inertia
    return {k: (np.asarray(v, dtype=float) if k != "gravity" else float(v)) for k, v in inr.items()}


def leg_dynamics_host(q, qd=None, qdd=None, rot=None, base=None, inertia=None):
    """The leg's equations of motion (the host counterpart of mpcqp_leg_dynamics, include/mpcqp_joints.h): q [B,4,3], qd / qdd
    [B,4,3] or None (0), rot [B,3,3] world <- torso or None, base [B,9] the torso's world-frame angular velocity, angular
    acceleration and linear acceleration of its origin or None (at rest), inertia a dict as `leg_inertia` -> (tau [B,4,3], mass
    [B,4,3,3], bias [B,4,3]): tau = mass qdd + bias, the joint torques without a foot force."""
    inr = _inertia_arrays(inertia)
    q = np.asarray(q, dtype=float)
    qd = np.zeros_like(q) if qd is None else np.asarray(qd, dtype=float)
    qdd = np.zeros_like(q) if qdd is None else np.asarray(qdd, dtype=float)
    B = q.shape[0]
    R = np.broadcast_to(np.eye(3), (B, 3, 3)) if rot is None else np.asarray(rot, dtype=float)
    bw = np.zeros((B, 9)) if base is None else np.asarray(base, dtype=float)
    with np.errstate(invalid="ignore", over="ignore"):
        w0, al0, a0 = (_mtv(R, bw[:, 3 * k:3 * k + 3])[:, None, :] for k in range(3))
        gb = (R[:, 2, :] * inr["gravity"])[:, None, :]
        chain = _leg_chain(q)
        tau = _leg_rnea(inr, chain, w0, al0, a0, gb, qd, qdd)[0]
        bias = _leg_rnea(inr, chain, w0, al0, a0, gb, qd, np.zeros_like(q))[0]
        cols = [_leg_rnea(inr, chain, None, None, None, None, None, np.broadcast_to(np.eye(3)[j], q.shape), vel=False)[0] for j in range(3)]
    return tau, np.stack(cols, axis=-1), bias


def plant_base_acc_host(actual, forces, feet, body=None, gravity=-9.81, wrench=None):
    """What base_acc = None means in `leg_effort_host` / mpcqp_leg_effort: the unpushed plant's right-hand side at every row of a log,
    [B,T,6] = (alpha, a) in world axes; a = sum f / m + g e_z, alpha = R I_b^-1 (R^T sum (foot - CoM) x f - wb x I_b wb), wb = R^T
    omega, in the plant's operation order.  body [B,7] or None (the default handle's model); an invalid row gives NaN.  wrench
    [B,T,6] = (F, tau) or None: the push acting at each row, added to the two sums -- the right-hand side mpcqp_rollout_legs forms."""
    from . import plant
    actual, forces, feet = (np.asarray(a, dtype=float) for a in (actual, forces, feet))
    B, T = actual.shape[:2]
    bd = np.broadcast_to(_BODY, (B, 7)) if body is None else np.asarray(body, dtype=float)
    bd = [np.repeat(bd[:, i][:, None], T, axis=1) for i in range(7)]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Ii, ok = plant.inertia_inverse(bd[0], bd[1:])
        R = plant.quat_to_matrix(plant.rotvec_to_quat(actual[..., 0:3])).reshape(B, T, 9)
        R = [R[..., a] for a in range(9)]
        f = forces.reshape(B, T, 4, 3)
        fk = [[f[:, :, k, a] for a in range(3)] for k in range(4)]
        cr = [plant._cross([feet[:, :, k, a] - actual[..., 3 + a] for a in range(3)], fk[k]) for k in range(4)]
        Fs = [(fk[0][a] + fk[1][a]) + (fk[2][a] + fk[3][a]) for a in range(3)]      # the device's sum across the row's four lanes
        Ms = [(cr[0][a] + cr[1][a]) + (cr[2][a] + cr[3][a]) for a in range(3)]
        if wrench is not None:
            wrench = np.asarray(wrench, dtype=float)
            Fs, Ms = [Fs[a] + wrench[..., a] for a in range(3)], [Ms[a] + wrench[..., 3 + a] for a in range(3)]
        om = [actual[..., 6 + a] for a in range(3)]
        wb = [(R[a] * om[0] + R[3 + a] * om[1]) + R[6 + a] * om[2] for a in range(3)]
        tb = [(R[a] * Ms[0] + R[3 + a] * Ms[1]) + R[6 + a] * Ms[2] for a in range(3)]
        aw = [Fs[a] / bd[0] for a in range(3)]
        aw[2] = aw[2] + gravity
        gy = plant._cross(wb, plant._symv(bd[1:], wb))
        e = plant._symv(Ii, [tb[a] - gy[a] for a in range(3)])
        alw = [(R[3 * a] * e[0] + R[3 * a + 1] * e[1]) + R[3 * a + 2] * e[2] for a in range(3)]
        out = np.stack(alw + aw, axis=-1)
    return np.where(ok[..., None], out, np.nan)


def leg_effort_host(actual, forces, feet, foot_vel=None, foot_acc=None, base_acc=None, body=None, inertia=None, actuators=None):
    """The full joint torques of a roll-out's log (the host counterpart of mpcqp_leg_effort, include/mpcqp_joints.h): the operands of
    `joint_rates_host` plus foot_acc [B,T,4,3] (None = 0), base_acc [B,T,6] world (alpha, a) of the torso / CoM (None =
    `plant_base_acc_host` with `body`) and inertia (a dict as `leg_inertia`) -> {"q", "qd", "tau_f", "reach"} of `joint_rates_host`
    and {"qdd", "tau_dyn", "tau" [B,T,4,3], "power" [B,T,4], "limit" uint8 [B,T,4]}.  qdd = J^-1 (R^T foot_acc - the foot point's
    acceleration in the recursion at qdd = 0) by the rates' adjugate and determinant; tau_dyn = the recursion at (q, qd, qdd);
    tau = tau_f + tau_dyn; power = tau_f . qd + tau_dyn . qd; limit bits 1: q, 2: qd, 4: tau beyond the row's limits, 8: out of
    reach; a non-finite leg: NaN and 0xff.  actuators [B,9] (actuators.py) or None: bit 4 is then tau outside robot b's envelope at the
    row's qd, and a robot with an invalid row gets limit = 0xff."""
    from . import actuators as _act, plant
    inr = _inertia_arrays(inertia)
    q, qd, tau_f, power_f, reach = joint_rates_host(actual, forces, feet, foot_vel)
    actual, forces = np.asarray(actual, dtype=float), np.asarray(forces, dtype=float)
    B, T = actual.shape[:2]
    fa = np.zeros((B, T, 4, 3)) if foot_acc is None else np.asarray(foot_acc, dtype=float)
    if base_acc is None:
        base_acc = plant_base_acc_host(actual, forces, feet, body, inr["gravity"])
    base_acc = np.asarray(base_acc, dtype=float)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        R = plant.quat_to_matrix(plant.rotvec_to_quat(actual[..., 0:3]))
        w0, al0, a0 = (_mtv(R, v)[:, :, None, :] for v in (actual[..., 6:9], base_acc[..., 0:3], base_acc[..., 3:6]))
        gb = (R[..., 2, :] * inr["gravity"])[:, :, None, :]
        chain = _leg_chain(q)
        z, p = chain[1], chain[2]
        J = np.stack([np.cross(z[k], p[3] - p[k]) for k in range(3)], axis=-1)
        j = [J[..., a // 3, a % 3] for a in range(9)]
        c = [[j[4] * j[8] - j[5] * j[7], j[5] * j[6] - j[3] * j[8], j[3] * j[7] - j[4] * j[6]],
             [j[2] * j[7] - j[1] * j[8], j[0] * j[8] - j[2] * j[6], j[1] * j[6] - j[0] * j[7]],
             [j[1] * j[5] - j[2] * j[4], j[2] * j[3] - j[0] * j[5], j[0] * j[4] - j[1] * j[3]]]
        det = j[0] * c[0][0] + j[1] * c[0][1] + j[2] * c[0][2]
        move = (reach != 0) & (det != 0.0)
        af0 = _leg_rnea(inr, chain, w0, al0, a0, gb, qd, np.zeros_like(q))[1]
        h = _mtv(R[:, :, None], fa) - af0
        qdd = np.stack([(c[0][k] * h[..., 0] + c[1][k] * h[..., 1] + c[2][k] * h[..., 2]) / det for k in range(3)], axis=-1)
        qdd = np.where(move[..., None], qdd, 0.0)
        tau_dyn = _leg_rnea(inr, chain, w0, al0, a0, gb, qd, qdd)[0]
        tau = tau_f + tau_dyn
        power = power_f + ((tau_dyn[..., 0] * qd[..., 0] + tau_dyn[..., 1] * qd[..., 1]) + tau_dyn[..., 2] * qd[..., 2])
        fin = np.isfinite(base_acc).all(axis=-1)[:, :, None] & np.isfinite(forces.reshape(B, T, 4, 3)).all(axis=-1)
        for v in (fa, q, qd, qdd, tau_dyn, tau):
            fin = fin & np.isfinite(v).all(axis=-1)
        lim = np.where(reach != 0, 0, 8)
        lim = lim | np.where(((q < inr["q_min"]) | (q > inr["q_max"])).any(axis=-1), 1, 0)
        lim = lim | np.where((np.abs(qd) > inr["qd_max"]).any(axis=-1), 2, 0)
        if actuators is None:
            lim = lim | np.where((np.abs(tau) > inr["tau_max"]).any(axis=-1), 4, 0)
            lim_ok = fin
        else:
            lo, hi = _act.limits_host(actuators, qd)
            lim = lim | np.where(((tau > hi) | (tau < lo)).any(axis=-1), 4, 0)
            lim_ok = fin & _act.valid_rows(actuators)[:, None, None]
    nan3 = lambda v: np.where(fin[..., None], v, np.nan)
    return {"q": q, "qd": qd, "tau_f": tau_f, "reach": reach, "qdd": nan3(qdd), "tau_dyn": nan3(tau_dyn), "tau": nan3(tau),
            "power": np.where(fin, power, np.nan), "limit": np.where(lim_ok, lim, 0xff).astype(np.uint8)}


# ---- the swing leg as a controlled plant (the host counterparts of mpcqp_leg_accel / mpcqp_swing_track, include/mpcqp_joints.h) ----
SWING_KP, SWING_KD = 250.0, 15.0      # gains = None: N / m and N s / m (src/main.py:48-49)
SWING_H0 = 2e-3                       # the default control period in s (include/mpcqp_joints.h has the bound it comes from)
SWING_MAX_SUBSTEPS = 1000
SWING_OUT = ("q", "qd", "tau", "foot", "err", "flag")


def _adj_solve(A, h):
    """x = A^-1 h of 3x3 systems [...,3,3], [...,3] by cofactors and determinant, in the order the rates solve J -> (x, det)."""
    a = [A[..., k // 3, k % 3] for k in range(9)]
    c = [[a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]],
         [a[2] * a[7] - a[1] * a[8], a[0] * a[8] - a[2] * a[6], a[1] * a[6] - a[0] * a[7]],
         [a[1] * a[5] - a[2] * a[4], a[2] * a[3] - a[0] * a[5], a[0] * a[4] - a[1] * a[3]]]
    det = a[0] * c[0][0] + a[1] * c[0][1] + a[2] * c[0][2]
    x = np.stack([(c[0][k] * h[..., 0] + c[1][k] * h[..., 1] + c[2][k] * h[..., 2]) / det for k in range(3)], axis=-1)
    return x, det


def _leg_mass(inr, chain, shape):
    """M(q) [...,4,3,3] of a chain: column j is the recursion at a unit qdd_j without velocity, torso and gravity terms."""
    cols = [_leg_rnea(inr, chain, None, None, None, None, None, np.broadcast_to(np.eye(3)[j], shape), vel=False)[0] for j in range(3)]
    return np.stack(cols, axis=-1)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def leg_accel_host(q, tau, qd=None, rot=None, base=None, inertia=None):
    """The leg's forward dynamics (the host counterpart of mpcqp_leg_accel, include/mpcqp_joints.h): the operands of
    `leg_dynamics_host` with the applied joint torques tau [B,4,3] on the input side -> (qdd [B,4,3], det [B,4] = det M(q));
    qdd = M^-1 (tau - bias) by cofactors and determinant, 0 where det M = 0 (massless legs), NaN in a leg with a non-finite operand."""
    inr = _inertia_arrays(inertia)
    q, tau = np.asarray(q, dtype=float), np.asarray(tau, dtype=float)
    qd = np.zeros_like(q) if qd is None else np.asarray(qd, dtype=float)
    B = q.shape[0]
    R = np.broadcast_to(np.eye(3), (B, 3, 3)) if rot is None else np.asarray(rot, dtype=float)
    bw = np.zeros((B, 9)) if base is None else np.asarray(base, dtype=float)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w0, al0, a0 = (_mtv(R, bw[:, 3 * k:3 * k + 3])[:, None, :] for k in range(3))
        gb = (R[:, 2, :] * inr["gravity"])[:, None, :]
        chain = _leg_chain(q)
        bias = _leg_rnea(inr, chain, w0, al0, a0, gb, qd, np.zeros_like(q))[0]
        x, det = _adj_solve(_leg_mass(inr, chain, q.shape), tau - bias)
        x = np.where((det != 0.0)[..., None], x, 0.0)
        fin = np.isfinite(q).all(axis=-1) & np.isfinite(qd).all(axis=-1) & np.isfinite(tau).all(axis=-1)
        fin = fin & (np.isfinite(R).all(axis=(1, 2)) & np.isfinite(bw).all(axis=1))[:, None] & np.isfinite(x).all(axis=-1)
    return np.where(fin[..., None], x, np.nan), det


def swing_substeps(delta, substeps=0):
    """The number of control periods per tick: `substeps`, or ceil(delta / SWING_H0) for 0 (mpcqp_swing_track's rule)."""
    substeps = int(substeps)
    if substeps < 0 or substeps > SWING_MAX_SUBSTEPS:
        raise ValueError(f"substeps must be in [0, {SWING_MAX_SUBSTEPS}], got {substeps}")
    if substeps:
        return substeps
    n = int(np.ceil(float(delta) / SWING_H0))
    while n > 1 and float(delta) / (n - 1) <= SWING_H0:      # (delta / h0 a whole number up to rounding)
        n -= 1
    return min(max(n, 1), SWING_MAX_SUBSTEPS)


def swing_gain_lambda(q, kd=SWING_KD, inertia=None):
    """max eig(M(q)^-1 J(q)^T kd J(q)) per leg of q [n,4,3]: the stiffness of the damping term that the explicit step has to resolve
    (h lambda < 2)."""
    inr = _inertia_arrays(inertia)
    q = np.asarray(q, dtype=float)
    chain = _leg_chain(q)
    z, p = chain[1], chain[2]
    J = np.stack([np.cross(z[k], p[3] - p[k]) for k in range(3)], axis=-1)
    M = _leg_mass(inr, chain, q.shape)
    A = np.linalg.solve(M, kd * np.einsum("...ki,...kj->...ij", J, J))
    return np.abs(np.linalg.eigvals(A)).max(axis=-1)


def swing_track_host(actual, forces, feet_log, contact_log, swing, base_acc=None, body=None, gains=None, state=None, substeps=0,
                     delta=0.03, inertia=None, actuators=None):
    """The swing legs of a roll-out as a controlled plant (the host counterpart of mpcqp_swing_track, include/mpcqp_joints.h, in the
    device's operation order): actual, forces [B,T,12], feet_log [B,T,4,3], contact_log [B,T,4] as `rollout_phase` logs them, swing
    [B,T,4,4,3] as `phase_swing` writes it, base_acc [B,T,6] or None (`plant_base_acc_host` at feet_log with `body`), gains [B,2] =
    (Kp, Kd) or None (250, 15), state [B,4,7] = (q, qd, live) per leg or None, `substeps` control periods per tick of `delta` s (0:
    `swing_substeps`) -> {"q", "qd", "tau", "foot" [B,T,4,3], "err" [B,T,4], "flag" uint8 [B,T,4], "state" [B,4,7]}.  A stance row
    logs `joint_rates_host`'s q, qd, tau and re-initialises the leg; a swing row logs the carried state, the applied torque of its
    first control period, and integrates the leg under computed torque plus Cartesian PD, clamped at tau_max, over the tick.
    "margin" [B,T,4] (host only) is the row's smallest distance |value - threshold| / max(1, |threshold|) to a joint, rate or torque
    limit over its control periods, to det J = 0 and, where the leg is (re-)initialised, to the reach decision: where it is tiny a rounding difference may flip a flag bit.
    actuators [B,9] (actuators.py, include/mpcqp_actuators.h) or None: each control period then clamps at robot b's envelope at the
    rate the period starts from, not at tau_max, and the margin counts the envelope's comparisons (|qd| at qd_knee and qd_free, the
    commanded torque at lo and hi); a robot with an invalid row logs NaN and 0xff on its swing rows."""
    from . import actuators as _act, plant
    inr = _inertia_arrays(inertia)
    actual, forces, feet_log, swing = (np.asarray(a, dtype=float) for a in (actual, forces, feet_log, swing))
    contact = np.asarray(contact_log)
    B, T = actual.shape[:2]
    n = swing_substeps(delta, substeps)
    h = float(delta) / n
    pos, vel, acc = swing[:, :, :, 0], swing[:, :, :, 1], swing[:, :, :, 2]
    f = forces.reshape(B, T, 4, 3)
    g = inr["gravity"]
    if base_acc is None:
        base_acc = plant_base_acc_host(actual, forces, feet_log, body, g)
    base_acc = np.asarray(base_acc, dtype=float)
    gn = np.broadcast_to(np.array([SWING_KP, SWING_KD]), (B, 2)) if gains is None else np.asarray(gains, dtype=float)
    with np.errstate(invalid="ignore"):
        gain_ok = np.isfinite(gn).all(axis=1) & (gn >= 0.0).all(axis=1)
    kp, kd = gn[:, 0][:, None, None], gn[:, 1][:, None, None]
    if state is None:
        sq, sqd, live = np.zeros((B, 4, 3)), np.zeros((B, 4, 3)), np.zeros((B, 4), bool)
    else:
        state = np.asarray(state, dtype=float)
        sq, sqd = state[:, :, 0:3].copy(), state[:, :, 3:6].copy()
        with np.errstate(invalid="ignore"):
            live = ~(state[:, :, 6] == 0.0)
    bad = live & ~(np.isfinite(sq).all(axis=-1) & np.isfinite(sqd).all(axis=-1))
    if B and T:
        q_on, qd_on, tau_f, _, reach = joint_rates_host(actual, forces, pos, vel)      # the on-trajectory state of every row
    out = {k: np.zeros((B, T, 4, 3)) for k in ("q", "qd", "tau", "foot")}
    out["err"], out["flag"] = np.zeros((B, T, 4)), np.zeros((B, T, 4), np.uint8)
    tmax, zero = inr["tau_max"], np.zeros((B, 4, 3))
    norm = lambda d: np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    limits = lambda q_, qd_: (np.where(((q_ < inr["q_min"]) | (q_ > inr["q_max"])).any(axis=-1), 4, 0)
                              | np.where((np.abs(qd_) > inr["qd_max"]).any(axis=-1), 8, 0))
    rel = lambda val, thr: (np.abs(val - thr) / np.maximum(1.0, np.abs(thr))).min(axis=-1)      # distance to a threshold, per leg
    margins = lambda q_, qd_: np.minimum(np.minimum(rel(q_, inr["q_min"]), rel(q_, inr["q_max"])), rel(np.abs(qd_), inr["qd_max"]))
    out["margin"] = np.full((B, T, 4), np.inf)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t in range(T):
            x = actual[:, t]
            qt = plant.rotvec_to_quat(x[:, 0:3])
            R = plant.quat_to_matrix(qt)
            c, om, v = x[:, None, 3:6], x[:, None, 6:9], x[:, None, 9:12]
            alw, aw = base_acc[:, t, None, 0:3], base_acc[:, t, None, 3:6]
            fin = np.isfinite(x).all(axis=1)[:, None] & np.isfinite(base_acc[:, t]).all(axis=1)[:, None] & gain_ok[:, None]
            for a in (pos[:, t], vel[:, t], acc[:, t], f[:, t], feet_log[:, t]):
                fin = fin & np.isfinite(a).all(axis=-1)
            stance = contact[:, t] != 0
            landing = stance & live
            miss = norm((c + _mv(R[:, None], _leg_chain(sq)[2][3])) - pos[:, t])
            init = stance | ~live
            carried_bad = landing & bad                                            # a poisoned swing ends NaN: its miss is not known
            sq, sqd = np.where(init[..., None], q_on[:, t], sq), np.where(init[..., None], qd_on[:, t], sqd)
            bad = np.where(init, ~fin, bad | ~fin)
            live = ~stance
            bits = np.where(stance, np.where(landing, 64, 0), 1) | np.where(init & (reach[:, t] == 0), 16, 0)
            foot = c + _mv(R[:, None], _leg_chain(sq)[2][3])
            out["q"][:, t], out["qd"][:, t], out["foot"][:, t] = sq, sqd, foot
            out["err"][:, t] = np.where(landing, miss, norm(pos[:, t] - foot))
            bits = bits | np.where(stance, limits(sq, sqd), 0)
            marg = margins(sq, sqd)
            # ... and of the reach decision where the leg was (re-)initialised: the closed form's three comparisons
            pt = _mtv(R[:, None], pos[:, t] - c) - _HIPX
            wr_ = (pt[..., 1] * pt[..., 1] + pt[..., 2] * pt[..., 2]) - _HIPY[:, 1] * _HIPY[:, 1]
            rr_ = np.sqrt(pt[..., 0] * pt[..., 0] + np.maximum(wr_, 0.0))
            l1_, l2_ = -_KNEE[2], -_FOOT[2]
            marg = np.where(init, np.minimum(marg, np.minimum(np.abs(wr_), np.minimum(np.abs(rr_ - abs(l1_ - l2_)), np.abs(rr_ - (l1_ + l2_))))), marg)
            tau_log = tau_f[:, t]
            if live.any():
                dq, dqd, dbits = sq, sqd, np.zeros((B, 4), np.int64)
                Rk = R
                for k in range(n):
                    s = k * h
                    cs, vs, oms = (c + s * v) + (0.5 * s * s) * aw, v + s * aw, om + s * alw
                    pd, vd = (pos[:, t] + s * vel[:, t]) + (0.5 * s * s) * acc[:, t], vel[:, t] + s * acc[:, t]
                    chain = _leg_chain(dq)
                    z, p = chain[1], chain[2]
                    J = np.stack([np.cross(z[j], p[3] - p[j]) for j in range(3)], axis=-1)
                    Rl = Rk[:, None]
                    rp = _mv(Rl, p[3])
                    jq = (J[..., 0] * dqd[..., 0:1] + J[..., 1] * dqd[..., 1:2]) + J[..., 2] * dqd[..., 2:3]
                    fv = (vs + np.cross(oms, rp)) + _mv(Rl, jq)
                    F = kp * (pd - (cs + rp)) + kd * (vd - fv)
                    w0, al0, a0 = _mtv(Rk, oms[:, 0])[:, None], _mtv(Rk, alw[:, 0])[:, None], _mtv(Rk, aw[:, 0])[:, None]
                    gb = (Rk[:, 2, :] * g)[:, None, :]
                    bias, af0 = _leg_rnea(inr, chain, w0, al0, a0, gb, dqd, zero)
                    M = _leg_mass(inr, chain, dq.shape)
                    qdes, detj = _adj_solve(J, _mtv(Rl, acc[:, t]) - af0)
                    qdes = np.where((detj != 0.0)[..., None], qdes, 0.0)
                    gF = _mtv(Rl, F)
                    tff = (M[..., 0] * qdes[..., 0:1] + M[..., 1] * qdes[..., 1:2]) + M[..., 2] * qdes[..., 2:3]
                    cmd = (np.stack([_dot3(J[..., j], gF) for j in range(3)], axis=-1) + tff) + bias
                    if actuators is None:
                        app, mclamp = np.minimum(np.maximum(cmd, -tmax), tmax), rel(np.abs(cmd), tmax)
                    else:
                        app, mclamp = _act.clamp_host(actuators, cmd, dqd), _act.margin_host(actuators, cmd, dqd)
                    qdd, detm = _adj_solve(M, app - bias)
                    qdd = np.where((detm != 0.0)[..., None], qdd, 0.0)
                    dbits = dbits | limits(dq, dqd) | np.where((app != cmd).any(axis=-1), 2, 0) | np.where(detj == 0.0, 16, 0)
                    marg = np.where(live, np.minimum(marg, np.minimum(np.minimum(margins(dq, dqd), mclamp), np.abs(detj))), marg)
                    if k == 0:
                        tau_log = np.where(stance[..., None], tau_log, app)
                    dqd = dqd + h * qdd
                    dq = dq + h * dqd
                    w, qx, qy, qz = qt[:, 0], qt[:, 1], qt[:, 2], qt[:, 3]      # the plant's quaternion rate at omega(s), one Euler step
                    o = oms[:, 0]
                    d = [0.5 * (-((o[:, 0] * qx + o[:, 1] * qy) + o[:, 2] * qz)), 0.5 * (w * o[:, 0] + (o[:, 1] * qz - o[:, 2] * qy)),
                         0.5 * (w * o[:, 1] + (o[:, 2] * qx - o[:, 0] * qz)), 0.5 * (w * o[:, 2] + (o[:, 0] * qy - o[:, 1] * qx))]
                    qt = np.stack([qt[:, i] + h * d[i] for i in range(4)], axis=-1)
                    qt = qt / np.sqrt(((qt[:, 0] * qt[:, 0] + qt[:, 1] * qt[:, 1]) + qt[:, 2] * qt[:, 2]) + qt[:, 3] * qt[:, 3])[:, None]
                    Rk = plant.quat_to_matrix(qt)
                sq, sqd = np.where(live[..., None], dq, sq), np.where(live[..., None], dqd, sqd)
                bits = bits | np.where(live, dbits, 0)
                bad = bad | (live & ~(np.isfinite(sq).all(axis=-1) & np.isfinite(sqd).all(axis=-1)))
            out["tau"][:, t], out["margin"][:, t] = tau_log, marg
            rowbad = bad | carried_bad | ~np.isfinite(tau_log).all(axis=-1) | ~np.isfinite(out["err"][:, t])
            for k in ("q", "qd", "tau", "foot"):
                out[k][:, t] = np.where(rowbad[..., None], np.nan, out[k][:, t])
            out["err"][:, t] = np.where(rowbad, np.nan, out["err"][:, t])
            out["flag"][:, t] = np.where(rowbad, 0xff, bits).astype(np.uint8)
    nan3 = lambda a: np.where(bad[..., None], np.nan, a)
    out["state"] = np.concatenate([nan3(sq), nan3(sqd), live[..., None].astype(float)], axis=-1)
    return out


# ---- the stance drive (the host counterpart of mpcqp_stance_drive, include/mpcqp_sim.h) ---------------------------------------------
DRIVE_CLAMPED, DRIVE_QLIM, DRIVE_UNRESOLVED, DRIVE_GROUND = 2, 4, 16, 32


def _stance_rule(x, f, feet, contact, ground, drive, inertia, actuators, slide=None):
    """The rule of `stance_drive_host` (slide = None: a held foot) and of `stance_slip_host` (slide = (foot_mass, slip, delta, n): a
    foot that slides), numpy in the device's order of operations.  The two differ in the poison terms, the foot velocity behind the
    envelope's rate, step 4, the margin and the "slip" / "disp" outputs; everything else is written once, here."""
    from scipy.spatial.transform import Rotation
    from . import actuators as _act
    inr = _inertia_arrays(inertia)
    x, feet = np.asarray(x, dtype=float), np.asarray(feet, dtype=float)
    B = x.shape[0]
    fr = np.asarray(f, dtype=float).reshape(B, 4, 3)
    stance = np.asarray(contact).reshape(B, 4) != 0
    mu = None if ground is None and slide is None else np.asarray(ground, dtype=float).reshape(B)
    with np.errstate(invalid="ignore"):
        robot = np.isfinite(x[:, :12]).all(axis=1) & (True if mu is None else (np.isfinite(mu) & (mu >= 0.0)))
    leg = np.isfinite(fr).all(axis=-1) & np.isfinite(feet).all(axis=-1)
    if slide is not None:
        me = np.broadcast_to(np.asarray(slide[0], dtype=float), (B,)).copy()
        s0 = np.asarray(slide[1], dtype=float).reshape(B, 4, 2)
        delta, n = float(slide[2]), slide[3]
        with np.errstate(invalid="ignore"):
            robot = robot & np.isfinite(me) & (me > 0.0)
        leg = leg & np.isfinite(s0).all(axis=-1)
    # a poisoned row computes on clean stand-ins and is selected away at the end
    xs = np.where(robot[:, None], x[:, :12], 0.0)
    fs, ps = np.where(leg[..., None], fr, 0.0), np.where(leg[..., None], feet, 0.0)
    mus = np.zeros((B, 1)) if mu is None else np.where(robot, mu, 0.0)[:, None]
    fv = ()       # the held foot is at rest in the world
    if slide is not None:
        ss, mes = np.where(leg[..., None], s0, 0.0), np.where(robot, me, 1.0)[:, None]
        fv = (np.concatenate([ss, np.zeros((B, 4, 1))], axis=-1)[:, None],)
    if actuators is None:
        q, tc, reach = (a[:, 0] for a in joint_log_host(xs[:, None], fs.reshape(B, 1, 12), ps[:, None]))
    else:
        q, rate, tc, _, reach = (a[:, 0] for a in joint_rates_host(xs[:, None], fs.reshape(B, 1, 12), ps[:, None], *fv))
    R = Rotation.from_rotvec(xs[:, :3]).as_matrix()
    tmax = inr["tau_max"]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        z, p = _leg_chain(q)[1:]
        J = np.stack([np.cross(z[k], p[3] - p[k]) for k in range(3)], axis=-1)                  # [B,4,3,3], leg_fk_jac's
        # 2. the actuators
        if drive != "limited":
            ta = tc
        elif actuators is None:
            ta = np.minimum(np.maximum(tc, -tmax), tmax)
        else:
            ta = _act.clamp_host(actuators, tc, rate)
        clamped = (ta != tc).any(axis=-1)
        # 3. the force the applied torque delivers
        g, det = _adj_solve(np.swapaxes(J, -1, -2), ta)                                       # J^-T tau_app
        Rl = R[:, None]
        fc = -np.stack([(Rl[..., a, 0] * g[..., 0] + Rl[..., a, 1] * g[..., 1]) + Rl[..., a, 2] * g[..., 2] for a in range(3)], axis=-1)
        solve = (reach != 0) & (det != 0.0)
        f1 = np.where((clamped & solve)[..., None], fc, fs)
        # 4. the ground
        rel = lambda val, thr: np.abs(val - thr) / np.maximum(1.0, np.abs(thr))
        pull = f1[..., 2] <= 0.0
        if slide is None:      # the held foot: the tangential part on the circular cone with its direction kept
            ft = np.sqrt(f1[..., 0] * f1[..., 0] + f1[..., 1] * f1[..., 1])
            cap = mus * f1[..., 2]
            cone = (ft > cap) if mu is not None else np.zeros((B, 4), bool)
            s = cap / ft
            f2 = np.stack([np.where(cone, f1[..., 0] * s, f1[..., 0]), np.where(cone, f1[..., 1] * s, f1[..., 1]), f1[..., 2]], axis=-1)
        else:                  # the slide
            h = delta / n
            fn = np.where(pull, 0.0, f1[..., 2])
            hm = h / mes
            cap = (mus * fn) * hm
            vx, vy = -f1[..., 0] * hm, -f1[..., 1] * hm
            sx, sy = ss[..., 0].copy(), ss[..., 1].copy()
            dx, dy = np.zeros((B, 4)), np.zeros((B, 4))
            slide_margin = np.full((B, 4), np.inf)
            for _ in range(n):
                tx, ty = sx + vx, sy + vy
                nrm = np.sqrt(tx * tx + ty * ty)
                stick = nrm <= cap
                # (cap = 0 -- a pull, or ice -- is an exact zero on both sides: |s*| <= 0 is then decided by exact zeros too)
                slide_margin = np.minimum(slide_margin, np.where(cap == 0.0, np.inf, rel(nrm, cap)))
                keep = 1.0 - cap / nrm
                sx, sy = np.where(stick, 0.0, tx * keep), np.where(stick, 0.0, ty * keep)
                dx, dy = dx + h * sx, dy + h * sy
            sliding = (ss[..., 0] != 0.0) | (ss[..., 1] != 0.0) | (sx != 0.0) | (sy != 0.0)
            med = mes / delta
            f2 = np.stack([np.where(sliding, f1[..., 0] + med * (sx - ss[..., 0]), f1[..., 0]),
                           np.where(sliding, f1[..., 1] + med * (sy - ss[..., 1]), f1[..., 1]), f1[..., 2]], axis=-1)
        f2 = np.where(pull[..., None], 0.0, f2)
        limited = (f2 != f1).any(axis=-1)
        fo = np.where(limited[..., None], f2, f1)
        # 5. the torque that goes with it
        h5 = -np.stack([(Rl[..., 0, a] * f2[..., 0] + Rl[..., 1, a] * f2[..., 1]) + Rl[..., 2, a] * f2[..., 2] for a in range(3)], axis=-1)
        tg = np.stack([(J[..., 0, j] * h5[..., 0] + J[..., 1, j] * h5[..., 1]) + J[..., 2, j] * h5[..., 2] for j in range(3)], axis=-1)
        to = np.where(limited[..., None], tg, ta)
        bits = (np.where(clamped, DRIVE_CLAMPED, 0) | np.where(clamped & ~solve, DRIVE_UNRESOLVED, 0) | np.where(limited, DRIVE_GROUND, 0)
                | np.where(((q < inr["q_min"]) | (q > inr["q_max"])).any(axis=-1), DRIVE_QLIM, 0))
        margin = np.full((B, 4), np.inf)
        if drive == "limited":
            margin = rel(np.abs(tc), tmax).min(axis=-1) if actuators is None else _act.margin_host(actuators, tc, rate)
        # an unclamped leg's f1 is f as read and its ground decisions are exact comparisons of correctly rounded operations: only a
        # clamped leg's computed f1 can fall on the other side of them.  The stick decisions compare computed values on every leg.
        ground_margin = rel(f1[..., 2], 0.0)
        if slide is None and mu is not None:
            ground_margin = np.minimum(ground_margin, np.where(pull, np.inf, rel(ft, cap)))
        margin = np.where(clamped & solve, np.minimum(margin, ground_margin), margin)
        own = leg & np.isfinite(fo).all(axis=-1) & np.isfinite(to).all(axis=-1)
        if slide is not None:
            bits = bits | np.where(sliding, DRIVE_SLIDING, 0)
            margin = np.minimum(margin, slide_margin)
            own = own & np.isfinite(sx) & np.isfinite(sy) & np.isfinite(dx) & np.isfinite(dy)
        good = robot[:, None] & (~stance | own)
    st3 = stance[..., None]
    sel = lambda a, off: np.where(good[..., None], np.where(st3, a, off), np.nan)
    out = {"f": sel(fo, fr).reshape(B, 12), "tau": sel(to, 0.0), "flag": np.where(good, np.where(stance, bits, 0), 0xff).astype(np.uint8)}
    if slide is not None:
        out["slip"], out["disp"] = sel(np.stack([sx, sy], axis=-1), 0.0), sel(np.stack([dx, dy], axis=-1), 0.0)
    out.update({"tau_cmd": np.where((good & stance)[..., None], tc, np.nan), "q": q, "reach": reach,
                "margin": np.where(good & stance, margin, np.inf)})
    if actuators is not None:
        out["rate"] = rate
    return out


def stance_drive_host(x, f, feet, contact, ground=None, drive="limited", inertia=None, actuators=None):
    """What the stance legs deliver of a commanded force (the host counterpart of mpcqp_stance_drive, include/mpcqp_sim.h, which has the
    rule; numpy in the device's order of operations): x [B,>=12] as stored, f [B,12] or [B,4,3] the commanded forces, feet [B,4,3] the
    held feet, contact [B,4], ground [B] the ground's friction coefficient or None (no friction limit; a foot still cannot pull),
    drive "limited" or "ideal" (the torque clamp is skipped: what mpcqp_rollout_drive does under MPCQP_DRIVE_IDEAL), inertia a dict as
    `leg_inertia` (tau_max, q_min, q_max are read) -> {"f": [B,12] applied forces, "tau": [B,4,3] applied torques, "flag": uint8 [B,4]
    (2 clamped, 4 q outside its limits, 16 clamped but not resolvable, 32 the ground limited the force, 0xff a non-finite leg),
    "tau_cmd": [B,4,3] = `joint_log_host`'s torque, "q": [B,4,3], "reach": uint8 [B,4], "margin": [B,4] (host only) the smallest
    distance |value - threshold| / max(1, |threshold|) of a stance leg to a threshold that decides a bit or a branch: |tau_cmd| at
    tau_max and, for a clamped leg, whose f1 is computed, f1_z at 0 and the tangential force at the cone -- where it is tiny a
    rounding difference may flip the decision}.
    tau_cmd = (R J)^T (-f) is `joint_log_host`'s; clamped legs get f1 = -R (J^-T tau_app) by `_adj_solve` on J^T.  The held foot does
    not move (`stance_slip_host` lets it slide).
    actuators [B,9] (actuators.py, include/mpcqp_actuators.h) or None: the clamp is then robot b's envelope at "rate" [B,4,3] (an extra
    key of the result), `joint_rates_host`'s joint rate with the foot at rest in the world, and the margin counts the envelope's
    comparisons; drive "ideal" does not read the table; a robot with an invalid row gets NaN and 0xff on its stance legs."""
    if drive not in ("limited", "ideal"):
        raise ValueError(f"drive must be 'ideal' or 'limited', got {drive!r}")
    return _stance_rule(x, f, feet, contact, ground, drive, inertia, actuators)


# ---- stance feet that slide (the host counterpart of mpcqp_stance_slip, include/mpcqp_slip.h) ----------------------------------------
DRIVE_SLIDING = 128


def foot_mass(inertia=None):
    """The effective mass m_e [kg] a sliding foot presents (include/mpcqp_slip.h): 1 / mean eig((J M^-1 J^T)_xy) over the four legs at
    the nominal stance (synth.NOMINAL_FEET seen from the CoM, torso level), M the leg's joint-space mass matrix of `leg_dynamics_host`
    with the row `inertia` (None: the Lite3's, about 0.258 kg)."""
    from .synth import NOMINAL_FEET
    q, reach = leg_ik_closed(NOMINAL_FEET[None])
    assert reach.all()
    M = leg_dynamics_host(q, inertia=inertia)[1][0]
    eig = []
    for l in range(4):
        J = leg_fk_jac(l, q[0, l])[1]
        eig.extend(np.linalg.eigvalsh((J @ np.linalg.solve(M[l], J.T))[:2, :2]))
    return float(1.0 / np.mean(eig))


def stance_slip_host(x, f, feet, contact, ground, foot_mass, slip, drive="limited", inertia=None, actuators=None, delta=0.03, substeps=10):
    """`stance_drive_host` with stance feet that slide (the host counterpart of mpcqp_stance_slip, include/mpcqp_slip.h, which has the
    rule; numpy in the device's order of operations): x, f, feet, contact, drive, inertia, actuators as for `stance_drive_host`; ground
    [B] the ground's friction coefficient and foot_mass [B] (or a number) the feet's effective mass, both required; slip [B,4,2] the
    world xy velocity of each held foot at the start of the tick; delta the tick and `substeps` the plant's substeps (0 means 10) ->
    `stance_drive_host`'s dict with flag bit 128 = the foot slides, plus "slip" [B,4,2] the velocities at the end of the tick (0 on a
    swing leg) and "disp" [B,4,2] how far each foot slid.  With actuators the envelope's rate is that of a foot moving at `slip`.
    "margin" [B,4] (host only) also covers, for every leg, the |s*| versus cap decision of each substep, and the ground's decisions
    no longer (the rule has no cone scaling; f1_z at 0 stays, for a clamped leg)."""
    if drive not in ("limited", "ideal"):
        raise ValueError(f"drive must be 'ideal' or 'limited', got {drive!r}")
    n = 10 if int(substeps) == 0 else int(substeps)
    if not 1 <= n <= 1000:
        raise ValueError(f"substeps must be in [0, 1000], got {substeps}")
    return _stance_rule(x, f, feet, contact, ground, drive, inertia, actuators, (foot_mass, slip, delta, n))


def world_jacobians(R_body, q_all):
    """{leg: 3x3 world-frame linear Jacobian block} for joint angles q_all[4,3] (src/main.py:205-210)."""
    return {LEGS[k]: R_body @ leg_fk_jac(k, q_all[k])[1] for k in range(4)}
