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


def world_jacobians(R_body, q_all):
    """{leg: 3x3 world-frame linear Jacobian block} for joint angles q_all[4,3] (src/main.py:205-210)."""
    return {LEGS[k]: R_body @ leg_fk_jac(k, q_all[k])[1] for k in range(4)}
