"""Logs with known joint angles and joint rates, shared by tests/test_joint_rates_host.py and tests/test_gpu_joint_rates.py."""
import numpy as np

from mpcqp import lite3_model

L1, L2 = 0.20, 0.21


def known_rate_logs(B=32, T=4, seed=128):
    """B T rows: joint angles on the box of the IK tests (HipX +-0.5, HipY -1.5 .. -0.2, Knee 0.5 .. 2.3; the few draws off the
    closed form's branch, foot above the HipX axis, are put back at (0, -1, 1.6)), joint rates up to 3 rad / s, random body twists
    and forces; row (0, 0) has |theta| < 1e-6 (the series range of the rotation-vector conversion), row (0, 1) none, row (1, 0) an
    angle of 1 rad.  feet = CoM + R FK(q) and foot_vel = v + omega x (foot - CoM) + R J(q) qd."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    q = np.stack([rng.uniform(-0.5, 0.5, (B, T, 4)), rng.uniform(-1.5, -0.2, (B, T, 4)), rng.uniform(0.5, 2.3, (B, T, 4))], axis=-1)
    off = L1 * np.cos(q[..., 1]) + L2 * np.cos(q[..., 1] + q[..., 2]) <= 0.0
    q[off] = [0.0, -1.0, 1.6]
    qd = rng.uniform(-3.0, 3.0, (B, T, 4, 3))
    actual = np.zeros((B, T, 12))
    actual[..., 0:3] = rng.normal(0.0, 0.15, (B, T, 3))
    actual[0, 0, 0:3] = [3e-7, -2e-7, 5e-7]
    actual[0, 1, 0:3] = 0.0
    actual[1, 0, 0:3] = np.array([0.6, -0.5, 0.62]) * (1.0 / np.linalg.norm([0.6, -0.5, 0.62]))
    actual[..., 3:6] = rng.normal(0.0, 0.5, (B, T, 3)) + [0.0, 0.0, 0.285]
    actual[..., 6:9] = rng.normal(0.0, 1.0, (B, T, 3))
    actual[..., 9:12] = rng.normal(0.0, 0.5, (B, T, 3))
    forces = rng.normal(0.0, 30.0, (B, T, 12))
    R = Rotation.from_rotvec(actual[..., :3].reshape(-1, 3)).as_matrix().reshape(B, T, 3, 3)
    p = np.empty((B, T, 4, 3)); Jq = np.empty((B, T, 4, 3))
    for b in range(B):
        for t in range(T):
            for l in range(4):
                p[b, t, l], J = lite3_model.leg_fk_jac(l, q[b, t, l])
                Jq[b, t, l] = J @ qd[b, t, l]
    r = np.einsum("btij,btlj->btli", R, p)
    feet = actual[:, :, None, 3:6] + r
    foot_vel = actual[:, :, None, 9:12] + np.cross(actual[:, :, None, 6:9], r) + np.einsum("btij,btlj->btli", R, Jq)
    return {"q": q, "qd": qd, "actual": actual, "forces": forces, "feet": feet, "foot_vel": foot_vel, "R": R}
