"""Logs with known joint angles, rates AND accelerations, shared by tests/test_leg_dynamics_host.py and tests/test_gpu_leg_dynamics.py:
the construction of rates_cases.known_rate_logs extended with qdd, base_acc and the foot acceleration that results."""
import numpy as np

from mpcqp import lite3_model
from rates_cases import known_rate_logs

JDOT_STEP = 1e-4          # step of the central difference that gives Jdot qd (in s: J is evaluated at q -+ step qd)
MIN_DET = 2e-3            # |det J| of every row of the generator is above this (m^3; asserted below)


def jdot_qd(leg, q, qd, h=JDOT_STEP):
    """d/dt [J(q(t))] qd along q(t) = q + t qd, by the central difference of lite3_model.leg_fk_jac: independent of the recursion."""
    return (lite3_model.leg_fk_jac(leg, q + h * qd)[1] - lite3_model.leg_fk_jac(leg, q - h * qd)[1]) @ qd / (2.0 * h)


def known_effort_logs(B=32, T=4, seed=128, h=JDOT_STEP):
    """known_rate_logs' rows plus joint accelerations up to 40 rad / s^2, a torso acceleration base_acc = (alpha, a) of up to a few
    rad / s^2 and m / s^2, and foot_acc = a + alpha x r + omega x (omega x r) + 2 omega x (R J qd) + R (Jdot qd) + R J qdd with
    r = foot - CoM.  Returns the dict of known_rate_logs with "qdd", "base_acc", "foot_acc" and "min_det" added."""
    s = known_rate_logs(B, T, seed)
    rng = np.random.default_rng(seed + 1)
    qdd = rng.uniform(-40.0, 40.0, (B, T, 4, 3))
    base_acc = np.concatenate([rng.normal(0.0, 3.0, (B, T, 3)), rng.normal(0.0, 2.0, (B, T, 3))], axis=-1)
    R, om = s["R"], s["actual"][..., 6:9]
    r = s["feet"] - s["actual"][:, :, None, 3:6]
    rel = np.empty((B, T, 4, 3)); u = np.empty((B, T, 4, 3)); det = np.empty((B, T, 4))
    for b in range(B):
        for t in range(T):
            for l in range(4):
                q, qd = s["q"][b, t, l], s["qd"][b, t, l]
                J = lite3_model.leg_fk_jac(l, q)[1]
                det[b, t, l] = np.linalg.det(J)
                u[b, t, l] = R[b, t] @ (J @ qd)
                rel[b, t, l] = R[b, t] @ (jdot_qd(l, q, qd, h) + J @ qdd[b, t, l])
    assert np.abs(det).min() > MIN_DET, np.abs(det).min()      # the conditioning of the rows is known
    o, al, a = om[:, :, None], base_acc[:, :, None, 0:3], base_acc[:, :, None, 3:6]
    foot_acc = a + np.cross(al, r) + np.cross(o, np.cross(o, r)) + 2.0 * np.cross(o, u) + rel
    return {**s, "qdd": qdd, "base_acc": base_acc, "foot_acc": foot_acc, "min_det": float(np.abs(det).min())}
