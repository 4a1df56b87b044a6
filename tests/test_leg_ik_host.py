"""Closed-form leg inverse kinematics on the host (lite3_model.leg_ik_closed, the counterpart of mpcqp_leg_ik in
include/mpcqp_joints.h): round trips through the forward map lite3_model.leg_fk_jac, agreement with the Newton loop
lite3_model.leg_ik where that converges on the same branch, the reach rule and non-finite rows."""
import numpy as np
import pytest

from mpcqp import lite3_model

L1, L2 = 0.20, 0.21
N_ROWS = 4000


@pytest.fixture(scope="module")
def targets():
    """4000 joint vectors over the four legs, drawn from the box HipX +-0.5, HipY -1.5 .. -0.2, Knee 0.5 .. 2.3, restricted to the
    closed form's branch (foot below the HipX axis), and their feet."""
    rng = np.random.default_rng(20251018)
    q = np.stack([rng.uniform(-0.5, 0.5, N_ROWS), rng.uniform(-1.5, -0.2, N_ROWS), rng.uniform(0.5, 2.3, N_ROWS)], axis=1)
    leg = np.arange(N_ROWS) % 4
    keep = L1 * np.cos(q[:, 1]) + L2 * np.cos(q[:, 1] + q[:, 2]) > 0.0
    assert (~keep).mean() < 0.01            # the branch filter cannot hide a failure
    q, leg = q[keep], leg[keep]
    p = np.array([lite3_model.leg_fk_jac(l, x)[0] for l, x in zip(leg, q)])
    return {"q": q, "leg": leg, "p": p}


def _ik_rows(p, leg):
    q = np.empty_like(p); reach = np.empty(len(p), np.uint8)
    for l in range(4):
        q[leg == l], reach[leg == l] = lite3_model.leg_ik_closed(p[leg == l], l)
    return q, reach


def test_ik_of_fk_returns_the_joint_angles(targets):
    """|leg_ik_closed(FK(q)) - q| <= 1e-10: fp64 rounding (1e-16) times the conditioning 1 / (l sin Knee) <~ 25 on this box, with a
    wide margin.  Measured maximum: 2.3e-15 rad."""
    q, reach = _ik_rows(targets["p"], targets["leg"])
    err = np.abs(q - targets["q"]).max()
    print(f"max |IK(FK(q)) - q| = {err:.3e}")
    assert err <= 1e-10
    assert np.all(reach == 1)
    # the four-leg form is the per-leg form
    n = 4 * (len(q) // 4)
    rows = np.stack([targets["p"][:n][targets["leg"][:n] == l][: n // 8] for l in range(4)], axis=1)
    q4, r4 = lite3_model.leg_ik_closed(rows)
    for l in range(4):
        ql, rl = lite3_model.leg_ik_closed(rows[:, l], l)
        assert np.array_equal(q4[:, l], ql) and np.array_equal(r4[:, l], rl)


def test_fk_of_ik_returns_the_foot(targets):
    """|FK(leg_ik_closed(p)) - p| <= 1e-12 m.  Measured maximum: 1.1e-16 m."""
    q, _ = _ik_rows(targets["p"], targets["leg"])
    p = np.array([lite3_model.leg_fk_jac(l, x)[0] for l, x in zip(targets["leg"], q)])
    err = np.abs(p - targets["p"]).max()
    print(f"max |FK(IK(p)) - p| = {err:.3e}")
    assert err <= 1e-12


def test_agrees_with_the_newton_loop_where_that_converges(targets):
    """Where lite3_model.leg_ik ends with an FK residual <= 1e-10 on the closed form's branch it has found the same root, to 1e-8.
    The branch is both of its conditions: a knee angle in (0, pi) AND the foot below the HipX axis, l1 cos HipY + l2 cos(HipY + Knee)
    > 0 (the filter of the round-trip test).  The knee angle alone does not select it: for one knee angle the foot has two HipX
    solutions, (d, z_s) and (d, -z_s) in the HipX link frame, and the Newton loop ends on the second one for a few targets.  Its
    iterate is also not confined to one turn (it ends at HipY + 2 pi on some targets), so HipX and HipY are compared modulo 2 pi.
    At least 95 % of the targets must take part in the comparison."""
    p, leg = targets["p"], targets["leg"]
    qc, _ = _ik_rows(p, leg)
    compared = 0
    for i in range(len(p)):
        qn = lite3_model.leg_ik(int(leg[i]), p[i])
        res = np.abs(lite3_model.leg_fk_jac(int(leg[i]), qn)[0] - p[i]).max()
        if res <= 1e-10 and 0.0 < qn[2] < np.pi and L1 * np.cos(qn[1]) + L2 * np.cos(qn[1] + qn[2]) > 0.0:
            diff = qn - qc[i]
            diff[:2] = (diff[:2] + np.pi) % (2.0 * np.pi) - np.pi
            assert np.abs(diff).max() <= 1e-8
            compared += 1
    print(f"{compared} of {len(p)} targets compared")
    assert compared >= 0.95 * len(p)


def test_reach_and_non_finite_rows():
    hip = lite3_model._HIPX[0] + lite3_model._HIPY[0]
    below = hip + [0.0, 0.0, -0.30]
    q, reach = lite3_model.leg_ik_closed(below, 0)
    assert reach == 1 and np.isfinite(q).all()
    # 0.5 m below the hip: farther than l1 + l2 = 0.41 -> the stretched leg
    q, reach = lite3_model.leg_ik_closed(hip + [0.0, 0.0, -0.5], 0)
    assert reach == 0 and np.isfinite(q).all() and q[2] == 0.0
    # closer than |l1 - l2| -> the folded leg
    q, reach = lite3_model.leg_ik_closed(hip + [0.0, 0.0, -0.005], 0)
    assert reach == 0 and np.isfinite(q).all() and q[2] == np.pi
    # inside the cylinder p_y^2 + p_z^2 < d^2 around the HipX axis
    q, reach = lite3_model.leg_ik_closed(lite3_model._HIPX[0] + [0.05, 0.05, -0.02], 0)
    assert reach == 0 and np.isfinite(q).all()
    for l in range(4):                      # (every leg, the mirrored ones too)
        q, reach = lite3_model.leg_ik_closed(lite3_model._HIPX[l] + [0.0, 0.0, -0.05], l)
        assert reach == 0 and np.isfinite(q).all()
    # a NaN / inf row is NaN and reach 0; its neighbours are what they are without it
    rows = np.stack([below, below + [0.01, 0.0, 0.0], below + [0.0, 0.01, 0.0], below + [0.02, 0.0, 0.01]])
    clean, rclean = lite3_model.leg_ik_closed(rows, 0)
    for bad in (np.nan, np.inf, -np.inf):
        dirty = rows.copy(); dirty[1, 2] = bad
        q, reach = lite3_model.leg_ik_closed(dirty, 0)
        assert np.isnan(q[1]).all() and reach[1] == 0
        assert np.array_equal(q[[0, 2, 3]], clean[[0, 2, 3]]) and np.array_equal(reach[[0, 2, 3]], rclean[[0, 2, 3]])
    with pytest.raises(ValueError):
        lite3_model.leg_ik_closed(np.zeros((5, 3)))


def test_joint_log_host_is_the_per_leg_chain():
    """joint_log_host = rotation vector -> R, leg_ik_closed on R^T (foot - CoM), tau = (R J)^T (-f), leg by leg."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(3)
    B, T = 3, 2
    q = np.stack([rng.uniform(-0.5, 0.5, (B, T, 4)), rng.uniform(-1.5, -0.2, (B, T, 4)), rng.uniform(0.5, 2.0, (B, T, 4))], axis=-1)
    actual = rng.normal(0.0, 0.2, (B, T, 12)); forces = rng.normal(0.0, 30.0, (B, T, 12))
    feet = np.empty((B, T, 4, 3)); want = np.empty((B, T, 4, 3))
    for b in range(B):
        for t in range(T):
            R = Rotation.from_rotvec(actual[b, t, :3]).as_matrix()
            for l in range(4):
                p, J = lite3_model.leg_fk_jac(l, q[b, t, l])
                feet[b, t, l] = actual[b, t, 3:6] + R @ p
                want[b, t, l] = (R @ J).T @ -forces[b, t, 3 * l:3 * l + 3]
    qh, tau, reach = lite3_model.joint_log_host(actual, forces, feet)
    assert np.all(reach == 1) and reach.shape == (B, T, 4) and reach.dtype == np.uint8
    assert np.abs(qh - q).max() <= 1e-10 and np.abs(tau - want).max() <= 1e-9
