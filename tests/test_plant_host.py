"""Host checker of the rigid-body plant (include/mpcqp_sim.h; mpcqp.plant): the physics it claims, its integration order, its
rotation conversions and its conventions, plus the C interface's symbol set.  No GPU: the device is held to this checker in
tests/test_gpu_plant.py."""
import os
import re

import numpy as np
import pytest

import mpcqp
from conftest import REPO
from mpcqp.plant import (model_body, push_wrench, quat_to_matrix, quat_to_rotvec, rollout_plant_host, rotvec_to_quat, srb_step,
                         stance_feet)

M, IBODY_INV = 8.885, (1.0 / 0.24, 1.0, 1.0)
I_ASYM = np.array([[0.24, 0.02, -0.01], [0.02, 1.0, 0.03], [-0.01, 0.03, 1.3]])


def _body(m, I):
    return np.array([[m, I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]])


def _spin_state(omega, theta=(0.3, -0.2, 0.5), g=0.0):
    x = np.zeros((1, 13))
    x[0, 0:3] = theta; x[0, 3:6] = (0.1, -0.2, 0.3); x[0, 6:9] = omega; x[0, 9:12] = (0.2, 0.0, -0.1); x[0, 12] = g
    return x


def _momentum_energy(x, I):
    R = quat_to_matrix(rotvec_to_quat(x[:, 0:3]))[0]
    Iw = R @ I @ R.T
    w = x[0, 6:9]
    return Iw @ w, 0.5 * w @ Iw @ w


def test_torque_free_asymmetric_body_conserves_momentum_and_energy():
    """g = 0, no forces, an asymmetric inertia with products of inertia, about 3 rad/s about a non-principal axis: the world
    angular momentum R I_b R^T omega and the kinetic energy stay put over 100 ticks, while omega itself tumbles (the gyroscopic
    term the MPC drops)."""
    x = _spin_state(np.array([2.0, -1.5, 1.6]))
    f, feet, ct = np.zeros((1, 12)), np.zeros((1, 4, 3)), np.zeros((1, 4), np.uint8)
    L0, E0 = _momentum_energy(x, I_ASYM)
    w0 = x[0, 6:9].copy()
    dL = dE = 0.0
    for _ in range(100):
        x = srb_step(x, f, feet, ct, _body(M, I_ASYM), None, 0.03, 10)
        L, E = _momentum_energy(x, I_ASYM)
        dL = max(dL, np.abs(L - L0).max() / np.linalg.norm(L0)); dE = max(dE, abs(E - E0) / E0)
    assert np.abs(x[0, 6:9] - w0).max() > 0.1
    assert dL <= 1e-9 and dE <= 1e-9, (dL, dE)
    assert np.linalg.norm(x[0, 0:3]) <= np.pi


def test_constant_force_without_rotation_is_the_closed_form_quadratic():
    """omega = 0, constant stance forces and a push force: p and v are the closed-form quadratic to 1e-12 (RK4 is exact on it)."""
    x = _spin_state(np.zeros(3), theta=(0.0, 0.0, 0.0), g=-9.81)
    x[0, 3:6] = 0.0
    f = np.array([[1.0, 2.0, 20.0, -3.0, 1.0, 25.0, 0.5, 0.5, 22.0, 2.0, -1.0, 24.0]])
    feet = np.zeros((1, 4, 3)); ct = np.ones((1, 4), np.uint8)   # feet under the CoM: no torque, omega stays 0
    wr = np.array([[5.0, -4.0, 1.0, 0.0, 0.0, 0.0]])
    a = (f.reshape(4, 3).sum(axis=0) + wr[0, :3]) / M + np.array([0.0, 0.0, -9.81])
    p0, v0 = x[0, 3:6].copy(), x[0, 9:12].copy()
    t = 0.0
    for _ in range(5):
        x = srb_step(x, f, feet, ct, _body(M, np.diag(1.0 / np.asarray(IBODY_INV))), wr, 0.03, 7)
        t += 0.03
        assert np.abs(x[0, 3:6] - (p0 + v0 * t + 0.5 * a * t * t)).max() <= 1e-12
        assert np.abs(x[0, 9:12] - (v0 + a * t)).max() <= 1e-12


def _rhs(body, f, feet, wrench, g):
    """The plant's equations in rotation-matrix form, for an independent integrator."""
    m = body[0, 0]
    I = np.array([[body[0, 1], body[0, 4], body[0, 5]], [body[0, 4], body[0, 2], body[0, 6]], [body[0, 5], body[0, 6], body[0, 3]]])
    F = f.reshape(4, 3); r = feet.reshape(4, 3)

    def rhs(_, s):
        R, p, w = s[0:9].reshape(3, 3), s[9:12], s[12:15]
        Iw = R @ I @ R.T
        tau = sum(np.cross(r[l] - p, F[l]) for l in range(4)) + wrench[3:]
        dw = np.linalg.solve(Iw, tau - np.cross(w, Iw @ w))
        W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        dv = (F.sum(axis=0) + wrench[:3]) / m + np.array([0.0, 0.0, g])
        return np.concatenate([(W @ R).ravel(), s[15:18], dw, dv])
    return rhs


def test_rk4_is_fourth_order_against_an_adaptive_reference():
    """A spinning body on stance forces over one tick: the error against solve_ivp (rtol 1e-12) falls by more than 10x each time the
    substeps double."""
    from scipy.integrate import solve_ivp
    from scipy.spatial.transform import Rotation
    x = _spin_state(np.array([4.0, -3.0, 5.0]), g=-9.81)
    f = np.array([[2.0, 1.0, 25.0, -1.0, 2.0, 20.0, 0.0, -2.0, 23.0, 1.0, 1.0, 21.0]])
    feet = np.array([[[0.2, 0.1, 0.0], [0.2, -0.15, 0.0], [-0.2, 0.12, 0.0], [-0.18, -0.1, 0.0]]])
    wr = np.array([3.0, -2.0, 0.0, 0.5, 0.2, -0.3])
    body = _body(M, I_ASYM)
    delta = 0.1
    s0 = np.concatenate([Rotation.from_rotvec(x[0, 0:3]).as_matrix().ravel(), x[0, 3:6], x[0, 6:9], x[0, 9:12]])
    ref = solve_ivp(_rhs(body, f, feet, wr, -9.81), (0.0, delta), s0, method="DOP853", rtol=1e-12, atol=1e-14).y[:, -1]
    ref_x = np.concatenate([Rotation.from_matrix(ref[0:9].reshape(3, 3)).as_rotvec(), ref[9:12], ref[12:15], ref[15:18]])
    errs = [np.abs(srb_step(x, f, feet, np.ones((1, 4), np.uint8), body, wr[None], delta, n)[0, :12] - ref_x).max() for n in (2, 4, 8)]
    assert errs[0] / errs[1] > 10 and errs[1] / errs[2] > 10, errs
    assert errs[2] < 1e-4, errs


@pytest.mark.parametrize("angle", [1e-14, 1e-6, 1.0, np.pi - 1e-9])
def test_rotation_vector_quaternion_round_trips_match_scipy(angle):
    from scipy.spatial.transform import Rotation
    axes = np.random.default_rng(3).normal(size=(16, 3))
    th = axes / np.linalg.norm(axes, axis=1, keepdims=True) * angle
    q = rotvec_to_quat(th)
    qs = Rotation.from_rotvec(th).as_quat()                       # (x, y, z, w), w >= 0 for |theta| <= pi
    assert np.abs(q - np.concatenate([qs[:, 3:], qs[:, :3]], axis=1)).max() <= 2e-16
    tol = 4e-16 * max(1.0, angle)
    back = quat_to_rotvec(q)
    assert np.abs(back - th).max() <= tol * 4
    assert np.abs(back - Rotation.from_quat(qs).as_rotvec()).max() <= tol * 4
    assert np.abs(quat_to_rotvec(-q) - back).max() <= tol * 4     # either sign of q is the same rotation, |theta| <= pi


def test_model_body_is_the_engines_model_and_invalid_rows_give_nan():
    """body = None means (cfg.m, diag(1 / Ibody_inv)); a row with m <= 0, a non-finite entry or an inertia that is not positive
    definite gives NaN in x[0..11] with x[12] kept, and leaves the other robots as they are."""
    x = np.repeat(_spin_state(np.array([0.5, -0.3, 0.2]), g=-9.81), 6, axis=0)
    f = np.tile([0.0, 0.0, 21.0], (6, 4)); feet = np.zeros((6, 4, 3)); ct = np.ones((6, 4), np.uint8)
    cfg = mpcqp.product_library().default_config(N=10, delta=0.03)
    body = np.tile([cfg.m, 1.0 / cfg.Ibody_inv[0], 1.0 / cfg.Ibody_inv[1], 1.0 / cfg.Ibody_inv[2], 0.0, 0.0, 0.0], (6, 1))
    assert np.array_equal(model_body(cfg.m, list(cfg.Ibody_inv), 6), body) and cfg.m == M
    good = srb_step(x, f, feet, ct, body, None, 0.03, 10)
    body[1, 0] = 0.0                                              # m <= 0
    body[2, 5] = np.inf                                           # non-finite
    body[3, 4] = 0.5                                              # Ixx Iyy - Ixy^2 < 0
    body[4, 4:7] = (0.0, 0.0, 1.0)                                # det < 0 with the leading 2x2 minor positive
    out = srb_step(x, f, feet, ct, body, None, 0.03, 10)
    assert np.array_equal(out[[0, 5]], good[[0, 5]])
    assert np.all(np.isnan(out[1:5, :12])) and np.all(out[:, 12] == -9.81)


def test_swing_legs_carry_nothing_and_substeps_are_checked():
    x = _spin_state(np.array([0.5, -0.3, 0.2]), g=-9.81)
    f = np.array([[0.0, 0.0, 30.0, np.nan, 1e9, 3.0, 0.0, 0.0, 30.0, 0.0, 0.0, 30.0]])
    feet = np.array([[[0.2, 0.1, 0.0], [np.inf, 0.0, 0.0], [-0.2, 0.1, 0.0], [-0.2, -0.1, 0.0]]])
    ct = np.array([[1, 0, 1, 1]], np.uint8)
    body = model_body(M, IBODY_INV)
    a = srb_step(x, f, feet, ct, body, None, 0.03, 10)
    f2, feet2 = f.copy(), feet.copy()
    f2[0, 3:6] = 0.0; feet2[0, 1] = 0.0
    assert np.all(np.isfinite(a)) and np.array_equal(a, srb_step(x, f2, feet2, ct, body, None, 0.03, 10))
    assert np.array_equal(srb_step(x, f, feet, ct, body, None, 0.03, 0), a)   # 0 means 10
    for bad in (-1, 1001):
        with pytest.raises(ValueError, match="substeps"):
            srb_step(x, f, feet, ct, body, None, 0.03, bad)


def test_stance_rule_and_push_window():
    rb = mpcqp.synth.make_rollout_batch(3, total_steps=5, seed=11)   # ss 4, ds 2
    feet, ct = stance_feet(rb["plan_pos"], rb["plan_feet_id"], rb["plan_meta"], np.array([0, 5, 100], np.int32))
    assert np.all(ct == 1)                                        # step 0, double support, past the plan
    assert np.array_equal(feet[2], rb["plan_pos"][2, 4])
    feet, ct = stance_feet(rb["plan_pos"], rb["plan_feet_id"], rb["plan_meta"], np.array([6, 7, 9], np.int32))
    assert np.array_equal(ct, rb["plan_feet_id"][:, 1].astype(np.uint8)) and np.array_equal(feet, rb["plan_pos"][:, 1])
    push = np.arange(18, dtype=float).reshape(3, 6)
    w = push_wrench(push, np.array([[2, 4], [0, 1], [3, 3]], np.int32), np.array([3, 1, 3], np.int32))
    assert np.array_equal(w[0], push[0]) and not w[1].any() and not w[2].any()


def test_rollout_plant_host_shares_the_first_solve_and_departs_from_the_model(oracle_lib):
    """Tick 0 solves from the same state as the kinematic roll-out (identical log rows); from then on the plant, not X[:,1], moves
    the robot: close to the model's own prediction, not equal to it."""
    rb = mpcqp.synth.make_rollout_batch(3, total_steps=5, seed=11)
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config(N=10, delta=0.03, max_iter=4000))
    args = (rb["x"], rb["ref"], rb["plan_pos"], rb["plan_feet_id"], rb["plan_meta"], rb["tick"], rb["mu"])
    kin = eng.rollout_host(*args, 1)
    pl = rollout_plant_host(eng, *args, 3)
    assert np.array_equal(pl["forces"][:, 0], kin["forces"][:, 0]) and np.array_equal(pl["actual"][:, 0], kin["actual"][:, 0])
    assert np.all(pl["solved"] == 3) and np.all(pl["tick"] == 3)
    d = np.abs(pl["actual"][:, 1] - kin["x"][:, :12]).max()
    assert 0.0 < d < 1e-2, d
    with pytest.raises(ValueError, match="push_ticks"):
        rollout_plant_host(eng, *args, 1, push=np.zeros((3, 6)))


def test_sim_header_declares_sim_symbols_product_only(oracle_lib):
    """include/mpcqp_sim.h declares exactly SIM_SYMBOLS; the product library exports them, mpcqp.h and its version are unchanged and
    the CPU checker does not have them (its binding refuses the calls)."""
    hdr = open(os.path.join(REPO, "include", "mpcqp_sim.h")).read()
    syms = set(re.findall(r"^\s*int\s+(mpcqp_[a-z_]+)\s*\(", hdr, re.M))
    assert syms == set(mpcqp._capi.SIM_SYMBOLS) and '#include "mpcqp.h"' in hdr
    lib = mpcqp.product_library()
    assert lib.has_sim and all(hasattr(lib.lib, s) for s in syms) and lib.version() == 0x00010301
    base = open(os.path.join(REPO, "include", "mpcqp.h")).read()
    assert not any(s in base for s in syms)
    assert not oracle_lib.has_sim and not any(hasattr(oracle_lib.lib, s) for s in syms)
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    with pytest.raises(mpcqp.MpcQpError, match="product library only"):
        eng.plant_step_ptr(1, 1, 1, 1, 1, 0, 0, 10, 1)
