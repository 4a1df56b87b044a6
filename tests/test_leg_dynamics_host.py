"""Host counterparts of the leg dynamics (mpcqp.lite3_model.leg_inertia, leg_dynamics_host, leg_effort_host; include/mpcqp_joints.h,
mpcqp_leg_dynamics / mpcqp_leg_effort): the default row against the C struct, the recursion against the principle of virtual work,
the inertia / bias / power identities, recovered accelerations on rows that were made from known ones, the limit flags, and what the
numbers say about the robot.  No GPU: the device is held to this module in tests/test_gpu_leg_dynamics.py.

Bands.  The physics checks compare the recursion with central differences, so their bands are finite-difference bands, not rounding:
each test evaluates its error at the step h it uses and at 2 h, asserts that it falls like h^2 (ratio in [3, 5]), and holds the error at
h to 10 x the maximum measured when the test was written (the constants below; the measured values are in DESIGN.md).  A wrong
sign, a missing Coriolis term or a wrong parallel-axis shift gives an error of the order of the torque itself, which is printed next
to the band."""
import ctypes
import functools

import numpy as np
from scipy.spatial.transform import Rotation

import mpcqp
from conftest import ORACLE_SO
from dynamics_cases import JDOT_STEP, MIN_DET, known_effort_logs
from mpcqp import gaits, lite3_model, synth

# measured maxima x 10 (see the module docstring); the size of the compared quantity on the same rows next to each
VW_STEP, VW_BAND = 1e-3, 1.3e-4          # virtual work, N m: measured 1.303e-5 at h = 1e-3 (5.211e-5 at 2e-3); |tau| max 1.84, median 0.45
POT_STEP, POT_BAND = 1e-3, 1.2e-6        # dV/dq, N m: measured 1.181e-7 at h = 1e-3 (4.726e-7 at 2e-3); |bias| max 0.71
PWR_STEP, PWR_BAND = 1e-3, 8.0e-4        # power balance, W: measured 7.958e-5 at h = 1e-3 (3.183e-4 at 2e-3); |tau . qd| max 7.5
# recovered qdd (rad / s^2, of up to 40) and tau (N m, of up to 42): the error of the generator's central difference for Jdot qd at its
# step 1e-4, through J^-1 (min |det J| 3.3e-3 m^3): measured 7.086e-6 (2.834e-5 at twice the step) and 6.562e-8
QDD_BAND, TAU_BAND = 7.1e-5, 6.6e-7


def _box(rng, n):
    """n rows of four legs on the box of the IK tests, with rates and accelerations and a moving torso of the size of rates_cases."""
    q = np.stack([rng.uniform(-0.5, 0.5, (n, 4)), rng.uniform(-1.5, -0.2, (n, 4)), rng.uniform(0.5, 2.3, (n, 4))], axis=-1)
    qd, qdd = rng.uniform(-3.0, 3.0, (n, 4, 3)), rng.uniform(-40.0, 40.0, (n, 4, 3))
    rotvec = rng.normal(0.0, 0.15, (n, 3))
    base = np.concatenate([rng.normal(0.0, 1.0, (n, 3)), rng.normal(0.0, 3.0, (n, 3)), rng.normal(0.0, 2.0, (n, 3))], axis=-1)
    return q, qd, qdd, rotvec, base


# ------------------------------------------------------------------------------------------------------------ 1. the default row
def test_default_row_is_the_c_struct_and_the_description():
    lib = mpcqp.product_library()
    c = lib.default_leg_inertia()
    d = lite3_model.leg_inertia()
    assert c.size == ctypes.sizeof(mpcqp._capi.MpcQpLegInertia) and set(c.as_dict()) == set(d)
    for k, v in c.as_dict().items():
        assert np.array_equal(np.asarray(v), np.asarray(d[k])), k            # field for field
    assert np.array_equal(mpcqp._capi.MpcQpLegInertia.from_dict(d).as_dict()["inertia"], d["inertia"])
    assert np.allclose(d["mass"].sum(axis=1), 0.428 + 0.61 + 0.115 + 0.01, rtol=0, atol=1e-15)
    m, com, I = d["mass"], d["com"], d["inertia"]
    assert np.all(m == m[0])
    # HIP: left / right mirror in y, front / hind in x.  A mirror in y flips com_y, Ixy, Iyz; one in x flips com_x, Ixy, Ixz.  The
    # description's own rows agree to its digits (8.1579e-07 against 8.1551e-07): signs exactly, magnitudes to 1e-3 relative.
    my, mx = np.array([1, -1, 1]), np.array([-1, 1, 1])
    py, px = np.array([1, 1, 1, -1, 1, -1]), np.array([1, 1, 1, -1, -1, 1])
    for a, b, mc, mp in ((0, 1, my, py), (2, 3, my, py), (0, 2, mx, px), (1, 3, mx, px)):
        assert np.array_equal(com[a, 0] * mc, com[b, 0])
        assert np.array_equal(np.sign(I[a, 0] * mp), np.sign(I[b, 0])) and np.allclose(I[a, 0] * mp, I[b, 0], rtol=1e-3, atol=0)
    # THIGH: the description mirrors it left / right only (the hind thighs are the front ones); SHANK: one row for all four legs
    assert np.array_equal(com[0, 1] * my, com[1, 1]) and np.array_equal(I[0, 1] * py, I[1, 1])
    assert np.array_equal(com[2, 1], com[0, 1]) and np.array_equal(I[3, 1], I[1, 1])
    assert np.all(com[:, 2] == com[0, 2]) and np.all(I[:, 2] == I[0, 2])
    # the FOOT folded into the SHANK: masses add, the centre of mass moves towards the foot point, the inertia is the foot's 1e-2
    # plus the shank's own plus the two parallel-axis shifts about the new centre
    own = lite3_model.leg_inertia(fold_foot=False)
    assert own["mass"][0, 2] == 0.115 and np.array_equal(own["inertia"][0, 2], [6.68e-04, 6.86e-04, 3.155e-05, -1.24e-08, 6.91e-06, 5.65e-09])
    c_new = (0.115 * own["com"][0, 2] + 0.01 * np.array([0.0, 0.0, -0.21])) / 0.125
    assert np.allclose(com[0, 2], c_new, rtol=0, atol=1e-18) and own["com"][0, 2][2] > com[0, 2][2] > -0.21
    full = lambda S: np.array([[S[0], S[3], S[4]], [S[3], S[1], S[5]], [S[4], S[5], S[2]]])
    shift = lambda mk, dv: mk * (dv @ dv * np.eye(3) - np.outer(dv, dv))
    want = (full(own["inertia"][0, 2]) + shift(0.115, own["com"][0, 2] - c_new) + 1e-2 * np.eye(3)
            + shift(0.01, np.array([0.0, 0.0, -0.21]) - c_new))
    assert np.allclose(full(I[0, 2]), want, rtol=1e-14, atol=1e-20) and I[0, 2, 0] > 15 * own["inertia"][0, 2, 0]
    # the joints' limit rows
    assert d["q_min"].tolist() == [-0.42, -2.67, 0.6] and d["q_max"].tolist() == [0.42, 0.314, 2.72]
    assert d["qd_max"].tolist() == [26.0, 26.0, 17.0] and d["tau_max"].tolist() == [24.0, 24.0, 36.0] and d["gravity"] == -9.81


# --------------------------------------------------------------------------------- 2. the recursion against the principle of virtual work
# Shares no code with leg_dynamics_host: its own forward kinematics (scipy rotations, the geometry and inertia DATA of the package).
def _fk_links(leg, q, Rw, pw):
    """World centre-of-mass positions [3,3], world orientations [3,3,3] and world joint axes [3,3] of the three links."""
    inr = lite3_model.leg_inertia()
    ax, ay = lite3_model._AX_X, lite3_model._AX_Y
    R1 = Rotation.from_rotvec(ax * q[0]).as_matrix()
    R2 = R1 @ Rotation.from_rotvec(ay * q[1]).as_matrix()
    R3 = R2 @ Rotation.from_rotvec(ay * q[2]).as_matrix()
    p1 = lite3_model._HIPX[leg]
    p2 = p1 + R1 @ lite3_model._HIPY[leg]
    p3 = p2 + R2 @ lite3_model._KNEE
    Rk, pk = (R1, R2, R3), (p1, p2, p3)
    c = np.stack([pw + Rw @ (pk[k] + Rk[k] @ inr["com"][leg, k]) for k in range(3)])
    return c, np.stack([Rw @ Rk[k] for k in range(3)]), np.stack([Rw @ R1 @ ax, Rw @ R2 @ ay, Rw @ R3 @ ay])


def _virtual_work_torque(leg, q0, qd0, qdd0, rotvec, base, h):
    """tau_j = sum_{k >= j} [m_k (a_k - g) . d c_k / d q_j + d/dt (I_k omega_k) . axis_j] along q(t) = q0 + qd0 t + qdd0 t^2 / 2,
    R(t) = exp([omega t + alpha t^2 / 2]) R0 (angular velocity omega and acceleration alpha at t = 0), origin p(t) = a t^2 / 2; all
    time derivatives by central differences of step h, the partial derivatives of c_k by central differences of step 1e-6 in q."""
    inr = lite3_model.leg_inertia()
    om, al, a = base[0:3], base[3:6], base[6:9]
    R0 = Rotation.from_rotvec(rotvec).as_matrix()
    g = np.array([0.0, 0.0, inr["gravity"]])
    full = lambda S: np.array([[S[0], S[3], S[4]], [S[3], S[1], S[5]], [S[4], S[5], S[2]]])

    def at(t):
        Rw = Rotation.from_rotvec(om * t + 0.5 * al * t * t).as_matrix() @ R0
        return _fk_links(leg, q0 + qd0 * t + 0.5 * qdd0 * t * t, Rw, 0.5 * a * t * t)

    def momentum(t):   # I_k omega_k in the world, omega_k from the link's own orientation at t -+ h
        (_, Ro, _), (_, Rlo, _), (_, Rhi, _) = at(t), at(t - h), at(t + h)
        L = []
        for k in range(3):
            w = Rotation.from_matrix(Rhi[k] @ Rlo[k].T).as_rotvec() / (2.0 * h)
            L.append(Ro[k] @ full(inr["inertia"][leg, k]) @ Ro[k].T @ w)
        return np.stack(L)

    (c0, _, axes), (cl, _, _), (ch, _, _) = at(0.0), at(-h), at(h)
    acc = (ch - 2.0 * c0 + cl) / (h * h)
    dL = (momentum(h) - momentum(-h)) / (2.0 * h)
    e = 1e-6
    tau = np.zeros(3)
    for j in range(3):
        dq = np.zeros(3); dq[j] = e
        dc = (_fk_links(leg, q0 + dq, R0, np.zeros(3))[0] - _fk_links(leg, q0 - dq, R0, np.zeros(3))[0]) / (2.0 * e)
        for k in range(j, 3):
            tau[j] += inr["mass"][leg, k] * (acc[k] - g) @ dc[k] + dL[k] @ axes[j]
    return tau


def test_recursion_against_the_principle_of_virtual_work():
    rng = np.random.default_rng(31)
    n = 52                                                                    # 208 legs
    q, qd, qdd, rotvec, base = _box(rng, n)
    R = Rotation.from_rotvec(rotvec).as_matrix()
    tau = lite3_model.leg_dynamics_host(q, qd, qdd, R, base)[0]
    err = {}
    for h in (VW_STEP, 2.0 * VW_STEP):
        vw = np.array([[_virtual_work_torque(l, q[i, l], qd[i, l], qdd[i, l], rotvec[i], base[i], h) for l in range(4)] for i in range(n)])
        err[h] = float(np.abs(vw - tau).max())
    ratio = err[2.0 * VW_STEP] / err[VW_STEP]
    print(f"virtual work against the recursion, {4 * n} legs: err {err[VW_STEP]:.3e} N m at h = {VW_STEP:g}, {err[2.0 * VW_STEP]:.3e} at 2 h "
          f"(ratio {ratio:.2f}); band {VW_BAND:.1e}; |tau| max {np.abs(tau).max():.2f} median {np.median(np.abs(tau)):.2f} N m")
    assert 3.0 <= ratio <= 5.0 and err[VW_STEP] <= VW_BAND


# ------------------------------------------------------------------------------------------- 3. inertia, bias and the power balance
def _potential(q, inr):
    """V = -sum_k m_k g . c_k of the four legs on a torso at rest in the world's axes, [n,4]."""
    Rl, _, p = lite3_model._leg_chain(q)
    V = 0.0
    for k in range(3):
        V = V - inr["mass"][:, k] * inr["gravity"] * (p[k] + np.einsum("...ij,...j->...i", Rl[k], inr["com"][:, k]))[..., 2]
    return V


def test_inertia_bias_and_power_balance():
    rng = np.random.default_rng(32)
    n = 64
    inr = lite3_model.leg_inertia()
    q, qd, qdd, rotvec, base = _box(rng, n)
    R = Rotation.from_rotvec(rotvec).as_matrix()
    tau, M, bias = lite3_model.leg_dynamics_host(q, qd, qdd, R, base)
    scale = np.abs(M).max(axis=(-1, -2), keepdims=True)
    assert np.abs(M - M.swapaxes(-1, -2)).max() <= 1e-12 * scale.max() and np.all(np.abs(M - M.swapaxes(-1, -2)) <= 1e-12 * scale)
    assert np.linalg.eigvalsh(0.5 * (M + M.swapaxes(-1, -2))).min() > 0.0
    resid = np.abs(tau - (np.einsum("nlij,nlj->nli", M, qdd) + bias)).max()
    print(f"tau - (M qdd + bias): {resid:.3e} N m of {np.abs(tau).max():.2f}; min eig M {np.linalg.eigvalsh(M).min():.3e} kg m^2")
    assert resid <= 1e-12 * max(1.0, np.abs(tau).max())
    # at rest on a resting torso the bias is the gradient of the potential energy
    b0 = lite3_model.leg_dynamics_host(q)[2]
    err = {}
    for h in (POT_STEP, 2.0 * POT_STEP):
        grad = np.empty_like(q)
        for j in range(3):
            dq = np.zeros(3); dq[j] = h
            grad[..., j] = (_potential(q + dq, inr) - _potential(q - dq, inr)) / (2.0 * h)
        err[h] = float(np.abs(grad - b0).max())
    ratio = err[2.0 * POT_STEP] / err[POT_STEP]
    print(f"bias at rest against dV/dq: err {err[POT_STEP]:.3e} N m at h = {POT_STEP:g}, {err[2.0 * POT_STEP]:.3e} at 2 h (ratio {ratio:.2f}); "
          f"band {POT_BAND:.1e}; |bias| max {np.abs(b0).max():.2f} N m")
    assert 3.0 <= ratio <= 5.0 and err[POT_STEP] <= POT_BAND
    # on a fixed torso the joints' power is the rate of the leg's kinetic plus potential energy
    tau_fixed = lite3_model.leg_dynamics_host(q, qd, qdd)[0]
    power = (tau_fixed * qd).sum(axis=-1)

    def energy(t):
        qt, qdt = q + qd * t + 0.5 * qdd * t * t, qd + qdd * t
        Mt = lite3_model.leg_dynamics_host(qt)[1]
        return 0.5 * np.einsum("nli,nlij,nlj->nl", qdt, Mt, qdt) + _potential(qt, inr)

    err = {h: float(np.abs((energy(h) - energy(-h)) / (2.0 * h) - power).max()) for h in (PWR_STEP, 2.0 * PWR_STEP)}
    ratio = err[2.0 * PWR_STEP] / err[PWR_STEP]
    print(f"power balance: err {err[PWR_STEP]:.3e} W at h = {PWR_STEP:g}, {err[2.0 * PWR_STEP]:.3e} at 2 h (ratio {ratio:.2f}); band {PWR_BAND:.1e}; "
          f"|tau . qd| max {np.abs(power).max():.1f} W")
    assert 3.0 <= ratio <= 5.0 and err[PWR_STEP] <= PWR_BAND


# ------------------------------------------------------------------------------------------------ 4. rows with known accelerations
def _known_tau(s):
    B, T = s["q"].shape[:2]
    base = np.concatenate([s["actual"][..., 6:9], s["base_acc"]], axis=-1).reshape(B * T, 9)
    dyn = lite3_model.leg_dynamics_host(s["q"].reshape(B * T, 4, 3), s["qd"].reshape(B * T, 4, 3), s["qdd"].reshape(B * T, 4, 3),
                                        s["R"].reshape(B * T, 3, 3), base)[0].reshape(B, T, 4, 3)
    tau_f = lite3_model.joint_rates_host(s["actual"], s["forces"], s["feet"], s["foot_vel"])[2]
    return tau_f + dyn, dyn


def test_effort_on_rows_with_known_accelerations():
    s = known_effort_logs()
    assert s["min_det"] > MIN_DET
    out = lite3_model.leg_effort_host(s["actual"], s["forces"], s["feet"], s["foot_vel"], s["foot_acc"], s["base_acc"])
    tau, dyn = _known_tau(s)
    assert np.all(out["reach"] == 1) and np.all(out["limit"] != 0xff)
    e_q = {1.0: float(np.abs(out["qdd"] - s["qdd"]).max())}
    e_t = float(np.abs(out["tau"] - tau).max())
    s2 = known_effort_logs(h=2.0 * JDOT_STEP)
    o2 = lite3_model.leg_effort_host(s2["actual"], s2["forces"], s2["feet"], s2["foot_vel"], s2["foot_acc"], s2["base_acc"])
    e_q[2.0] = float(np.abs(o2["qdd"] - s2["qdd"]).max())
    ratio = e_q[2.0] / e_q[1.0]
    print(f"recovered qdd: err {e_q[1.0]:.3e} rad/s^2 at the generator's step {JDOT_STEP:g}, {e_q[2.0]:.3e} at twice (ratio {ratio:.2f}), band "
          f"{QDD_BAND:.1e}, |qdd| <= 40; tau: err {e_t:.3e} N m, band {TAU_BAND:.1e}, |tau| max {np.abs(tau).max():.1f}, |tau_dyn| max "
          f"{np.abs(dyn).max():.2f}; min |det J| {s['min_det']:.3e}")
    assert 3.0 <= ratio <= 5.0 and e_q[1.0] <= QDD_BAND and e_t <= TAU_BAND
    assert np.abs(out["tau_dyn"] - dyn).max() <= TAU_BAND and np.array_equal(out["tau"], out["tau_f"] + out["tau_dyn"])
    assert np.abs(out["power"] - (out["tau"] * out["qd"]).sum(axis=-1)).max() <= 1e-12 * np.abs(out["power"]).max()
    # base_acc = None is the unpushed plant's right-hand side at the row: passing that explicitly is the same call, bit for bit
    body = synth.make_plant_rows(s["q"].shape[0], seed=3)["body"]
    rhs = lite3_model.plant_base_acc_host(s["actual"], s["forces"], s["feet"], body)
    a = lite3_model.leg_effort_host(s["actual"], s["forces"], s["feet"], s["foot_vel"], s["foot_acc"], None, body)
    b = lite3_model.leg_effort_host(s["actual"], s["forces"], s["feet"], s["foot_vel"], s["foot_acc"], rhs)
    for k in ("qdd", "tau_dyn", "tau", "power", "limit"):
        assert np.array_equal(a[k], b[k]), k
    m = body[:, 0][:, None, None]
    assert np.allclose(rhs[..., 3:6] * m, s["forces"].reshape(*s["forces"].shape[:2], 4, 3).sum(axis=2) + m * [0.0, 0.0, -9.81], rtol=1e-12, atol=1e-9)
    assert not np.array_equal(a["tau_dyn"], out["tau_dyn"])                    # (and it is not the random base_acc of the rows)


# ------------------------------------------------------------------------------------------------------------- 5. the limit flags
def _crafted_rows():
    """One robot, six ticks on a level torso at rest: all clear; a HipX angle beyond its limit; a knee rate beyond its limit; a force
    whose torque is beyond the limit; a foot out of reach; and again all clear."""
    T = 6
    q = np.tile(np.array([0.0, -1.0, 1.6]), (1, T, 4, 1))
    qd = np.zeros((1, T, 4, 3))
    forces = np.tile(np.array([0.0, 0.0, 20.0]), (1, T, 4)).reshape(1, T, 12)
    q[0, 1, 2, 0] = 0.45                                                        # HipX limit 0.42
    qd[0, 2, 1, 2] = 20.0                                                       # knee rate limit 17
    forces[0, 3, 9:12] = [0.0, 0.0, 400.0]                                      # HR
    actual = np.zeros((1, T, 12)); actual[..., 5] = 0.3
    feet = np.empty((1, T, 4, 3)); vel = np.empty((1, T, 4, 3))
    for t in range(T):
        for l in range(4):
            p, J = lite3_model.leg_fk_jac(l, q[0, t, l])
            feet[0, t, l] = actual[0, t, 3:6] + p
            vel[0, t, l] = J @ qd[0, t, l]
    feet[0, 4, 0, 2] -= 0.5                                                     # FL out of reach
    return actual, forces, feet, vel


def test_limit_flags_on_crafted_rows():
    actual, forces, feet, vel = _crafted_rows()
    out = lite3_model.leg_effort_host(actual, forces, feet, vel)
    want = np.zeros((1, 6, 4), np.uint8)
    want[0, 1, 2] = 1
    want[0, 2, 1] = 2
    want[0, 3, 3] = 4
    want[0, 4, 0] = 8 | 1        # out of reach: the clamped leg is straight, and a knee angle of 0 is below the knee's 0.6 rad
    assert np.array_equal(out["limit"], want), out["limit"]
    assert out["reach"][0, 4, 0] == 0 and not out["qdd"][0, 4, 0].any() and np.abs(out["tau_dyn"][0, 4, 0]).max() > 0.0   # holding torque
    assert np.abs(out["tau"][0, 3, 3]).max() > 36.0 and np.abs(out["tau"][0, 0]).max() < 24.0
    bad = feet.copy(); bad[0, 5, 2, 1] = np.nan
    o2 = lite3_model.leg_effort_host(actual, forces, bad, vel, body=None, base_acc=np.zeros((1, 6, 6)))
    o1 = lite3_model.leg_effort_host(actual, forces, feet, vel, body=None, base_acc=np.zeros((1, 6, 6)))
    hit = np.zeros((1, 6, 4), bool); hit[0, 5, 2] = True
    assert o2["limit"][0, 5, 2] == 0xff and np.isnan(o2["tau"][hit]).all() and np.isnan(o2["power"][hit]).all()
    for k in ("qdd", "tau_dyn", "tau", "power", "limit"):
        assert np.array_equal(o2[k][~hit], o1[k][~hit]), k


# ------------------------------------------------------------------------------------------------- 6. what it says about the robot
B_LOOP, T_LOOP, PERIOD, DELTA, STEP_HEIGHT = 8, 25, 12, 0.03, 0.06


@functools.lru_cache(maxsize=None)
def _loop():
    """The closed loop of tests/test_phase_swing_host.py on the CPU checker."""
    pb = gaits.make_phase_batch(B_LOOP, ("trot", "bound"), PERIOD, seed=6)
    rows = synth.make_plant_rows(B_LOOP, seed=6, push_start=(3, 15))
    lib = mpcqp.Library(ORACLE_SO)
    eng = mpcqp.Engine(lib, lib.default_config(N=10, delta=DELTA, max_iter=4000))
    o = gaits.rollout_phase_host(eng, pb["x"], pb["ref"], pb["feet"], pb["gait"], pb["stand"], pb["gain"], pb["tick"], pb["mu"], T_LOOP,
                                 rows["body"], rows["push"], rows["push_ticks"])
    sw = gaits.phase_swing_host(o["actual"], o["desired"], o["feet_log"], pb["gait"], pb["tick"], pb["stand"], pb["gain"],
                                np.full(B_LOOP, STEP_HEIGHT), DELTA)
    return rows, o, sw


def test_what_it_says_about_the_robot_is_reported(oracle_lib):
    """A finding, not a bound: the swing legs' dynamic torques, the stance legs' full torques and the share of robot-ticks with a
    limit flag, over the unpushed robots of the closed loop (base_acc = None is the unpushed plant's right-hand side)."""
    rows, o, sw = _loop()
    s = sw["swing"]
    out = lite3_model.leg_effort_host(o["actual"], o["forces"], sw["feet_des"], s[:, :, :, 1], s[:, :, :, 2], None, rows["body"])
    calm = ~rows["pushed"]
    up = (o["contact_log"] == 0) & calm[:, None, None]
    down = (o["contact_log"] != 0) & calm[:, None, None]
    assert up.any() and down.any() and np.all(out["limit"][calm] != 0xff)
    peak_dyn = np.abs(out["tau_dyn"][up]).max(axis=0)
    peak_st = np.abs(out["tau"][down]).max(axis=0)
    any_bit = (out["limit"][calm] != 0).any(axis=-1)
    print(f"{int(calm.sum())} unpushed robots x {T_LOOP} ticks (trot and bound, period {PERIOD}): peak |tau_dyn| over swing legs HipX / HipY / Knee "
          f"{peak_dyn[0]:.2f} / {peak_dyn[1]:.2f} / {peak_dyn[2]:.2f} N m (peak |qdd| {np.abs(out['qdd'][up]).max():.0f} rad/s^2, peak |qd| "
          f"{np.abs(out['qd'][up]).max():.1f} rad/s); peak |tau| over stance legs {peak_st[0]:.2f} / {peak_st[1]:.2f} / {peak_st[2]:.2f} N m; "
          f"robot-ticks with a limit bit: {any_bit.sum()} of {any_bit.size} ({100.0 * any_bit.mean():.1f} %), bits seen "
          f"{sorted(set(out['limit'][calm].ravel().tolist()) - {0})}")
    assert np.all(np.abs(out["tau_dyn"][up]).max(axis=-1) > 0.0)             # moving a leg costs something
    assert np.array_equal(out["tau"][up], out["tau_dyn"][up] + out["tau_f"][up]) and not out["tau_f"][up].any()
