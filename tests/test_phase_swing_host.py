"""Host counterpart of the swing-foot trajectories of the roll-out on a gait clock (mpcqp.gaits.phase_swing_host, swing_target,
swing_profile; include/mpcqp_plan.h, mpcqp_phase_swing): the ends of a swing, the apex, the target against every landing of a closed
loop on the CPU checker, the derivatives against central differences, and how far the target drifts before the landing.  No GPU: the
device is held to this module in tests/test_gpu_phase_swing.py."""
import functools

import numpy as np

import mpcqp
from conftest import ORACLE_SO
from mpcqp import gaits, lite3_model, synth

DELTA = 0.03
STEP_HEIGHT = 0.06


def _row(P, off, st):
    return np.array([[P, *off, *st]], np.int32)


def _one_robot(T, gait, seed=1):
    """Synthetic logs of one robot: a slowly moving, slightly turned torso over feet near the nominal stance."""
    rng = np.random.default_rng(seed)
    actual = np.zeros((1, T, 12))
    actual[0, :, 0:3] = rng.normal(0.0, 0.05, (T, 3))
    actual[0, :, 3:6] = np.array([0.0, 0.0, synth.H_COM]) + np.arange(T)[:, None] * DELTA * np.array([0.2, 0.02, 0.0])
    actual[0, :, 6:9] = rng.normal(0.0, 0.1, (T, 3))
    actual[0, :, 9:12] = np.array([0.2, 0.02, 0.0]) + rng.normal(0.0, 0.02, (T, 3))
    desired = np.zeros((1, T, 12))
    desired[0, :, 8] = 0.3
    desired[0, :, 9:12] = [0.18, 0.0, 0.0]
    stand = np.concatenate([synth.NOMINAL_FEET[:, :2], np.zeros((4, 1))], axis=1)[None]
    feet_log = np.repeat((stand + rng.normal(0.0, 0.01, (1, 4, 3)) * [1.0, 1.0, 0.0])[:, None], T, axis=1)
    return {"actual": actual, "desired": desired, "feet_log": feet_log, "gait": gait, "tick0": np.zeros(1, np.int32), "stand": stand,
            "gain": np.array([0.05]), "step_height": np.array([STEP_HEIGHT])}


def _host(p):
    return gaits.phase_swing_host(p["actual"], p["desired"], p["feet_log"], p["gait"], p["tick0"], p["stand"], p["gain"], p["step_height"],
                                  DELTA)["swing"]


def test_start_and_end_of_a_swing():
    P, st = 12, 7
    p = _one_robot(P, _row(P, [0, 0, 0, 0], [st] * 4))
    sw = _host(p)
    # s = 0 at the lift-off tick: the lift-off foot itself, at rest
    assert np.array_equal(sw[0, st, :, 0], p["feet_log"][0, st]) and not sw[0, st, :, 1].any()
    assert np.abs(sw[0, st, :, 2]).max() > 0.0 and not np.array_equal(sw[0, st, :, 3], p["feet_log"][0, st])
    # stance rows: pos = target = the log row, vel = acc = 0
    for t in range(st):
        assert np.array_equal(sw[0, t, :, 0], p["feet_log"][0, t]) and np.array_equal(sw[0, t, :, 3], p["feet_log"][0, t])
        assert not sw[0, t, :, 1:3].any()
    # s = 1 is the touchdown tick, a stance row: fed by hand, rem = 0
    a, d = p["actual"][:, 0], p["desired"][:, 0]
    p1 = gaits.swing_target(a, d, p["gait"], p["stand"], p["gain"], np.zeros((1, 4)), DELTA)
    rule = gaits.touchdown_foothold(a[:, 3:6], gaits.measured_yaw(a[:, 0:3]), a[:, 9:12], d[:, 9:12], p["stand"], p["gain"], p["gait"], DELTA)
    assert np.array_equal(p1, rule)
    p0 = p["feet_log"][:, 0]
    pos, vel, acc = gaits.swing_profile(np.ones((1, 4)), p0, p1, np.full((1, 4), STEP_HEIGHT), np.full((1, 4), (P - st) * DELTA))
    assert np.abs(pos - p1).max() <= 2.0 * np.spacing(max(np.abs(p0).max(), np.abs(p1).max())) and not vel.any()   # p0 + (p1 - p0)
    assert np.abs(acc).max() > 0.0
    # every swing row's s lies in [0, 1): the z of a swing over level ground is the bump alone
    zb = sw[0, st:, 0, 0, 2]
    assert np.all(zb[1:] > 0.0) and zb[0] == 0.0 and zb.max() <= STEP_HEIGHT


def test_bump_peaks_at_step_height_at_half_swing():
    P, st = 12, 6                       # n = 6: tick 9 is s = 1 / 2 exactly
    p = _one_robot(P, _row(P, [0, 0, 0, 0], [st] * 4))
    sw = _host(p)
    z = sw[0, :, :, 0, 2]
    assert np.all(z[9] == STEP_HEIGHT) and np.all(z.max(axis=0) == STEP_HEIGHT)
    assert not sw[0, 9, :, 1, 2].any()                                           # the apex: no vertical velocity
    assert np.all(sw[0, 9, :, 2, 2] == -16.0 * STEP_HEIGHT / (st * DELTA) ** 2)      # z_b''(1/2) = 32 H (1 - 3 + 3/2)


def test_derivatives_are_the_central_differences_of_the_frozen_curve():
    """pos is a polynomial of degree <= 4 in s: |pos'''| <= 12 |dp| + 192 H and |pos''''| <= 384 H.  The central difference of step h
    has truncation error h^2 / 6 |pos'''| for the first and h^2 / 12 |pos''''| for the second derivative, and rounding error at most
    2 eps |pos| / (2 h) and 4 eps |pos| / h^2 (eps = 2^-52, each evaluation good to an eps of |pos| and a few more for its own
    arithmetic: a factor 8 covers those)."""
    rng = np.random.default_rng(4)
    n, h, H, tsw = 200, 1e-3, 0.08, 0.15
    s = rng.uniform(h, 1.0 - h, n)
    p0, p1 = rng.normal(0.0, 0.3, (n, 3)), rng.normal(0.0, 0.3, (n, 3))
    hh, tt = np.full(n, H), np.full(n, tsw)
    pos, vel, acc = gaits.swing_profile(s, p0, p1, hh, tt)
    lo, hi = gaits.swing_profile(s - h, p0, p1, hh, tt)[0], gaits.swing_profile(s + h, p0, p1, hh, tt)[0]
    dp, scale, eps = np.abs(p1 - p0).max(), max(np.abs(p0).max(), np.abs(p1).max()) + H, 2.0 ** -52
    band1 = h * h / 6.0 * (12.0 * dp + 192.0 * H) + 8.0 * eps * scale / h
    band2 = h * h / 12.0 * 384.0 * H + 8.0 * 4.0 * eps * scale / (h * h)
    e1 = np.abs((hi - lo) / (2.0 * h) - vel * tsw).max()
    e2 = np.abs((hi - 2.0 * pos + lo) / (h * h) - acc * tsw * tsw).max()
    print(f"central differences: d/ds {e1:.3e} (band {band1:.3e}), d2/ds2 {e2:.3e} (band {band2:.3e})")
    assert e1 <= band1 and e2 <= band2
    assert np.abs(vel).max() > 1.0 and np.abs(acc).max() > 10.0


# ------------------------------------------------------------------------------------------------ a closed loop on the CPU checker
B_LOOP, T_LOOP, PERIOD = 8, 25, 12


@functools.lru_cache(maxsize=None)
def _loop():
    pb = gaits.make_phase_batch(B_LOOP, ("trot", "bound"), PERIOD, seed=6)
    rows = synth.make_plant_rows(B_LOOP, seed=6, push_start=(3, 15))        # (this seed pushes half of them)
    lib = mpcqp.Library(ORACLE_SO)
    eng = mpcqp.Engine(lib, lib.default_config(N=10, delta=DELTA, max_iter=4000))
    o = gaits.rollout_phase_host(eng, pb["x"], pb["ref"], pb["feet"], pb["gait"], pb["stand"], pb["gain"], pb["tick"], pb["mu"], T_LOOP,
                                 rows["body"], rows["push"], rows["push_ticks"])
    sw = gaits.phase_swing_host(o["actual"], o["desired"], o["feet_log"], pb["gait"], pb["tick"], pb["stand"], pb["gain"],
                                np.full(B_LOOP, STEP_HEIGHT), DELTA)
    return pb, rows, o, sw


def test_target_at_rem_0_is_every_landing_of_the_closed_loop(oracle_lib):
    pb, rows, o, sw = _loop()
    assert rows["pushed"].sum() == B_LOOP // 2 and np.all(o["solved"] == T_LOOP)
    cl, fl = o["contact_log"], o["feet_log"]
    landings, worst = 0, 0.0
    for t in range(1, T_LOOP):
        landed = (cl[:, t] == 1) & (cl[:, t - 1] == 0)
        p1 = gaits.swing_target(o["actual"][:, t], o["desired"][:, t], pb["gait"], pb["stand"], pb["gain"], np.zeros((B_LOOP, 4)), DELTA)
        if landed.any():
            landings += int(landed.sum())
            worst = max(worst, np.abs(p1[landed] - fl[:, t][landed]).max())
    print(f"{landings} landings, target at rem = 0 against the landed foot: {worst:.3e}")
    assert landings >= 2 * B_LOOP and worst <= 1e-12
    # the log's stance rows come back bit for bit, its swing rows leave from the lift-off foot and stay in reach of the leg
    s = sw["swing"]
    up = cl == 0
    assert np.array_equal(s[:, :, :, 0][~up], fl[~up]) and np.array_equal(s[:, :, :, 3][~up], fl[~up]) and not s[:, :, :, 1:3][~up].any()
    assert np.array_equal(sw["feet_des"], s[:, :, :, 0]) and np.all(s[:, :, :, 0, 2][up] >= fl[:, :, :, 2][up])
    reach = lite3_model.joint_rates_host(o["actual"], o["forces"], sw["feet_des"], s[:, :, :, 1])[4]
    calm = ~rows["pushed"]
    assert up[calm].any() and np.all(reach[calm] == 1)


def test_target_drift_before_the_landing_is_reported(oracle_lib):
    """A finding, not a bound: how far the last swing tick's target lies from the foothold the leg then lands on."""
    pb, rows, o, sw = _loop()
    cl, fl, tg = o["contact_log"], o["feet_log"], sw["swing"][:, :, :, 3]
    drift = {True: 0.0, False: 0.0}
    count = {True: 0, False: 0}
    for t in range(1, T_LOOP):
        landed = (cl[:, t] == 1) & (cl[:, t - 1] == 0)
        for b, l in zip(*np.nonzero(landed)):
            k = bool(rows["pushed"][b])
            drift[k] = max(drift[k], float(np.linalg.norm(tg[b, t - 1, l] - fl[b, t, l])))
            count[k] += 1
    print(f"target drift over the last swing tick: unpushed {drift[False] * 1e3:.3f} mm ({count[False]} landings), "
          f"pushed {drift[True] * 1e3:.3f} mm ({count[True]} landings)")
    assert count[True] > 0 and count[False] > 0
