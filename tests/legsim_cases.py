"""Cases shared by tests/test_swing_track_host.py and tests/test_gpu_swing_track.py (include/mpcqp_joints.h, mpcqp_leg_accel /
mpcqp_swing_track): the random joint rows of tests/test_gpu_leg_dynamics.py, hand-made swing logs on a torso in uniform motion, the
roll-out case of the end-to-end test, the growth factor of the serial state and the margins of the flags to their thresholds."""
import os

import numpy as np

from mpcqp import gaits, lite3_model, synth

DELTA, STEP_HEIGHT = 0.03, 0.06
GROWTH_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swing_track_growth.npz")
ROLL_B, ROLL_T, ROLL_PERIOD, ROLL_SEED = 16, 25, 12, 6
FLAG_MARGIN = 1e-9


def box_rows(n=33, seed=41):
    """The 33 random rows (132 legs) of test_leg_dynamics_against_the_host, in its draw order: q on the IK box, qd, qdd, rot, base."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    q = np.stack([rng.uniform(-0.5, 0.5, (n, 4)), rng.uniform(-1.5, -0.2, (n, 4)), rng.uniform(0.5, 2.3, (n, 4))], axis=-1)
    ops = {"qd": rng.uniform(-3.0, 3.0, (n, 4, 3)), "qdd": rng.uniform(-40.0, 40.0, (n, 4, 3)),
           "rot": Rotation.from_rotvec(rng.normal(0.0, 0.15, (n, 3))).as_matrix(),
           "base": np.concatenate([rng.normal(0.0, 1.0, (n, 3)), rng.normal(0.0, 3.0, (n, 3)), rng.normal(0.0, 2.0, (n, 3))], axis=-1)}
    return q, ops


def parabola_logs(n_swing=5, B=1, offset=0.0, seed=3):
    """B robots whose torso moves uniformly (no rotation, base_acc = 0) and whose four feet each follow a parabola of constant world
    acceleration for n_swing swing rows, framed by one stance row before and one after: T = n_swing + 2.  Within a row the desired
    arc pos + s vel + s^2 / 2 acc IS the parabola, so a tracking error comes from the integration alone.  `offset` [m] moves the
    lift-off state off the trajectory: it is returned as a live `state` (made with the closed-form IK at the displaced foot) and the
    logs then start at the first swing row, T = n_swing + 1.  Returns the operands of swing_track_host (base_acc given) plus "state" and "T"."""
    rng = np.random.default_rng(seed)
    T = n_swing + 2
    tsw = n_swing * DELTA
    actual = np.zeros((B, T, 12))
    v = np.array([0.18, 0.02, 0.0]) + rng.normal(0.0, 0.02, (B, 3)) * [1.0, 1.0, 0.0]
    com0 = np.array([0.0, 0.0, synth.H_COM]) + rng.normal(0.0, 0.005, (B, 3))
    tt = np.arange(T)[None, :, None] * DELTA
    actual[:, :, 3:6] = com0[:, None] + tt * v[:, None]
    actual[:, :, 9:12] = v[:, None]
    stand = np.concatenate([synth.NOMINAL_FEET[:, :2], np.full((4, 1), synth.FOOT_Z)], axis=1)
    p0 = com0[:, None, :] * [1.0, 1.0, 0.0] + stand[None] + rng.normal(0.0, 0.005, (B, 4, 3)) * [1.0, 1.0, 0.0]
    p0 = p0 + DELTA * v[:, None] * [1.0, 1.0, 0.0]                               # the foot at lift-off (row 1)
    p1 = p0 + (tsw * v[:, None] * 2.0 + rng.normal(0.0, 0.01, (B, 4, 3))) * [1.0, 1.0, 0.0]
    # constant acceleration a with lift-off velocity u, p(tsw) = p1, apex STEP_HEIGHT at half time
    a = np.zeros((B, 4, 3)); u = np.zeros((B, 4, 3))
    a[..., 2] = -8.0 * STEP_HEIGHT / tsw ** 2
    u[..., 2] = 4.0 * STEP_HEIGHT / tsw
    a[..., :2] = 2.0 * (p1 - p0)[..., :2] / tsw ** 2 * 0.5                      # half of the way by acceleration, half by velocity
    u[..., :2] = (p1 - p0)[..., :2] / tsw * 0.5
    swing = np.zeros((B, T, 4, 4, 3)); contact = np.zeros((B, T, 4), np.uint8)
    contact[:, 0] = 1; contact[:, -1] = 1
    for t in range(T):
        s = min(max(t - 1, 0), n_swing) * DELTA
        pos = p0 + s * u + 0.5 * s * s * a
        up = 0 < t < T - 1
        swing[:, t, :, 0] = pos
        swing[:, t, :, 1] = (u + s * a) if up else 0.0
        swing[:, t, :, 2] = a if up else 0.0
        swing[:, t, :, 3] = pos
    forces = np.zeros((B, T, 12))
    forces[:, 0, 2::3] = 22.0; forces[:, -1, 2::3] = 22.0
    feet_log = swing[:, :, :, 0].copy()
    feet_log[:, 1:-1] = p0[:, None]                                              # a swing row logs its lift-off foot
    out = {"actual": actual, "forces": forces, "feet_log": feet_log, "contact_log": contact, "swing": swing,
           "base_acc": np.zeros((B, T, 6)), "T": T, "state": None}
    if offset:
        d = offset * np.array([0.6, 0.0, 0.8])
        q0 = lite3_model.joint_rates_host(actual[:, 1:2], forces[:, 1:2], swing[:, 1:2, :, 0] + d, swing[:, 1:2, :, 1])
        out["state"] = np.concatenate([q0[0][:, 0], q0[1][:, 0], np.ones((B, 4, 1))], axis=-1)
        for k in TRACK_IN + ("base_acc",):                                      # the state belongs to the first swing row: start there
            out[k] = out[k][:, 1:].copy()
        out["T"] = T - 1
    return out


TRACK_IN = ("actual", "forces", "feet_log", "contact_log", "swing")


def turning_logs(n_swing=5, B=2, seed=5):
    """parabola_logs on a torso that turns and accelerates: constant world acceleration a of the CoM and constant angular acceleration
    alpha about a fixed axis n (omega = (w0 + alpha t) n, so the orientation is exactly the rotation vector n (w0 t + alpha t^2 / 2)),
    base_acc = (alpha n, a) given.  The rows are exact samples of that motion and the feet still follow world parabolas, so with a
    perfect start whatever the tracker loses is its own step: the torso's extrapolation inside a tick (c(s), omega(s), the
    quaternion step), the torso terms of the recursion and the integrator."""
    s = parabola_logs(n_swing, B=B, seed=seed)
    rng = np.random.default_rng(seed + 1)
    T = s["T"]
    n = rng.normal(0.0, 1.0, (B, 3)); n /= np.linalg.norm(n, axis=1)[:, None]
    w0, al = rng.uniform(0.5, 1.0, B), rng.uniform(2.0, 4.0, B)                   # rad / s, rad / s^2
    a = rng.normal(0.0, 1.0, (B, 3)) * [1.0, 1.0, 0.3]                           # m / s^2
    t = (np.arange(T) * DELTA)[None, :, None]
    v0, c0 = s["actual"][:, :1, 9:12], s["actual"][:, :1, 3:6]
    s["actual"][:, :, 0:3] = n[:, None] * (w0[:, None, None] * t + 0.5 * al[:, None, None] * t * t)
    s["actual"][:, :, 6:9] = n[:, None] * (w0[:, None, None] + al[:, None, None] * t)
    s["actual"][:, :, 9:12] = v0 + t * a[:, None]
    s["actual"][:, :, 3:6] = c0 + t * v0 + 0.5 * t * t * a[:, None]
    s["base_acc"] = np.broadcast_to(np.concatenate([al[:, None] * n, a], axis=1)[:, None], (B, T, 6)).copy()
    return s


def track(s, **kw):
    """swing_track_host on a dict of operands as the generators above return it (base_acc and state from the dict unless given)."""
    kw.setdefault("base_acc", s.get("base_acc"))
    kw.setdefault("state", s.get("state"))
    return lite3_model.swing_track_host(*[s[k] for k in TRACK_IN], delta=DELTA, **kw)


def rollout_batch():
    """The end-to-end case: 16 robots over the eight named gaits at period 12, two of them pushed."""
    pb = gaits.make_phase_batch(ROLL_B, tuple(gaits.GAITS), ROLL_PERIOD, seed=ROLL_SEED)
    rows = synth.make_plant_rows(ROLL_B, seed=ROLL_SEED, push_start=(3, 15))
    keep = np.zeros(ROLL_B, bool)
    keep[np.nonzero(rows["pushed"])[0][:2]] = True                             # of the robots this seed pushes, the first two
    rows["push"] = rows["push"] * keep[:, None]
    rows["push_ticks"][:, 1] = np.where(keep, rows["push_ticks"][:, 1], rows["push_ticks"][:, 0])
    rows["pushed"] = keep
    return pb, rows


def growth_factor(logs, swing, body, eps=1e-10, seed=9):
    """The largest ratio of output change to input change of swing_track_host over these logs when the initial state (every leg live
    at its on-trajectory state of row 0) is perturbed by eps: max over q, qd, tau, foot, err of max |change| / eps."""
    a = [np.asarray(logs[k]) for k in ("actual", "forces", "feet_log", "contact_log")]
    on = lite3_model.joint_rates_host(a[0][:, :1], a[1][:, :1], np.asarray(swing)[:, :1, :, 0], np.asarray(swing)[:, :1, :, 1])
    B = a[0].shape[0]
    st = np.concatenate([on[0][:, 0], on[1][:, 0], np.ones((B, 4, 1))], axis=-1)
    rng = np.random.default_rng(seed)
    st2 = st.copy()
    st2[:, :, :6] += eps * rng.choice([-1.0, 1.0], (B, 4, 6))
    o1 = lite3_model.swing_track_host(*a, swing, body=body, state=st, delta=DELTA)
    o2 = lite3_model.swing_track_host(*a, swing, body=body, state=st2, delta=DELTA)
    ok = (o1["flag"] != 0xff) & (o2["flag"] != 0xff)
    worst = 0.0
    for k in ("q", "qd", "tau", "foot", "err"):
        d = np.abs(o1[k] - o2[k])
        worst = max(worst, float(d[ok].max()))
    return worst / eps


def flag_margins(host):
    """True where a (robot, tick, leg) of the host's result came within FLAG_MARGIN max(1, |threshold|) of a threshold that decides one
    of its flag bits (joint limits, rate limits, the torque clamp, in any control period): there device and host may differ in a bit."""
    return (host["margin"] <= FLAG_MARGIN) & (host["flag"] != 0xff)
