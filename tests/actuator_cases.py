"""Cases shared by tests/test_actuators_host.py and tests/test_gpu_actuators.py (include/mpcqp_actuators.h, mpcqp_set_actuators): the
stance draw with per-robot rows, the row classes of the closed loops, the classification of a clamped leg, and the growth factors that
widen the bands of the device comparisons (measured on the host, stored in tests/golden/actuator_growth.npz)."""
import os

import numpy as np

import drive_cases as dc
import legsim_cases
from mpcqp import actuators, gaits, lite3_model

DRAW_SEED = 3
INVALID_ROBOT = 13                 # the robot of the draw whose row is invalid (qd_free below qd_knee)
# (scale, knee, free) of the closed loops; knee and free are fractions of qd_max
LITE3, HALF, CURVE, WEAK_CURVE = (1.0, np.inf, np.inf), (0.5, np.inf, np.inf), (1.0, 0.05, 0.25), (0.5, 0.1, 0.4)
CLASSES = (LITE3, HALF, CURVE, WEAK_CURVE)
GROWTH_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actuator_growth.npz")
GROWTH_EPS = 1e-10                 # operands moved by this much, relative (legsim_cases.growth_factor's step)


def rows_of(classes, B):
    """[B,9]: robot b gets classes[b mod len(classes)]."""
    pick = [classes[b % len(classes)] for b in range(B)]
    return actuators.actuator_rows(B, None, *[np.array([p[k] for p in pick]) for k in range(3)])


def drive_draw(seed=DRAW_SEED, moved=0.0):
    """drive_cases.clamp_draw() with a torso that moves -- omega of about 1 rad/s, v of about 0.3 m/s, so that the stance joints turn at a
    few rad/s with their feet at rest -- and one actuator row per robot: scale 0.4 to 1.2, knee 0.01 to 0.08 and free 0.1 to 0.35 of
    qd_max (0.2 to 2 rad/s and 1.7 to 9 rad/s), a flat row on every fifth robot, an invalid one on INVALID_ROBOT.  `moved`: x[6:12]
    scaled by (1 + moved), the operand the rate is made of.  Returns clamp_draw's dict plus "rows"."""
    c = dc.clamp_draw()
    B = c["x"].shape[0]
    rng = np.random.default_rng(seed)
    c["x"][:, 6:9] = rng.normal(0.0, 0.8, (B, 3))
    c["x"][:, 9:12] = rng.normal(0.0, 0.3, (B, 3))
    c["x"][:, 6:12] *= 1.0 + moved
    scale, knee, free = rng.uniform(0.4, 1.2, B), rng.uniform(0.01, 0.08, (B, 3)), rng.uniform(0.1, 0.35, (B, 3))
    flat = np.arange(B) % 5 == 4
    knee[flat], free[flat] = np.inf, np.inf
    rows = actuators.actuator_rows(B, None, scale, knee, free)
    rows[INVALID_ROBOT, 6:9] = 0.5 * rows[INVALID_ROBOT, 3:6]
    c["rows"], c["row_scale"], c["flat"] = rows, scale, flat
    return c


def as_io(case, dtype):
    """drive_cases.as_io, the table kept in fp64 (it is fp64 whatever the I/O dtype)."""
    keep = ("rows", "row_scale", "flat")
    out = dc.as_io({k: v for k, v in case.items() if k not in keep}, dtype)
    out.update({k: case[k] for k in keep})
    return out


def drive(case, **kw):
    return lite3_model.stance_drive_host(case["x"], case["f"], case["feet"], case["contact"], case["ground"], actuators=case["rows"], **kw)


def classify(rows, cmd, app, rate):
    """Per leg of cmd / app / rate [...,4,3] under rows [B,9]: (falling, flat, moving) -- clamped with a joint held at the falling part
    of its curve (the applied torque is below tau_max in size), clamped at tau_max only, and not clamped with a joint that turns."""
    tm = np.asarray(rows)[:, 0:3].reshape((-1,) + (1,) * (np.ndim(cmd) - 2) + (3,))
    with np.errstate(invalid="ignore"):
        hit = app != cmd
        fall = hit & (np.abs(app) < tm)
        clamped = hit.any(axis=-1)
        return fall.any(axis=-1), clamped & ~fall.any(axis=-1), ~clamped & (np.asarray(rate) != 0.0).any(axis=-1)


def draw_growth(dtype=np.float64):
    """How much the outputs of the draw move per unit the stance rate moves when x[6:12] is moved by GROWTH_EPS relative: max |change
    of f, tau| / max |change of rate| over the legs whose flags stay."""
    a, b = drive(as_io(drive_draw(), dtype)), drive(as_io(drive_draw(moved=GROWTH_EPS), dtype))
    ok = (a["flag"] != 0xff) & (a["flag"] == b["flag"])
    drate = np.abs(a["rate"] - b["rate"])[ok].max()
    dout = max(np.abs(a["f"] - b["f"]).reshape(-1, 4, 3)[ok].max(), np.abs(a["tau"] - b["tau"])[ok].max())
    return float(dout / drate)


def track_growth(logs, swing, body, rows, eps=GROWTH_EPS, seed=9):
    """legsim_cases.growth_factor with an actuator table: swing_track_host over the logs from an initial state moved by eps."""
    a = [np.asarray(logs[k]) for k in ("actual", "forces", "feet_log", "contact_log")]
    on = lite3_model.joint_rates_host(a[0][:, :1], a[1][:, :1], np.asarray(swing)[:, :1, :, 0], np.asarray(swing)[:, :1, :, 1])
    B = a[0].shape[0]
    st = np.concatenate([on[0][:, 0], on[1][:, 0], np.ones((B, 4, 1))], axis=-1)
    st2 = st.copy()
    st2[:, :, :6] += eps * np.random.default_rng(seed).choice([-1.0, 1.0], (B, 4, 6))
    o1 = lite3_model.swing_track_host(*a, swing, body=body, state=st, delta=legsim_cases.DELTA, actuators=rows)
    o2 = lite3_model.swing_track_host(*a, swing, body=body, state=st2, delta=legsim_cases.DELTA, actuators=rows)
    ok = (o1["flag"] != 0xff) & (o2["flag"] != 0xff)
    return max(float(np.abs(o1[k] - o2[k])[ok].max()) for k in ("q", "qd", "tau", "foot", "err")) / eps


def recorded_growth():
    """{"draw": ..., "rollout": ...} as stored by tests/test_actuators_host.py's measurement."""
    with np.load(GROWTH_NPZ) as z:
        return {k: float(z[k]) for k in z.files}


def rollout_rows():
    """The table of the 16-robot roll-out batch: the four classes cycling through the robots."""
    return rows_of(CLASSES, legsim_cases.ROLL_B)
