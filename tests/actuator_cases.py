"""Cases shared by tests/test_actuators_host.py and tests/test_gpu_actuators.py (include/mpcqp_actuators.h, mpcqp_set_actuators): the
stance draw with per-robot rows, the row classes of the closed loops, the classification of a clamped leg, and the growth factors that
widen the bands of the device comparisons (measured on the host, stored in tests/golden/actuator_growth.npz); and, further down, the
cases of tests/test_actuator_rows_host.py and tests/test_gpu_actuator_rows.py: rows that differ per robot through every reader of the
table."""
import functools
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


# ------------------------------------------------------- the cases of tests/test_actuator_rows_host.py and tests/test_gpu_actuator_rows.py
def drawn_rows(B, seed=DRAW_SEED, invalid=None):
    """[B,9]: one row per robot in drive_draw's ranges: scale 0.4 to 1.2, knee 0.01 to 0.08 and free 0.1 to 0.35 of qd_max, every
    fifth row flat, row `invalid` (or None) with qd_free = qd_knee / 2.  No two valid rows are equal."""
    rng = np.random.default_rng(seed)
    scale, knee, free = rng.uniform(0.4, 1.2, B), rng.uniform(0.01, 0.08, (B, 3)), rng.uniform(0.1, 0.35, (B, 3))
    flat = np.arange(B) % 5 == 4
    knee[flat], free[flat] = np.inf, np.inf
    rows = actuators.actuator_rows(B, None, scale, knee, free)
    if invalid is not None:
        rows[invalid, 6:9] = 0.5 * rows[invalid, 3:6]
    return rows


EFFORT_ROBOTS_MOVED = 20           # a neighbour's row must change leg_effort's limit on at least this many of the 32 robots


def effort_case(io):
    """leg_effort with one row per robot: the 32 x 4 rows of tests/test_gpu_leg_dynamics.py (known accelerations, a leg out of reach, far
    feet) as the I/O dtype holds them, and drawn_rows(32) with robot INVALID_ROBOT invalid.  Returns (operands dict, rows)."""
    from test_gpu_leg_dynamics import B, _logs
    return _logs(io), drawn_rows(B, DRAW_SEED, INVALID_ROBOT)


EFFORT_IN = ("actual", "forces", "feet", "foot_vel", "foot_acc", "base_acc", "body")
EFFORT_VARIANTS = (("all operands", ()), ("base_acc = None", ("base_acc",)), ("only the required", EFFORT_IN[3:]))


def effort_host(s, rows, drop=()):
    return lite3_model.leg_effort_host(*[None if k in drop else s[k] for k in EFFORT_IN], actuators=rows)


def effort_margin(host, rows):
    """[B,T,4]: actuators.margin_host of leg_effort_host's torque against robot b's envelope at the row's rate; inf on a 0xff leg."""
    m = actuators.margin_host(rows, host["tau"], host["qd"])
    return np.where(host["limit"] == 0xff, np.inf, m)


def invalid_kinds(good):
    """The ten invalid kinds of tests/test_actuators_host.py's test_valid_rows_rejects_each_invalid_kind on the curved row `good`: a list of
    (name, column, value)."""
    return [("tau_max nan", 0, np.nan), ("tau_max inf", 1, np.inf), ("tau_max negative", 2, -1.0), ("knee negative", 3, -0.5),
            ("knee nan", 4, np.nan), ("free below knee", 6, good[3] * 0.5), ("free equal knee", 7, good[4]),
            ("free inf at a finite knee", 8, np.inf), ("free nan at a finite knee", 6, np.nan), ("knee -inf", 5, -np.inf)]


CONV_TILES, CONV_SEED = 19, 11
CONV_INVALID = (0, 255, 256, 257, 300, 511, 512, 513, 600, 626)   # the first and last row and both sides of each block boundary
CONV_EDGES = (40, 41, 42, 43, 44)


def conversion_case():
    """The conversion kernel over three blocks: drive_draw()'s operands repeated CONV_TILES times (627 rows, the last block partial) with
    rows drawn per row (CONV_SEED), one row of each invalid kind planted at CONV_INVALID and the valid edge rows at CONV_EDGES: tau_max[0] =
    0, qd_knee[0] = 0, tau_max[1] = -0.0, qd_free one spacing above qd_knee, flat with qd_free = NaN.  (A denormal tau_max is left out: its
    margin to the envelope is 0 by construction.)  Returns (drive_draw's dict with "rows" the planted table, the
    table with a flat Lite3 row in place of each invalid one, bool [627] the invalid rows)."""
    c = drive_draw()
    n = c["x"].shape[0] * CONV_TILES
    out = {k: np.tile(c[k], (CONV_TILES,) + (1,) * (c[k].ndim - 1)) for k in ("x", "f", "feet", "contact", "ground")}
    rows = drawn_rows(n, CONV_SEED)
    assert n == 627 and np.all(np.isfinite(rows[list(CONV_INVALID) + list(CONV_EDGES[:4]), 3:6]))     # curved rows where a curve is altered
    for k, r in enumerate(CONV_INVALID):
        _, col, val = invalid_kinds(rows[r])[k]
        rows[r, col] = val
    e = CONV_EDGES
    rows[e[0], 0] = 0.0
    rows[e[1], 3] = 0.0
    rows[e[2], 1] = -0.0
    rows[e[3], 6:9] = np.nextafter(rows[e[3], 3:6], np.inf)
    assert np.all(np.isinf(rows[e[4], 3:6]))                                    # (every fifth row is flat)
    rows[e[4], 6:9] = np.nan
    bad = np.zeros(n, bool)
    bad[list(CONV_INVALID)] = True
    mended = rows.copy()
    mended[bad] = actuators.actuator_rows(1)[0]
    out.update(rows=rows, row_scale=None, flat=np.arange(n) % 5 == 4, scale=c["scale"])
    return out, mended, bad


def combined_tables(B=legsim_cases.ROLL_B):
    """The three per-robot tables of the combined case next to models_rollout_cases.legs_case(), whose model class is b mod 4: the actuator
    class (b // 4) mod 4 of CLASSES and GROUND_MU under the even robots -- sixteen distinct combinations on 16 robots.  Returns (actuator
    rows [B,9], ground [B], actuator class [B])."""
    cls = (np.arange(B) // 4) % 4
    pick = [CLASSES[c] for c in cls]
    rows = actuators.actuator_rows(B, None, *[np.array([p[k] for p in pick]) for k in range(3)])
    return rows, np.where(np.arange(B) % 2 == 0, dc.GROUND_MU, 1e3), cls


INVALID_IN_LOOP = 6                # the robot of drive_cases.loop_batch() (walk) whose row is invalid in the clause-by-clause case
# (name, drive, land): drive None is rollout_legs; the ideal drive runs without a ground
LOOP_MODES = (("legs_rule", None, "rule"), ("ideal_rule", "ideal", "rule"), ("limited_actual", "limited", "actual"), ("legs_actual", None, "actual"))


def loop_rows(invalid=True):
    """rows_of(CLASSES, 8) for drive_cases.loop_batch(), robot INVALID_IN_LOOP's curved row with qd_free = qd_knee / 2 (or mended)."""
    rows = rows_of(CLASSES, dc.LOOP_B)
    if invalid:
        rows[INVALID_IN_LOOP, 6:9] = 0.5 * rows[INVALID_IN_LOOP, 3:6]
    return rows


LOOP_HOST_T = 8                    # the ticks of the host loop that a device test runs next to its own roll-out
LOOP_FLOATS = ("x", "ref", "feet", "stand", "gain", "mu")


def loop_pb(io="f64"):
    """drive_cases.loop_batch() as the I/O dtype holds it."""
    pb = dc.loop_batch()
    if io == "f32":
        pb = {k: (np.asarray(v, np.float32).astype(np.float64) if k in LOOP_FLOATS else v) for k, v in pb.items()}
    return pb


def checker_engine():
    """A handle of the CPU checker with the configuration of the closed loops (tests/test_actuators_host.py's)."""
    import mpcqp
    from conftest import ORACLE_SO
    lib = mpcqp.Library(ORACLE_SO)
    return mpcqp.Engine(lib, lib.default_config(N=10, delta=legsim_cases.DELTA, max_iter=4000))


@functools.lru_cache(maxsize=None)
def loop_host(mode, invalid=True, T=dc.LOOP_T, io="f64"):
    """Robot INVALID_IN_LOOP of loop_pb(io) alone (the robots of a batch do not meet) through the host loop of LOOP_MODES[mode] over T
    ticks, its row invalid or mended; the result is shared: do not alter it."""
    _, drive, land = LOOP_MODES[mode]
    sub = slice(INVALID_IN_LOOP, INVALID_IN_LOOP + 1)
    pb = {k: (v[sub] if isinstance(v, np.ndarray) else v) for k, v in loop_pb(io).items()}
    return dc.run_loop(checker_engine(), pb, T=T, actuators=loop_rows(invalid)[sub], drive=drive, land=land)


def first_nonfinite_tick(actual):
    """The first tick of actual [T,12] with a non-finite entry, or T."""
    bad = np.nonzero(~np.isfinite(actual).all(axis=-1))[0]
    return int(bad[0]) if bad.size else actual.shape[0]


@functools.lru_cache(maxsize=None)
def combined_host():
    """models.rollout_drive_models_host (limited, land = actual) on models_rollout_cases.legs_case() with combined_tables(); shared: do
    not alter it."""
    import models_rollout_cases as C
    from mpcqp import models as M
    pb, pr, rows, T = C.legs_case()
    act, ground, _ = combined_tables()
    return M.rollout_drive_models_host(C.oracle_lib(), C.LOOP_KW, rows, *[pb[k] for k in C.LEGS_ARGS], T, pb["step_height"], land="actual",
                                       drive="limited", ground=ground, actuators=act, **pr)


def swing_and_landing_rows(contact_log):
    """(swing, landing) bool [...,T,4] of a contact log: a swing row, and the stance row that follows a swing row of the same leg."""
    up = np.asarray(contact_log) == 0
    land = np.zeros_like(up)
    land[..., 1:, :] = ~up[..., 1:, :] & up[..., :-1, :]
    return up, land
