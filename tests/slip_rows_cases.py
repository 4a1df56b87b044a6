"""Cases shared by tests/test_slip_rows_host.py and tests/test_gpu_slip_rows.py (include/mpcqp_slip.h, mpcqp_stance_slip /
mpcqp_rollout_slip): the slip rule and its roll-out with per-robot model rows, actuator rows, ground rows, foot masses and a start
slip state that is not zero.

The combined case.  models_rollout_cases.legs_case() -- 16 robots, 25 ticks, model class b mod 4, matched bodies, two robots pushed --
with actuator_cases.combined_tables()'s actuator rows (class (b // 4) mod 4), LOW_MU under the even robots and 1e3 under the odd ones,
sixteen distinct foot masses in [slip_cases.MASS_LO, MASS_HI] and a start slip state of N(0, START_SPEED) on half the feet, stance and
swing legs alike; land = actual, drive = limited.  LOW_MU and START_SPEED were chosen on the CPU checker so that the conditions of
tests/test_slip_rows_host.py hold: at ground 0.3 robots of this case fall through the floor, at 0.6 with N(0, 0.3 m/s) one falls, and
at 0.6 no clamped stance leg moves, so nothing there depends on s0 in the envelope's rate; at 0.56 and below robot 10 (the full-torque
curve on the heaviest model class) drops below 0.2 m.  At 0.58 it slides hard and stays up: every s0-sensitive leg-row is its.

The draw.  actuator_cases.drive_draw() -- 33 robots, a moving torso, one actuator row per robot, an invalid row on robot 13 -- with
slip_cases.slip_draw()'s foot velocities and foot masses (the same seed, the same third of the stance feet: both draws stand on
drive_cases.clamp_draw()'s contacts).

The growth factor of the draw (measured on the host, stored in tests/golden/slip_rows_growth.npz) widens the bands of the device
comparisons as actuator_cases.recorded_growth() does for the drive's."""
import functools
import os

import numpy as np

import actuator_cases as ac
import drive_cases as dc
import models_rollout_cases as C
import slip_cases as sc
from legsim_cases import DELTA
from mpcqp import actuators, lite3_model
from mpcqp import models as M

LOW_MU = 0.58                      # the slippery ground under the even robots
START_SEED, START_SPEED = 23, 0.1  # the start slip state: N(0, START_SPEED) [m/s] per component on half the feet
MASS_SEED = 29
SECOND_SUBSTEPS = 4                # the other substep count of the plant and the rule
S0_TORQUE = 1e-3                   # a leg counts as s0-sensitive when its applied torque moves by more than this [N m]
S0_LEGS = 10                       # ... and at least this many moving stance legs must be
GROWTH_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slip_rows_growth.npz")
FIVE = ("rows", "act", "ground", "foot_mass", "slip")


# ------------------------------------------------------------------------------------------------------------------ the combined case
def combined_case():
    """{"pb", "pr", "rows" [16,6], "T", "act" [16,9], "acls" [16], "ground" [16], "foot_mass" [16], "slip" [16,4,2]}."""
    pb, pr, rows, T = C.legs_case()
    B = C.LEGS_B
    act, _, acls = ac.combined_tables()
    ground = np.where(np.arange(B) % 2 == 0, LOW_MU, 1e3)
    foot_mass = np.random.default_rng(MASS_SEED).permutation(np.linspace(sc.MASS_LO, sc.MASS_HI, B))
    rng = np.random.default_rng(START_SEED)
    on = rng.uniform(size=(B, 4)) < 0.5
    slip = np.where(on[..., None], rng.normal(0.0, START_SPEED, (B, 4, 2)), 0.0)
    return {"pb": pb, "pr": pr, "rows": rows, "T": T, "act": act, "acls": acls, "ground": ground, "foot_mass": foot_mass, "slip": slip}


def run_host(K, **kw):
    """models.rollout_slip_models_host on a case as combined_case returns it (land = actual, drive = limited unless given)."""
    pb, pr = K["pb"], K["pr"]
    kw.setdefault("land", "actual")
    kw.setdefault("drive", "limited")
    return M.rollout_slip_models_host(C.oracle_lib(), C.LOOP_KW, K["rows"], *[pb[k] for k in C.LEGS_ARGS], K["T"], pb["step_height"],
                                      K["ground"], K["foot_mass"], K["slip"], actuators=K["act"], **pr, **kw)


@functools.lru_cache(maxsize=None)
def combined_host(substeps=10):
    """The combined case on the CPU checker, once per substep count; the result is shared: do not alter it."""
    return run_host(combined_case(), substeps=substeps)


def replay_operands(logs, K):
    """The operands of stance_slip / stance_slip_host for the B T logged rows of a slip roll-out, robot-major, all four per-robot
    tables tiled: (x [n,12], f = cmd [n,12], feet [n,4,3], contact [n,4], ground [n], foot_mass [n], slip_in [n,4,2], actuators [n,9])."""
    B, T = logs["contact_log"].shape[:2]
    n = B * T
    return (np.asarray(logs["actual"]).reshape(n, 12), np.asarray(logs["cmd"]).reshape(n, 12), np.asarray(logs["feet_log"]).reshape(n, 4, 3),
            np.asarray(logs["contact_log"]).reshape(n, 4), np.repeat(K["ground"], T), np.repeat(K["foot_mass"], T),
            np.asarray(logs["slip_log"]).reshape(n, 4, 2), actuators.tile(K["act"], T))


def replay_host(logs, K, substeps=10, drive="limited"):
    """lite3_model.stance_slip_host on the logged rows of a slip roll-out of the case K (host or device logs, as float64)."""
    x, f, feet, contact, ground, me, s0, act = replay_operands(logs, K)
    f64 = lambda a: np.asarray(a, np.float64)
    return lite3_model.stance_slip_host(f64(x), f64(f), f64(feet), contact, f64(ground), f64(me), s0, drive, actuators=act, delta=DELTA,
                                        substeps=substeps)


def counts(logs, K):
    """The figures of the conditions: per kind the number of leg-rows, and the low-friction robots with a sliding stance row."""
    fl, st = np.asarray(logs["flag"]), np.asarray(logs["contact_log"]) != 0
    live = fl != 0xff
    bit = lambda b: ((fl & b) != 0) & live
    low = K["ground"] < 1.0
    return {"clamped stance": int((bit(2) & st).sum()), "clamped swing": int((bit(2) & ~st).sum()), "ground": int((bit(32) & st).sum()),
            "sliding": int((bit(128) & st).sum()), "sliding low-friction robots": int((bit(128) & st).any(axis=(1, 2))[low].sum()),
            "low-friction robots": int(low.sum()), "stance": int(st.sum()), "dead": int((~live).sum())}


def start_on_swing(K, contact_log):
    """bool [B,4]: legs with a start slip entry that are in swing on the first tick."""
    return K["slip"].any(axis=-1) & (np.asarray(contact_log)[:, 0] == 0)


# ------------------------------------------------------------------------------------------------------------------------- the draw
def rows_draw(moved=0.0):
    """actuator_cases.drive_draw(moved=moved) plus slip_cases.slip_draw()'s "slip" [33,4,2] and "foot_mass" [33]."""
    c, s = ac.drive_draw(moved=moved), sc.slip_draw()
    assert np.array_equal(c["contact"], s["contact"]) and np.array_equal(c["feet"], s["feet"])
    c["slip"], c["foot_mass"] = s["slip"], s["foot_mass"]
    return c


def as_io(case, dtype):
    """actuator_cases.as_io; the slip state stays fp64 whatever the I/O dtype."""
    out = ac.as_io({k: v for k, v in case.items() if k != "slip"}, dtype)
    out["slip"] = case["slip"]
    return out


def slip(case, **kw):
    """stance_slip_host on the draw with its table."""
    kw.setdefault("actuators", case["rows"])
    return sc.slip(case, **kw)


def s0_sensitive(tau_cmd, rate_moving, rate_rest, rows, moving):
    """bool [n,4]: moving stance legs whose applied torque -- the envelope's clamp of tau_cmd -- differs by more than S0_TORQUE between
    the envelope read at the moving foot's joint rate and at the foot-at-rest rate (stance_drive_host's "rate")."""
    with np.errstate(invalid="ignore"):
        d = np.abs(actuators.clamp_host(rows, tau_cmd, rate_moving) - actuators.clamp_host(rows, tau_cmd, rate_rest)).max(axis=-1)
        return moving & (d > S0_TORQUE)


def tau_moves_without_s0(with_s0, without, moving):
    """bool [n,4]: live moving stance legs, off the thresholds in both results, whose applied torque is another one when the same call
    is made with slip = 0 (host results of `slip`)."""
    ok = moving & (with_s0["flag"] != 0xff) & ~dc.near_threshold(with_s0) & ~dc.near_threshold(without)
    with np.errstate(invalid="ignore"):
        return ok & (with_s0["tau"] != without["tau"]).any(axis=-1)


def rest_rate(x, f, feet, contact, ground, rows):
    """stance_drive_host's "rate": the stance joint rates with every foot at rest in the world."""
    return lite3_model.stance_drive_host(x, f, feet, contact, ground, actuators=rows)["rate"]


def rule_with_rate(x, f, feet, contact, ground, foot_mass, slip_in, rows, rate, **kw):
    """The slip rule with the envelope read at `rate` [n,4,3] whatever s0 is, through stance_slip_host's own arguments: every leg
    becomes a robot of its own (the other three in swing) under a FLAT actuator row whose tau_max is the side of the envelope at
    `rate` that the leg's tau_cmd can reach (hi for tau_cmd >= 0, -lo below): a flat row clamps without reading a rate, and the clamp
    of a torque only ever meets the bound on its own side.  With `rate` the moving foot's own this is stance_slip_host, bit for bit
    (tests/test_slip_rows_host.py holds that); with the foot-at-rest rate it is the rule with s0 left out of the rate.
    Returns {"f" [n,4,3], "tau", "flag", "slip", "disp"} on the stance legs (a swing leg: f as given, zeros)."""
    n = np.asarray(x).shape[0]
    fr = np.asarray(f, np.float64).reshape(n, 4, 3)
    st = np.asarray(contact).reshape(n, 4) != 0
    tc = lite3_model.stance_slip_host(x, f, feet, contact, ground, foot_mass, slip_in, actuators=rows, **kw)["tau_cmd"]
    lo, hi = actuators.limits_host(rows, rate)
    with np.errstate(invalid="ignore"):
        side = np.where(np.nan_to_num(tc) >= 0.0, hi, -lo)                      # [n,4,3]; NaN on an invalid row
    rep = lambda a: np.repeat(np.asarray(a), 4, axis=0)
    one = np.zeros((n, 4, 4), np.uint8)
    one[:, np.arange(4), np.arange(4)] = st                                     # pseudo-robot (b, l): leg l alone, if it is in stance
    flat = np.concatenate([side.reshape(4 * n, 3), np.full((4 * n, 6), np.inf)], axis=1)
    o = lite3_model.stance_slip_host(rep(x), rep(fr.reshape(n, 12)), rep(feet), one.reshape(4 * n, 4), rep(ground), rep(foot_mass),
                                     rep(slip_in), actuators=flat, **kw)
    pick = lambda a: a.reshape((n, 4, 4) + a.shape[2:])[:, np.arange(4), np.arange(4)]
    return {"f": pick(o["f"].reshape(4 * n, 4, 3)), "tau": pick(o["tau"]), "flag": pick(o["flag"]), "slip": pick(o["slip"]),
            "disp": pick(o["disp"])}


def draw_growth(dtype=np.float64):
    """actuator_cases.draw_growth's measurement on rows_draw(): max |change of f, tau, s, d| / max |change of rate| over the legs whose
    flags stay, when x[6:12] is moved by actuator_cases.GROWTH_EPS relative."""
    a, b = slip(as_io(rows_draw(), dtype)), slip(as_io(rows_draw(moved=ac.GROWTH_EPS), dtype))
    ok = (a["flag"] != 0xff) & (a["flag"] == b["flag"])
    drate = np.abs(a["rate"] - b["rate"])[ok].max()
    dout = max(np.abs(a["f"] - b["f"]).reshape(-1, 4, 3)[ok].max(), *[np.abs(a[k] - b[k])[ok].max() for k in ("tau", "slip", "disp")])
    return float(dout / drate)


def recorded_growth():
    """{"draw": ...} as stored by tests/test_slip_rows_host.py's measurement."""
    with np.load(GROWTH_NPZ) as z:
        return {k: float(z[k]) for k in z.files}


def band_scale():
    """What the bands of tests/test_gpu_slip.py's comparison are multiplied by when a table is set: max(1, the recorded growth)."""
    return max(1.0, recorded_growth()["draw"])


def compare_with_host(tag, io, dev, host, f_in, foot_mass, stance, scale, error):
    """test_gpu_slip._compare_with_host with every band times `scale`: flags equal outside the margin; f_out bit-equal to f where the
    rule left the leg alone; elsewhere f_out and tau within band x scale; s and d within theirs x scale.  dev = {"f" [n,4,3], "tau",
    "flag" [n,4], "slip" [n,4,2], "disp"} as float64 numpy, `error` = test_gpu_stance_drive._error (or any (dev, host, io) -> (err,
    band)).  Legs the host poisoned (0xff) must be 0xff / NaN on the device.  Returns the worst error / band ratios."""
    npdt = np.float64 if io == "f64" else np.float32
    near = dc.near_threshold(host)
    print(f"{tag} {io}: {int(near.sum())} of {int(stance.sum())} stance legs within FLAG_MARGIN of a threshold")
    assert near.sum() <= dc.MARGIN_SHARE * stance.sum()
    keep = ~near
    assert np.array_equal(dev["flag"][keep], host["flag"][keep])
    hf = host["f"].reshape(-1, 4, 3)
    live = host["flag"] != 0xff
    free = keep & live & ((host["flag"] & (2 | 32 | 128)) == 0)
    assert np.array_equal(dev["f"][free], f_in[free], equal_nan=True)
    rest = keep & ~free
    worst = {}
    for k, d, h in (("f_out", dev["f"], hf), ("tau", dev["tau"], host["tau"])):
        err, band = error(d[rest], h[rest], io)
        print(f"{tag} {io} {k}: err {err:.3e} band {band:.1e} x {scale:.2f} on {int(rest.sum())} legs (max |{k}| {np.nanmax(np.abs(h[rest])):.1f})")
        assert err <= band * scale, (k, err)
        worst[k] = err / (band * scale)
    err, band = error(dev["tau"][free], host["tau"][free], io)
    assert err <= band * scale
    me = np.where(np.isfinite(foot_mass) & (np.asarray(foot_mass) > 0.0), foot_mass, 1.0)
    bs, bd = sc.state_bands(npdt, hf, f_in, me)
    for k, d, h, b in (("s", dev["slip"], host["slip"], bs), ("d", dev["disp"], host["disp"].astype(npdt).astype(np.float64), bd)):
        nan = np.isnan(h)
        assert np.array_equal(nan, np.isnan(d)), k
        ratio = np.where(nan, 0.0, np.abs(d - h) / (b * scale)[..., None])[keep]
        worst[k] = float(ratio.max())
        print(f"{tag} {io} {k}: worst |dev - host| / (band x {scale:.2f}) {worst[k]:.3e} (largest |{k}| {np.nanmax(np.abs(h)):.3f})")
        assert worst[k] <= 1.0, (k, worst[k])
    return worst
