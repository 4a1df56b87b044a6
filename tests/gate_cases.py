"""Cases shared by tests/test_gate_host.py and tests/test_gpu_gate.py (include/mpcqp_gate.h, mpcqp_estimate_track_gated and
mpcqp_rollout_observe_gated): the thresholds, the eight-gait batch of tools/estimate_report.py and tools/observe_report.py (one robot
per named gait, period 12, 36 ticks, seed 6) with its sensor rows, and the conditions on what the gate does.

The conditions are the issue's, which sit well inside the figures of the host study the thresholds come from: they are not
measurements of the code under test."""
import functools

import numpy as np

from conftest import ORACLE_SO                                                  # noqa: F401  (first: it puts the repository on the path)
import mpcqp
from mpcqp import estimator, gaits, lite3_model, score

GATE = {"d_lo": 1.0, "d_hi": 4.0}                                              # the defaults, spelled out
OPEN = {"d_lo": 1e300, "d_hi": 2e300}                                          # thresholds no d reaches
GAIT_T, GAIT_PERIOD, GAIT_SEED, DELTA, STEP_HEIGHT = 36, 12, 6, 0.03, 0.06
NAMES = tuple(gaits.GAITS)
GAIT_B = len(NAMES)
ICE, FIRM = 0.3, 1e3
HALVED = ("flying_trot", "bound", "pronk", "gallop", "walk")                   # gaits whose v_xy error must fall by a factor 2 on the ice
NOISE_SEED = 24


def gait_batch():
    return gaits.make_phase_batch(GAIT_B, NAMES, GAIT_PERIOD, seed=GAIT_SEED)


def checker():
    lib = mpcqp.Library(ORACLE_SO)
    return mpcqp.Engine(lib, lib.default_config(N=10, delta=DELTA, max_iter=4000))


def _head(pb):
    return [pb[k] for k in ("x", "ref", "feet")] + [np.zeros((GAIT_B, 4, 7))] + [pb[k] for k in ("gait", "stand", "gain", "tick", "mu")]


@functools.lru_cache(maxsize=None)
def slip_run(ground):
    """tools/estimate_report.py's roll-out: gaits.rollout_slip_host of the eight gaits on `ground`, land = actual."""
    pb = gait_batch()
    return gaits.rollout_slip_host(checker(), *_head(pb), GAIT_T, np.full(GAIT_B, STEP_HEIGHT), np.full(GAIT_B, ground),
                                   lite3_model.foot_mass(), land="actual")


@functools.lru_cache(maxsize=None)
def sensors(ground, noise):
    """tools/estimate_report.py's sensor rows of `slip_run(ground)`: (imu, q, qd), with its sensor noise where `noise`."""
    o = slip_run(ground)
    acc = lite3_model.plant_base_acc_host(o["actual"], o["forces"], o["feet_log"])
    imu = estimator.imu_log_host(o["actual"], o["forces"], o["feet_log"], base_acc=acc)
    stance = np.asarray(o["contact_log"]) != 0
    vel = np.zeros((GAIT_B, GAIT_T, 4, 3))
    vel[..., :2] = np.where(stance[..., None], o["slip_log"], 0.0)
    q1, qd1, _, _, _ = lite3_model.joint_rates_host(o["actual"], o["forces"], o["feet_log"], vel)
    q, qd = np.where(stance[..., None], q1, o["q"]), np.where(stance[..., None], qd1, o["qd"])
    if noise:
        rng = np.random.default_rng(NOISE_SEED)
        imu = imu + rng.normal(0.0, 1.0, imu.shape) * np.array([0.01] * 3 + [0.1] * 3)
        q, qd = q + rng.normal(0.0, 1e-3, q.shape), qd + rng.normal(0.0, 0.05, qd.shape)
    return imu, q, qd


@functools.lru_cache(maxsize=None)
def log_pass(ground, noise, gated):
    """estimate_track_host over `sensors(ground, noise)`, init = the first actual row, no height rows: ungated, or at the defaults."""
    o = slip_run(ground)
    imu, q, qd = sensors(ground, noise)
    return estimator.estimate_track_host(imu, q, qd, o["contact_log"], o["actual"][:, 0], delta=DELTA, gate=GATE if gated else None)


def rms_vxy(est, actual):
    d = np.asarray(est, np.float64) - np.asarray(actual, np.float64)
    return np.sqrt(np.nanmean((d[..., 9:11] ** 2).sum(-1), axis=1))


def rms_pz(est, actual):
    d = np.asarray(est, np.float64) - np.asarray(actual, np.float64)
    return np.sqrt(np.nanmean(d[..., 5] ** 2, axis=1))


def sliding(o):
    """Stance leg-rows the plant marks sliding (bit 128), and all stance leg-rows that are not poisoned."""
    flag, stance = np.asarray(o["flag"]), np.asarray(o["contact_log"]) != 0
    live = stance & (flag != 0xff)
    return live & ((flag & 128) != 0), live


@functools.lru_cache(maxsize=None)
def closed_loop_host(ground, gated):
    """tools/observe_report.py's roll-out with feed = "estimate": the eight gaits, land = rule, no noise, no height rows."""
    pb = gait_batch()
    return gaits.rollout_observe_host(checker(), *_head(pb), GAIT_T, np.full(GAIT_B, STEP_HEIGHT), np.full(GAIT_B, ground),
                                      lite3_model.foot_mass(), feed="estimate", gate=GATE if gated else None)


def loop_figures(o):
    """(lowest CoM [m], worst tilt [rad], ticks solved) per robot of a closed-loop run's logs (numpy)."""
    s = score.summarize(score.score_host(o), DELTA)
    with np.errstate(invalid="ignore"):
        low = np.nanmin(np.asarray(o["actual"], np.float64)[..., 5], axis=1)
    return low, np.asarray(s["tilt_max"]), np.asarray(o["solved"])


def check_flying_trot(tag, ungated, gated):
    """The closed-loop conditions on ground 0.3, feed = "estimate", flying trot, 36 ticks.  The host study: 192.8 mm without the gate;
    283.0 mm and 0.076 rad with it."""
    b = NAMES.index("flying_trot")
    (l0, t0, s0), (l1, t1, s1) = loop_figures(ungated), loop_figures(gated)
    print(f"{tag} flying trot on ground 0.3, feed = estimate: ungated lowest CoM {1e3 * l0[b]:.1f} mm, tilt {t0[b]:.3f} rad, solved {int(s0[b])}; "
          f"gated lowest CoM {1e3 * l1[b]:.1f} mm, tilt {t1[b]:.3f} rad, solved {int(s1[b])}")
    assert l0[b] < 0.230
    assert l1[b] > 0.250 and t1[b] < 0.2
    assert int(s0[b]) == GAIT_T and int(s1[b]) == GAIT_T
