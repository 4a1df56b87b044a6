"""Cases shared by tests/test_attitude_host.py and tests/test_gpu_attitude.py (include/mpcqp_attitude.h, mpcqp_estimate_track_aided
and mpcqp_rollout_observe_aided):

  gains      ATT (the defaults, spelled out), IDENTITY (k_s = 1, k_v = k_b = 0: the unaided row as values), GYRO_ONLY (all three zero).
  real       estimate_cases.real_case, the 16 x 25 logs.
  edges      estimate_cases.edge_case at B in {1, 15, 16, 17, 63, 64, 65, 257} x T in {1, 2, 25}: 16 robots fill a wave, 64 a block.
  live       a live filter state and a non-zero att_state for an edge case: the unaided host's state after the case's rows, and b^
             drawn with sigma 0.01 rad/s (e_b and the reserved pair zero).
  gaits      gate_cases' eight-gait batch (tools/estimate_report.py's setup: 36 rows, ground 1e3, noise-free, exact init) and the RMS
             tilt error of an estimate against its truth.
  standing   STAND_B robots standing still for STAND_T rows, feet fixed in the world, exact encoders: the convergence case.

and the growth factor of the aided rule: estimate_cases.measure_growth's figure with attitude = ATT, recorded in
tests/golden/attitude_growth.npz (`python tests/golden/attitude_growth.py` regenerates it)."""
import functools
import os

import numpy as np

import estimate_cases as C
from legsim_cases import DELTA
from mpcqp import estimator, gaits, lite3_model, plant

GROWTH_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attitude_growth.npz")
ATT = {"k_s": 0.0, "k_v": 2.0, "k_b": 5.0, "b_max": 0.1}
IDENTITY = {"k_s": 1.0, "k_v": 0.0, "k_b": 0.0}
GYRO_ONLY = {"k_s": 0.0, "k_v": 0.0, "k_b": 0.0}
OUT = estimator.OUT + ("gyro_bias",)
EDGE_B, EDGE_T = (1, 15, 16, 17, 63, 64, 65, 257), (1, 2, 25)
STAND_B, STAND_T = 4, 300
STAND_TILT, STAND_BIAS = 0.1, (0.02, -0.015, 0.01)


def growth():
    return float(np.load(GROWTH_NPZ)["growth"])


def measure_growth(eps=1e-10, seed=11):
    """estimate_cases.measure_growth under the aided rule: the worst relative change of an output or of b^ over the real case's 25 rows
    under perturbations of eps of the start state and the operands, over eps."""
    ops = C.operands(C.real_case())
    rng = np.random.default_rng(seed)
    pert = {k: (v + eps * rng.choice([-1.0, 1.0], v.shape) if k in ("imu", "q", "qd", "init") else v) for k, v in ops.items()}
    a = estimator.estimate_track_host(**ops, delta=DELTA, attitude=ATT)
    b = estimator.estimate_track_host(**pert, delta=DELTA, attitude=ATT)
    return max(float((np.abs(a[k] - b[k]) / np.maximum(1.0, np.abs(a[k]))).max()) for k in OUT + ("att_state",)) / eps


def edge_pairs():
    return [(B, T) for B in EDGE_B for T in EDGE_T]


@functools.lru_cache(maxsize=None)
def live_state(B, T, with_height, io):
    """(est_state [B,131] live, att_state [B,8] with a non-zero b^) for the edge case as the I/O dtype holds it."""
    case = C.as_io(C.edge_case(B, T, with_height), io)
    st = estimator.estimate_track_host(**C.operands(case), delta=DELTA)["state"]
    att = np.zeros((B, estimator.ATT_STATE))
    att[:, 0:3] = np.random.default_rng(7 * B + T).normal(0.0, 0.01, (B, 3))
    return st, att


def tilt_error(est, actual):
    """The angle between the true and the estimated torso z axis, per row."""
    zt = plant.quat_to_matrix(plant.rotvec_to_quat(np.asarray(actual, np.float64)[..., 0:3]))[..., :, 2]
    ze = plant.quat_to_matrix(plant.rotvec_to_quat(np.asarray(est, np.float64)[..., 0:3]))[..., :, 2]
    return np.arccos(np.clip((zt * ze).sum(-1), -1.0, 1.0))


def rms_tilt(est, actual):
    t = tilt_error(est, actual)
    return np.sqrt(np.nanmean(t * t, axis=1))


@functools.lru_cache(maxsize=None)
def gait_pass(bias, setting):
    """estimate_track_host over gate_cases' firm-ground, noise-free sensor rows with `bias` rad/s added to the three gyro axes;
    setting "today" (attitude = None), "gyro" (GYRO_ONLY) or "aided" (the defaults)."""
    import gate_cases as G
    o = G.slip_run(G.FIRM)
    imu, q, qd = G.sensors(G.FIRM, False)
    imu = imu.copy()
    imu[..., 0:3] += bias
    att = {"today": None, "gyro": GYRO_ONLY, "aided": {}}[setting]
    return estimator.estimate_track_host(imu, q, qd, o["contact_log"], o["actual"][:, 0], delta=G.DELTA, attitude=att)


@functools.lru_cache(maxsize=None)
def standing_case():
    """STAND_B robots at rest for STAND_T rows: estimate_cases.exact_case's construction (the stand batch of seed 24, feet fixed in the
    world, encoders from joint_rates_host with the feet at rest) without its motion."""
    B, T = STAND_B, STAND_T
    pb = gaits.make_phase_batch(B, ("stand",), 12, seed=24)
    actual = np.zeros((B, T, 12))
    actual[:, :, 3:6] = pb["x"][:, None, 3:6]
    feet_log = np.ascontiguousarray(np.broadcast_to(pb["feet"][:, None], (B, T, 4, 3)))
    forces = np.zeros((B, T, 12))
    q, qd, _, _, reach = lite3_model.joint_rates_host(actual, forces, feet_log)
    assert (reach == 1).all()
    imu = estimator.imu_log_host(actual, forces, feet_log, base_acc=np.zeros((B, T, 6)))
    return {"actual": actual, "imu": imu, "q": q, "qd": qd, "contact_log": np.ones((B, T, 4), np.uint8),
            "init": np.ascontiguousarray(actual[:, 0])}


@functools.lru_cache(maxsize=None)
def standing_run(kind, setting):
    """The standing case with an initial tilt error of STAND_TILT rad (kind "tilt": about a horizontal axis that differs per robot, no
    bias) or a constant gyro bias STAND_BIAS and exact init (kind "bias"), under setting "gyro" or "aided" -> (tilt error [B,T], result)."""
    c = standing_case()
    imu, init = c["imu"].copy(), c["init"].copy()
    if kind == "tilt":
        ang = np.pi * np.arange(STAND_B) / STAND_B
        init[:, 0], init[:, 1] = STAND_TILT * np.cos(ang), STAND_TILT * np.sin(ang)
    else:
        imu[..., 0:3] += np.asarray(STAND_BIAS)
    att = {"gyro": GYRO_ONLY, "aided": {}}[setting]
    o = estimator.estimate_track_host(imu, c["q"], c["qd"], c["contact_log"], init, delta=DELTA, attitude=att)
    return tilt_error(o["est"], c["actual"]), o


def first_row_below_quarter(kind):
    """The first row from which the aided run's tilt error stays below a quarter of the gyro-only run's at the same row, over all robots
    (STAND_T if there is none)."""
    a, g = standing_run(kind, "aided")[0], standing_run(kind, "gyro")[0]
    below = (a < 0.25 * g).all(axis=0)
    bad = np.flatnonzero(~below)
    return 0 if bad.size == 0 else int(bad[-1]) + 1
