"""Cases shared by tests/test_rollout_observe_host.py and tests/test_gpu_rollout_observe.py (include/mpcqp_observe.h,
mpcqp_rollout_observe): the sensor draws of the legsim batch, the six-robot feedback case and its conditions."""
import numpy as np

import drive_cases as dc
from legsim_cases import ROLL_B, ROLL_T
from mpcqp import gaits, lite3_model, synth

SENSOR_SEED = 25
EST_LOGS = ("imu", "q_enc", "qd_enc", "est", "feet_est", "sigma", "nis")
ICE = 0.3
FEED_B, FEED_T, FEED_TAIL, FEED_OFFSET = 6, 60, 10, 0.04


def sensor_draw(B=ROLL_B, T=ROLL_T, seed=SENSOR_SEED):
    """Bias [B,6], IMU noise [B,T,6] and encoder noise [B,T,4,6], drawn once with a fixed seed and non-zero for the odd robots only:
    gyro 0.01 rad/s and accelerometer 0.05 m/s^2 of noise, 0.005 / 0.03 of bias, encoders 1e-3 rad and 0.02 rad/s."""
    rng = np.random.default_rng(seed)
    on = (np.arange(B) % 2 == 1).astype(np.float64)
    bias = rng.normal(0.0, 1.0, (B, 6)) * np.array([0.005] * 3 + [0.03] * 3) * on[:, None]
    noise = rng.normal(0.0, 1.0, (B, T, 6)) * np.array([0.01] * 3 + [0.05] * 3) * on[:, None, None]
    enc = rng.normal(0.0, 1.0, (B, T, 4, 6)) * np.array([1e-3] * 3 + [0.02] * 3) * on[:, None, None, None]
    return {"bias": bias, "noise": noise, "enc_noise": enc, "noisy": on != 0}


def ground_rows(B=ROLL_B):
    """Ground 0.3 under the even robots, 1e3 under the odd ones (tests/test_gpu_stance_drive.py's rows)."""
    return np.where(np.arange(B) % 2 == 0, dc.GROUND_MU, 1e3)


def feedback_batch():
    """The six robots of the feedback case: stand, trot and walk at period 12, no reference velocity, with a leg state, step heights
    and an est_init that is the first state with p_z + 0.04 m."""
    pb = gaits.make_phase_batch(FEED_B, ("stand", "trot", "walk"), 12, seed=6, v_ref=(0.0, 0.0, 0.0))
    pb["legs"] = np.zeros((FEED_B, 4, 7))
    pb["step_height"] = np.full(FEED_B, 0.06)
    pb["est_init"] = pb["x"][:, :12].copy()
    pb["est_init"][:, 5] += FEED_OFFSET
    pb["height"] = pb["stand"][:, :, 2].copy()
    pb["ground"] = np.full(FEED_B, 1e3)
    pb["foot_mass"] = np.full(FEED_B, lite3_model.foot_mass())
    return pb


def feedback_figures(actual, est, z_ref=synth.H_COM):
    """Over the last FEED_TAIL rows of the feedback case: (max |z^ - z_ref|, mean(z^ - z) per robot, min and max |z - z_ref|) in m."""
    z, zh = actual[:, -FEED_TAIL:, 5], est[:, -FEED_TAIL:, 5]
    return float(np.abs(zh - z_ref).max()), (zh - z).mean(axis=1), float(np.abs(z - z_ref).min()), float(np.abs(z - z_ref).max())


def check_feedback(tag, blind, seen, solved_blind, solved_seen):
    """The conditions of the feedback case on the logs of the run without height rows (blind) and with them (seen); (actual, est) each.
    Without height rows the absolute height is unobservable and the controller regulates the wrong height; with them the offset is
    gone.  The thresholds are conditions -- a factor of two or more over the values the rule was specified with (4.6 mm, 40.0-41.9 mm,
    38.5-45.1 mm, 3.5 mm) and a factor of three or more below the 40 mm signal --, not measurements of the code under test."""
    zh_err, off, lo, hi = feedback_figures(*blind)
    print(f"{tag} no height rows: |z^ - z_ref| <= {1e3 * zh_err:.2f} mm, mean(z^ - z) {1e3 * off.min():.2f} .. {1e3 * off.max():.2f} mm, "
          f"|z - z_ref| {1e3 * lo:.2f} .. {1e3 * hi:.2f} mm")
    _, off2, _, hi2 = feedback_figures(*seen)
    print(f"{tag} with height rows: |z - z_ref| <= {1e3 * hi2:.2f} mm, mean(z^ - z) {1e3 * off2.min():.2f} .. {1e3 * off2.max():.2f} mm")
    assert zh_err < 0.010
    assert (np.abs(off - FEED_OFFSET) < 0.005).all()
    assert lo > 0.030
    assert hi2 < 0.010
    assert (np.asarray(solved_blind) == FEED_T).all() and (np.asarray(solved_seen) == FEED_T).all()
