"""Developer tool: what the state estimator (mpcqp.estimator, include/mpcqp_estimate.h) makes of a roll-out's logs, on the host.  One
robot per named gait at period 12, 36 ticks of gaits.rollout_slip_host on the CPU checker (land = actual, nominal foot mass), the IMU
rows from estimator.imu_log_host on the plant's right-hand side under the applied forces, the encoders from the roll-out's q / qd logs
(stance rows of a sliding foot: lite3_model.joint_rates_host with the foot's logged velocity), init = the first actual row, no height
rows, default gains.  Three cases: noise-free sensors on ground 1e3 (no foot moves), the same with sensor noise (sigma gyro 0.01 rad/s,
accelerometer 0.1 m/s^2, q 1e-3 rad, qd 0.05 rad/s), and noise-free on ground 0.3, where stance feet slide.  Prints per gait the RMS
error of p_z, v_xy and the tilt (the angle between the true and the estimated torso z axis) and the mean nis.  A report: nothing is
asserted.
usage: python tools/estimate_report.py"""
import os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import estimator, gaits, lite3_model, plant

T, DELTA, STEP_HEIGHT = 36, 0.03, 0.06
names = tuple(gaits.GAITS)
B = len(names)
lib = mpcqp.Library(os.path.join(REPO, "oracle", "libmpcqp_oracle.so"))
eng = mpcqp.Engine(lib, lib.default_config(N=10, delta=DELTA, max_iter=4000))
pb = gaits.make_phase_batch(B, names, 12, seed=6)


def run(ground):
    return gaits.rollout_slip_host(eng, pb["x"], pb["ref"], pb["feet"], np.zeros((B, 4, 7)), pb["gait"], pb["stand"], pb["gain"], pb["tick"],
                                   pb["mu"], T, np.full(B, STEP_HEIGHT), np.full(B, ground), lite3_model.foot_mass(), land="actual")


def sensors(o, noise):
    acc = lite3_model.plant_base_acc_host(o["actual"], o["forces"], o["feet_log"])
    imu = estimator.imu_log_host(o["actual"], o["forces"], o["feet_log"], base_acc=acc)
    stance = np.asarray(o["contact_log"]) != 0
    vel = np.zeros((B, T, 4, 3))
    vel[..., :2] = np.where(stance[..., None], o["slip_log"], 0.0)
    q1, qd1, _, _, _ = lite3_model.joint_rates_host(o["actual"], o["forces"], o["feet_log"], vel)
    q, qd = np.where(stance[..., None], q1, o["q"]), np.where(stance[..., None], qd1, o["qd"])
    if noise:
        rng = np.random.default_rng(24)
        imu = imu + rng.normal(0.0, 1.0, imu.shape) * np.array([0.01] * 3 + [0.1] * 3)
        q, qd = q + rng.normal(0.0, 1e-3, q.shape), qd + rng.normal(0.0, 0.05, qd.shape)
    return imu, q, qd


def figures(o, noise):
    imu, q, qd = sensors(o, noise)
    e = estimator.estimate_track_host(imu, q, qd, o["contact_log"], o["actual"][:, 0], delta=DELTA)
    d = e["est"] - o["actual"]
    zt = plant.quat_to_matrix(plant.rotvec_to_quat(o["actual"][..., 0:3]))[..., :, 2]
    ze = plant.quat_to_matrix(plant.rotvec_to_quat(e["est"][..., 0:3]))[..., :, 2]
    tilt = np.arccos(np.clip((zt * ze).sum(-1), -1.0, 1.0))
    rms = lambda a: np.sqrt(np.nanmean(a * a, axis=1))
    slid = ((np.asarray(o["flag"]) & 128) != 0) & (np.asarray(o["flag"]) != 0xff)
    return rms(d[..., 5]), np.sqrt(np.nanmean((d[..., 9:11] ** 2).sum(-1), axis=1)), rms(tilt), np.nanmean(e["nis"], axis=1), slid.sum(axis=(1, 2))


firm, ice = run(1e3), run(0.3)
for title, o, noise in (("noise-free sensors, ground 1e3", firm, False), ("sensor noise, ground 1e3", firm, True),
                        ("noise-free sensors, ground 0.3", ice, False)):
    pz, vxy, tilt, nis, slid = figures(o, noise)
    print(f"{title}: gait | RMS p_z error [mm] | RMS v_xy error [mm/s] | RMS tilt error [mrad] | mean nis | sliding leg-rows")
    for b, n in enumerate(names):
        print(f"  {n:12s} | {pz[b] * 1e3:7.2f} | {vxy[b] * 1e3:7.1f} | {tilt[b] * 1e3:7.2f} | {nis[b]:9.3f} | {int(slid[b]):3d}")
