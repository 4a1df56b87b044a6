"""Developer tool: what the trust gate (include/mpcqp_gate.h) does to the state estimate and to the closed loop, on the host, with the
set-ups of tools/estimate_report.py and tools/observe_report.py: one robot per named gait at period 12, 36 ticks on the CPU checker,
seed 6, default gains, default thresholds (1, 4).

  log pass     gaits.rollout_slip_host (land = actual) on ground 1e3 and 0.3; sensors as in tools/estimate_report.py, noise-free and
               with its sensor noise; estimator.estimate_track_host without and with gate={}.  Per gait: RMS v_xy and p_z error, mean
               nis, the largest d over stance leg-rows, and how many sliding (bit 128) and held stance leg-rows have w < 1.
  closed loop  gaits.rollout_observe_host (land = rule, no noise, no height rows) with feed = "estimate" on ground 1e3 and 0.3, without
               and with gate={}.  Per gait: ticks solved, lowest CoM, worst tilt, whether the robot falls under score's default rule.
A report: nothing is asserted.
usage: python tools/gate_report.py"""
import os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import estimator, gaits, lite3_model, score

T, DELTA, STEP_HEIGHT = 36, 0.03, 0.06
names = tuple(gaits.GAITS)
B = len(names)
lib = mpcqp.Library(os.path.join(REPO, "oracle", "libmpcqp_oracle.so"))
eng = mpcqp.Engine(lib, lib.default_config(N=10, delta=DELTA, max_iter=4000))
pb = gaits.make_phase_batch(B, names, 12, seed=6)
head = [pb["x"], pb["ref"], pb["feet"], np.zeros((B, 4, 7)), pb["gait"], pb["stand"], pb["gain"], pb["tick"], pb["mu"], T, np.full(B, STEP_HEIGHT)]


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


def errors(e, o):
    d = e["est"] - o["actual"]
    return np.sqrt(np.nanmean(d[..., 5] ** 2, axis=1)), np.sqrt(np.nanmean((d[..., 9:11] ** 2).sum(-1), axis=1)), np.nanmean(e["nis"], axis=1)


for ground in (1e3, 0.3):
    o = gaits.rollout_slip_host(eng, *head, np.full(B, ground), lite3_model.foot_mass(), land="actual")
    flag, stance = np.asarray(o["flag"]), np.asarray(o["contact_log"]) != 0
    live = stance & (flag != 0xff)
    slid = live & ((flag & 128) != 0)
    for noise in (False, True):
        imu, q, qd = sensors(o, noise)
        a = estimator.estimate_track_host(imu, q, qd, o["contact_log"], o["actual"][:, 0], delta=DELTA)
        g = estimator.estimate_track_host(imu, q, qd, o["contact_log"], o["actual"][:, 0], delta=DELTA, gate={})
        same = all(np.array_equal(a[k], g[k], equal_nan=True) for k in estimator.OUT + ("state",))
        (pz0, v0, n0), (pz1, v1, n1) = errors(a, o), errors(g, o)
        print(f"log pass, ground {ground:g}, {'sensor noise' if noise else 'noise-free sensors'} (every output the ungated filter's bit for bit: "
              f"{same}): gait | RMS v_xy error [mm/s] ungated -> gated | RMS p_z error [mm] | mean nis | largest d on a stance leg | "
              f"sliding leg-rows with w < 1 | held leg-rows with w < 1")
        for b, n in enumerate(names):
            w, d = g["trust"][b], g["gate_d"][b]
            print(f"  {n:12s} | {v0[b] * 1e3:6.1f} -> {v1[b] * 1e3:6.1f} | {pz0[b] * 1e3:6.2f} -> {pz1[b] * 1e3:6.2f} | {n0[b]:8.3f} -> {n1[b]:7.3f} | "
                  f"{d[live[b]].max():9.3f} | {int((w[slid[b]] < 1).sum()):3d} of {int(slid[b].sum()):3d} | "
                  f"{int((w[live[b] & ~slid[b]] < 1).sum()):2d} of {int((live[b] & ~slid[b]).sum()):3d}")

for ground in (1e3, 0.3):
    runs = [gaits.rollout_observe_host(eng, *head, np.full(B, ground), lite3_model.foot_mass(), feed="estimate", gate=gate) for gate in (None, {})]
    fig = []
    for o in runs:
        s = score.summarize(score.score_host(o), DELTA)
        with np.errstate(invalid="ignore"):
            fig.append((np.nanmin(o["actual"][..., 5], axis=1), s["tilt_max"], s["fell"], s["fall_row"], o["solved"]))
    same = all(np.array_equal(runs[0][k], runs[1][k], equal_nan=True) for k in runs[0])
    print(f"closed loop, ground {ground:g}, feed = estimate (every log the ungated loop's bit for bit: {same}): gait | solved ungated -> gated | "
          f"lowest CoM [mm] | worst tilt [rad] | falls")
    fall = lambda f, b: "row %d" % int(f[3][b]) if f[2][b] else "no"
    for b, n in enumerate(names):
        print(f"  {n:12s} | {int(fig[0][4][b]):2d} -> {int(fig[1][4][b]):2d} of {T} | {fig[0][0][b] * 1e3:7.1f} -> {fig[1][0][b] * 1e3:7.1f} | "
              f"{fig[0][1][b]:6.3f} -> {fig[1][1][b]:6.3f} | {fall(fig[0], b)} -> {fall(fig[1], b)}")
