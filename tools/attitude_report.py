"""Developer tool: what the velocity-aided attitude rule (include/mpcqp_attitude.h, estimator.estimate_track_host(attitude=)) makes of
a roll-out's logs, and of the closed loop, on the host.  The log pass is tools/estimate_report.py's setup: one robot per named gait at
period 12, 36 ticks of gaits.rollout_slip_host on the CPU checker on ground 1e3 (land = actual), noise-free sensors, init = the first
actual row, no height rows.  It prints per gait the RMS tilt error of today's filter (attitude = None), of the gyro-only setting (k_s =
k_v = k_b = 0) and of the aided rule at its defaults, without and with a gyro bias of 0.02 rad/s on all three axes, then the RMS v_xy
and p_z errors, and b^ at the last row against the injected bias over 36 and over 72 rows.  The closed loop is
gaits.rollout_observe_host with feed = "estimate" (land = rule) on ground 1e3 and 0.3, without and with the trust gate, without and
with the rule, with a gyro bias of 0.02 rad/s injected through bias=: per gait the lowest CoM height, whether the robot falls under
score's default rule, the RMS tilt and v_xy errors of the estimate, and b^ at the last row.  A report: nothing is asserted.
usage: python tools/attitude_report.py [--no-loop]"""
import os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import estimator, gaits, lite3_model, plant, score

T, DELTA, STEP_HEIGHT, BIAS = 36, 0.03, 0.06, 0.02
GYRO_ONLY = {"k_s": 0.0, "k_v": 0.0, "k_b": 0.0}
names = tuple(gaits.GAITS)
B = len(names)
lib = mpcqp.Library(os.path.join(REPO, "oracle", "libmpcqp_oracle.so"))
eng = mpcqp.Engine(lib, lib.default_config(N=10, delta=DELTA, max_iter=4000))
pb = gaits.make_phase_batch(B, names, 12, seed=6)
head = [pb[k] for k in ("x", "ref", "feet")] + [np.zeros((B, 4, 7))] + [pb[k] for k in ("gait", "stand", "gain", "tick", "mu")]


def tilt_error(est, actual):
    zt = plant.quat_to_matrix(plant.rotvec_to_quat(actual[..., 0:3]))[..., :, 2]
    ze = plant.quat_to_matrix(plant.rotvec_to_quat(est[..., 0:3]))[..., :, 2]
    return np.arccos(np.clip((zt * ze).sum(-1), -1.0, 1.0))


def rms(a):
    return np.sqrt(np.nanmean(a * a, axis=1))


def sensors(o):
    n = o["actual"].shape[1]
    acc = lite3_model.plant_base_acc_host(o["actual"], o["forces"], o["feet_log"])
    imu = estimator.imu_log_host(o["actual"], o["forces"], o["feet_log"], base_acc=acc)
    stance = np.asarray(o["contact_log"]) != 0
    vel = np.zeros((B, n, 4, 3))
    vel[..., :2] = np.where(stance[..., None], o["slip_log"], 0.0)
    q1, qd1, _, _, _ = lite3_model.joint_rates_host(o["actual"], o["forces"], o["feet_log"], vel)
    return imu, np.where(stance[..., None], q1, o["q"]), np.where(stance[..., None], qd1, o["qd"])


def table(title, rows, scale, fmt):
    print(title)
    print("  " + " | ".join(["setting".ljust(28)] + [n.rjust(11) for n in names]))
    for label, v in rows:
        print("  " + " | ".join([label.ljust(28)] + [format(x * scale, fmt).rjust(11) for x in v]))


def log_pass(n):
    o = gaits.rollout_slip_host(eng, *head, n, np.full(B, STEP_HEIGHT), np.full(B, 1e3), lite3_model.foot_mass(), land="actual")
    imu, q, qd = sensors(o)
    out = {}
    for bias in (0.0, BIAS):
        im = imu.copy()
        im[..., 0:3] += bias
        for label, att in (("today (kappa = 2)", None), ("gyro only", GYRO_ONLY), ("aided (defaults)", {})):
            out[label, bias] = estimator.estimate_track_host(im, q, qd, o["contact_log"], o["actual"][:, 0], delta=DELTA, attitude=att)
    return o, out


o, runs = log_pass(T)
for bias in (0.0, BIAS):
    table(f"log pass, ground 1e3, {T} rows, gyro bias {bias} rad/s: RMS tilt error [mrad]",
          [(k[0], rms(tilt_error(e["est"], o["actual"]))) for k, e in runs.items() if k[1] == bias], 1e3, ".1f")
vxy = lambda e: np.sqrt(np.nanmean(((e["est"] - o["actual"])[..., 9:11] ** 2).sum(-1), axis=1))
table("no bias: RMS v_xy error [mm/s]", [(k[0], vxy(e)) for k, e in runs.items() if k[1] == 0.0], 1e3, ".0f")
table("no bias: RMS p_z error [mm]", [(k[0], rms((e["est"] - o["actual"])[..., 5])) for k, e in runs.items() if k[1] == 0.0], 1e3, ".0f")
for n in (T, 2 * T):
    bh = (runs if n == T else log_pass(n)[1])["aided (defaults)", BIAS]["att_state"][:, 0:3]
    print(f"b^ after {n} rows for a true ({BIAS}, {BIAS}, {BIAS}) rad/s:")
    for b, name in enumerate(names):
        print(f"  {name:12s} | " + " ".join(f"{v:8.4f}" for v in bh[b]))

if "--no-loop" not in sys.argv:
    bias = np.zeros((B, 6))
    bias[:, 0:3] = BIAS
    for ground in (1e3, 0.3):
        for gate in (None, {}):
            for att in (None, {}):
                c = gaits.rollout_observe_host(eng, *head, T, np.full(B, STEP_HEIGHT), np.full(B, ground), lite3_model.foot_mass(),
                                               feed="estimate", bias=bias, gate=gate, attitude=att)
                s = score.summarize(score.score_host(c), DELTA)
                with np.errstate(invalid="ignore"):
                    low = np.nanmin(c["actual"][..., 5], axis=1)
                d = c["est"] - c["actual"]
                print(f"closed loop, ground {ground:g}, gyro bias {BIAS}, gate {'on' if gate is not None else 'off'}, "
                      f"attitude {'aided' if att is not None else 'today'}: gait | lowest CoM [mm] | fell | RMS tilt error [mrad] | "
                      f"RMS v_xy error [mm/s] | b^ at the last row")
                for b, name in enumerate(names):
                    bh = " ".join(f"{v:7.4f}" for v in c["att_state"][b, 0:3]) if att is not None else "-"
                    print(f"  {name:12s} | {low[b] * 1e3:6.1f} | {int(np.asarray(s['fell'])[b]):d} | {rms(tilt_error(c['est'], c['actual']))[b] * 1e3:7.1f} | "
                          f"{np.sqrt(np.nanmean((d[..., 9:11] ** 2).sum(-1), axis=1))[b] * 1e3:7.1f} | {bh}")
