"""Developer tool, host only: what the wrench observer inside the roll-out's tick is worth in closed loop, on the CPU checker
(include/mpcqp_compensate.h; disturbance.rollout_compensated_host).  The eight named gaits of mpcqp.gaits at period 12, one robot each,
36 ticks of the leg roll-out on a ground that never limits, no sensor noise, an exact est_init and height rows.  Every robot sees a
constant 10 N forward push and 1 N m of yaw torque (`push`) and carries a 2 kg payload that only the plant knows (`body`); the observer
believes the configuration's body.  The controller reads the estimate (feed = "estimate") in every run but the first two.  Runs:

    not told          gaits.rollout_observe_host, feed = "truth", no table
    told              the table holds the truth: the push, and the payload's weight as F_z = -2 kg x 9.81 m/s^2 (feed = "truth")
    truth 1           hold = 1, the observer reads the plant's truth (feed = "truth")
    sensed 1          hold = 1, the observer reads the estimate, the commanded forces and the estimated feet; plain estimator
    sensed 1 gate     the same with gate = {}
    sensed 1 aided    the same with gate = {} and attitude = {}

For each: the final and the worst CoM error |p - p_ref| in mm, the final and the worst yaw error in mrad, the last estimate (F_x, F_z,
tau_z) and the ticks solved.  Prints a markdown table and writes it to profiles/r31_compensate_report.txt (or --out PATH).
A report: nothing is asserted, worse cases are printed as they come out.
usage: compensate_report.py [--out PATH]"""
import os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import disturbance, gaits, lite3_model, plant

T, PERIOD, PAYLOAD, G = 36, 12, 2.0, -9.81
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r31_compensate_report.txt")
NAMES = tuple(gaits.GAITS)
B = len(NAMES)

lib = mpcqp.Library(os.path.join(REPO, "oracle", "libmpcqp_oracle.so"))
cfg = lib.default_config(N=10, delta=0.03, max_iter=4000)
pb = gaits.make_phase_batch(B, NAMES, PERIOD, seed=31)
push = np.tile(np.array([10.0, 0.0, 0.0, 0.0, 0.0, 1.0]), (B, 1))
ticks = np.tile(np.array([[0, 1 << 20]], np.int32), (B, 1))
body = plant.model_body(cfg.m, list(cfg.Ibody_inv), B)
body[:, 0] += PAYLOAD
truth = push.copy()
truth[:, 2] = PAYLOAD * G
args = (pb["x"], pb["ref"], pb["feet"], np.zeros((B, 4, 7)), pb["gait"], pb["stand"], pb["gain"], pb["tick"], pb["mu"], T, np.full(B, 0.06),
        np.full(B, 1e3), np.full(B, lite3_model.foot_mass()))
common = dict(est_init=pb["x"][:, :12].copy(), height=pb["stand"][:, :, 2].copy(), body=body, push=push, push_ticks=ticks)


def run(kind, **kw):
    if kind in ("untold", "told"):
        eng = disturbance.DisturbedEngine(mpcqp.Engine(lib, cfg), truth if kind == "told" else None)
        return gaits.rollout_observe_host(eng, *args, feed="truth", **common), None
    out = disturbance.rollout_compensated_host(mpcqp.Engine(lib, cfg), *args, compensate={"source": kind, "hold": 1}, **common, **kw)
    return out, out["dist"][:, -1]


lines = [f"Closed loop of the leg roll-out on the CPU checker, {T} ticks, period {PERIOD}: 10 N forward push, 1 N m yaw torque, {PAYLOAD:g} kg payload in "
         "`body` only; tools/compensate_report.py", "",
         "| gait | run | CoM error final / worst [mm] | yaw error final / worst [mrad] | estimate F_x, F_z [N], tau_z [N m] | solved |",
         "|---|---|---|---|---|---|"]
for kind, kw, label in (("untold", {}, "not told"), ("told", {}, "told"), ("truth", {"feed": "truth"}, "truth 1"),
                        ("sensed", {"feed": "estimate"}, "sensed 1"), ("sensed", {"feed": "estimate", "gate": {}}, "sensed 1 gate"),
                        ("sensed", {"feed": "estimate", "gate": {}, "attitude": {}}, "sensed 1 aided")):
    logs, est = run(kind, **kw)
    ep = 1e3 * np.linalg.norm(logs["actual"][:, :, 3:6] - logs["desired"][:, :, 3:6], axis=2)
    ey = 1e3 * (logs["actual"][:, :, 2] - logs["desired"][:, :, 2])
    for b, name in enumerate(NAMES):
        e = "" if est is None else f"{est[b, 0]:.2f}, {est[b, 2]:.2f}, {est[b, 5]:.3f}"
        lines.append(f"| {name} | {label} | {ep[b, -1]:.1f} / {np.nanmax(ep[b]):.1f} | {ey[b, -1]:.1f} / {np.nanmax(np.abs(ey[b])):.1f} | {e} | "
                     f"{int(logs['solved'][b])} / {T} |")
print("\n".join(lines))
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
