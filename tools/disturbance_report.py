"""Developer tool, host only: what telling the MPC a disturbance is worth in closed loop, on the CPU checker (include/mpcqp_disturb.h;
mpcqp.disturbance).  The eight named gaits of mpcqp.gaits at period 12, one robot each, 36 ticks of gaits.rollout_phase_host.  Every
robot sees a constant 10 N forward push and 1 N m of yaw torque (`push`) and carries a 2 kg payload that only the plant knows (`body`).
Four runs:

    not told     no table
    told         the table holds the truth: the push, and the payload's weight as F_z = -2 kg x 9.81 m/s^2
    observer 1   compensated_rollout at piece = 1: the observer (default parameters, the configuration's body, truth logs) sets the
                 table after every tick
    observer 6   the same at piece = 6

For each: the final and the worst CoM error |p - p_ref| in mm, the final and the worst yaw error in mrad, the last estimate (F_x, F_z,
tau_z) and the ticks solved.  Prints a markdown table and writes it to profiles/r29_disturbance_report.txt (or --out PATH).
A report: nothing is asserted, worse cases are printed as they come out.
usage: disturbance_report.py [--out PATH]"""
import os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import disturbance, gaits, plant

T, PERIOD, PAYLOAD, G = 36, 12, 2.0, -9.81
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r29_disturbance_report.txt")
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


def run(kind, piece=1):
    eng = disturbance.DisturbedEngine(mpcqp.Engine(lib, cfg), truth if kind == "told" else None)
    st = {k: pb[k].copy() for k in ("x", "ref", "feet", "tick")}

    def step(n):
        o = gaits.rollout_phase_host(eng, st["x"], st["ref"], st["feet"], pb["gait"], pb["stand"], pb["gain"], st["tick"], pb["mu"], n,
                                     body=body, push=push, push_ticks=ticks)
        st.update({k: o[k] for k in ("x", "ref", "feet", "tick")})
        return o
    if kind != "observer":
        return step(T), None
    out = disturbance.compensated_rollout(step, T, piece, lambda logs, state: disturbance.disturbance_track_host(logs, eng.cfg, state=state),
                                          eng.set_rows)
    return out["logs"], out["dist"][:, -1]


lines = [f"Closed loop on the CPU checker, {T} ticks, period {PERIOD}: 10 N forward push, 1 N m yaw torque, {PAYLOAD:g} kg payload in `body` only; "
         "tools/disturbance_report.py", "",
         "| gait | run | CoM error final / worst [mm] | yaw error final / worst [mrad] | estimate F_x, F_z [N], tau_z [N m] | solved |",
         "|---|---|---|---|---|---|"]
for kind, piece, label in (("untold", 1, "not told"), ("told", 1, "told"), ("observer", 1, "observer 1"), ("observer", 6, "observer 6")):
    logs, est = run(kind, piece)
    ep = 1e3 * np.linalg.norm(logs["actual"][:, :, 3:6] - logs["desired"][:, :, 3:6], axis=2)
    ey = 1e3 * (logs["actual"][:, :, 2] - logs["desired"][:, :, 2])
    for b, name in enumerate(NAMES):
        e = "" if est is None else f"{est[b, 0]:.2f}, {est[b, 2]:.2f}, {est[b, 5]:.3f}"
        lines.append(f"| {name} | {label} | {ep[b, -1]:.1f} / {ep[b].max():.1f} | {ey[b, -1]:.1f} / {np.abs(ey[b]).max():.1f} | {e} | "
                     f"{int(logs['solved'][b])} / {T} |")
print("\n".join(lines))
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
