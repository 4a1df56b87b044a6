"""Developer tool: what the state estimate does to the closed loop (gaits.rollout_observe_host, include/mpcqp_observe.h), on the host.
One robot per named gait at period 12, 36 ticks on the CPU checker (land = rule, nominal foot mass, no sensor noise, no height rows,
est_init = the first state, default gains), on ground 1e3 and on ground 0.3, each once with feed = "truth" (the estimator only shadows
the loop) and once with feed = "estimate" (the MPC reads the estimate).  Prints per gait the ticks solved, the lowest CoM, the worst
tilt, the RMS height and velocity tracking error, the worst |z^ - z| and whether the robot falls under score's default rule.  A report:
nothing is asserted.
usage: python tools/observe_report.py"""
import os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import gaits, lite3_model, score

T, DELTA, STEP_HEIGHT = 36, 0.03, 0.06
names = tuple(gaits.GAITS)
B = len(names)
lib = mpcqp.Library(os.path.join(REPO, "oracle", "libmpcqp_oracle.so"))
eng = mpcqp.Engine(lib, lib.default_config(N=10, delta=DELTA, max_iter=4000))
pb = gaits.make_phase_batch(B, names, 12, seed=6)


def run(ground, feed):
    return gaits.rollout_observe_host(eng, pb["x"], pb["ref"], pb["feet"], np.zeros((B, 4, 7)), pb["gait"], pb["stand"], pb["gain"], pb["tick"],
                                      pb["mu"], T, np.full(B, STEP_HEIGHT), np.full(B, ground), lite3_model.foot_mass(), feed=feed)


for ground in (1e3, 0.3):
    for feed in ("truth", "estimate"):
        o = run(ground, feed)
        s = score.summarize(score.score_host(o), DELTA)
        with np.errstate(invalid="ignore"):
            dz = np.nanmax(np.abs(o["est"][..., 5] - o["actual"][..., 5]), axis=1)
            low = np.nanmin(o["actual"][..., 5], axis=1)
        print(f"ground {ground:g}, feed = {feed}: gait | solved | lowest CoM [mm] | worst tilt [rad] | RMS z error [mm] | "
              f"RMS v error [mm/s] | worst |z^ - z| [mm] | falls")
        for b, n in enumerate(names):
            print(f"  {n:12s} | {int(o['solved'][b]):2d}/{T} | {low[b] * 1e3:7.1f} | {s['tilt_max'][b]:6.3f} | {s['z_rms'][b] * 1e3:7.2f} | "
                  f"{s['vel_rms'][b] * 1e3:7.1f} | {dz[b] * 1e3:7.1f} | {'row %d' % int(s['fall_row'][b]) if s['fell'][b] else 'no'}")
