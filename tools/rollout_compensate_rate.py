"""Developer tool: what the wrench observer inside the roll-out's tick costs (include/mpcqp_compensate.h), measured in one run on one
batch: the named trot (period 12) at v_ref = 0.18 m/s, B = 65 536 and 4096 robots x T = 50 ticks, f32 buffers, ground 1e3, a constant push
of 5 to 15 N and up to 1 N m on half of the robots, all logs on, feed = "truth".  Five cases per size, each timed with a pair of device
events around everything the case enqueues, so the time a host-driven loop leaves the device idle counts:

    constant_table    rollout_observe under a table of zero rows: nine launches per tick and the solve's shift and add-back
    compensated_truth the new call at hold = 1, source "truth": one more launch per tick
    compensated_sensed  the same, source "sensed"
    table_pieces      the constant table again as T calls of one tick: what the composed loop's roll-out calls cost without its observer
                      (a one-tick call writes [B,1,...] logs, contiguous, where a call of T ticks writes rows strided by T)
    composed          disturbance.compensated_rollout at piece = 1 on the device: per tick a one-tick rollout_observe, a disturbance_track
                      over its row, a slice, a cast and a set_disturbance, driven from Python

One warm-up round, then REPS rounds that alternate the cases; prints the median and, in brackets, the spread (max - min) over the rounds
in ms per tick, and writes the lines to profiles/r31_compensate.txt (or --out PATH).  A measurement: nothing is asserted.
usage: rollout_compensate_rate.py [--size B] [--out PATH]"""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import disturbance, gaits, lite3_model

T, REPS, B0 = 50, 5, 64
SIZES = (int(sys.argv[sys.argv.index("--size") + 1]),) if "--size" in sys.argv else (65536, 4096)
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r31_compensate.txt")
CASES = ("constant_table", "compensated_truth", "compensated_sensed", "table_pieces", "composed")


def tiled(a, B, dt):
    return torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * (B // B0), axis=0)), dtype=dt).cuda().contiguous()


trot = gaits.make_phase_batch(B0, "trot", 12, seed=9)
lines = ["rollout_observe with the wrench observer in its tick against a constant table and against the loop composed on the host, ms per "
         "tick: median [spread = max - min over %d rounds]; tools/rollout_compensate_rate.py" % REPS]

for B in SIZES:
    rows = mpcqp.synth.make_plant_rows(B, seed=1, push_force=(5.0, 15.0), push_torque=(0.0, 1.0), push_start=(0, 0), push_len=(T, T))
    ms, note = {k: [] for k in CASES}, {}
    for rep in range(REPS + 1):
        for name in CASES:
            # a fresh handle per run, with its workspace and its table reserved before the clock starts
            sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed")
            sol.engine.reserve(B)
            d, pb = sol.tdtype, trot
            z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
            st = {"x": tiled(pb["x"], B, d), "ref": tiled(pb["ref"], B, d), "feet": tiled(pb["feet"], B, d), "legs": z(B, 4, 7),
                  "tick": tiled(pb["tick"], B, torch.int32), "slip": z(B, 4, 2), "est": z(B, 131), "dist": z(B, 40)}
            const = (tiled(pb["gait"], B, torch.int32), tiled(pb["stand"], B, d), tiled(pb["gain"], B, d))
            mu, hs = tiled(pb["mu"], B, d), torch.full((B,), 0.06, dtype=d, device="cuda")
            ground, me = torch.full((B,), 1e3, dtype=d, device="cuda"), torch.full((B,), lite3_model.foot_mass(), dtype=d, device="cuda")
            kw = dict(body=torch.as_tensor(rows["body"], dtype=d).cuda(), push=torch.as_tensor(rows["push"], dtype=d).cuda(),
                      push_ticks=torch.as_tensor(rows["push_ticks"]).cuda())
            roll = lambda n, **more: sol.rollout_observe(st["x"], st["ref"], st["feet"], st["legs"], *const, st["tick"], mu, n, hs, ground, me,
                                                         st["slip"], st["est"], "truth", **kw, **more)
            sol.set_disturbance(disturbance.wrench_rows(B))      # (every case starts with its table allocated and zero)
            roll(0)
            torch.cuda.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            if name == "constant_table":
                out = roll(T)
            elif name == "table_pieces":
                out = {"solved": sum(roll(1)["solved"] for _ in range(T))}
            elif name == "composed":
                out = disturbance.compensated_rollout(roll, T, 1, lambda logs, s: sol.disturbance_track(logs, state=s), sol.set_disturbance,
                                                      st["dist"])["logs"]
            else:
                out = roll(T, compensate={"source": name.split("_")[1], "hold": 1}, dist_state=st["dist"])
            ev1.record()
            torch.cuda.synchronize()
            if rep > 0:                            # (round 0 is the warm-up)
                ms[name].append(ev0.elapsed_time(ev1) / T)
            note[name] = {"all_ticks_solved": float((out["solved"].cpu().numpy() == T).mean())}
            del out, st
            sol.clear_disturbance()
            sol.engine.close()
    base = float(np.median(ms["constant_table"]))
    for name, v in ms.items():
        v = np.asarray(v)
        row = {"B": B, "T": T, "case": name, "ms_per_tick_median": round(float(np.median(v)), 4), "spread": round(float(v.max() - v.min()), 4),
               "over_constant_table": round(float(np.median(v)) / base, 4), "extra_us_per_tick": round(1e3 * (float(np.median(v)) - base), 2),
               "M_robot_ticks_per_s": round(B / float(np.median(v)) / 1e3, 3), **note[name]}
        print(json.dumps(row), flush=True)
        lines.append(f"B = {B:6d}  {name:18s} {row['ms_per_tick_median']:8.4f} [{row['spread']:.4f}] ms/tick, x{row['over_constant_table']:.3f} of the "
                     f"constant table ({row['extra_us_per_tick']:+.2f} us/tick), {row['M_robot_ticks_per_s']:.3f} M robot-ticks/s, all ticks solved "
                     f"{row['all_ticks_solved']:.4f}")

with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
