"""Developer tool: what a disturbance table costs inside the roll-out (include/mpcqp_disturb.h) against the same rollout_phase call
without one in the same run on the same batch: the named trot (period 10) at v_ref = 0.18 m/s, B = 4096 and 65 536 robots x T = 50
ticks, f32 buffers, warm-started, heterogeneous bodies, a constant push of 5 to 15 N and up to 1 N m on half of the robots, all logs
on.  Three cases per size, each timed with mpcqp_last_kernel_ms (device events around all T ticks):

    plain        rollout_phase without a table: the yardstick, three launches per tick
    zero_table   with a table of zero rows: the same QPs bit for bit (tests/test_gpu_disturbance.py), five launches per tick, so the
                 difference is what the two extra launches -- the shift in front of the solve, the add-back behind it -- cost
    told         with the plant's own push rows as the table: the MPC knows the push, so other QPs

and disturbance_track over the T = 50 rows of the plain case's logs, timed with device events around the one launch.
One warm-up round, then REPS rounds that alternate the cases; prints the median and, in brackets, the spread (max - min) over the
rounds in ms per tick, and writes the lines to profiles/r29_disturbance.txt (or --out PATH).  A measurement: nothing is asserted.
--library PATH measures another build of the product library (`make -C csrc dist_elem`: the lane-per-element form of the two kernels).
usage: disturbance_rate.py [--size B] [--out PATH] [--library PATH]"""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import disturbance, gaits

T, REPS, B0 = 50, 5, 64
SIZES = (int(sys.argv[sys.argv.index("--size") + 1]),) if "--size" in sys.argv else (65536, 4096)
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r29_disturbance.txt")


def tiled(a, B, dt):
    return torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * (B // B0), axis=0)), dtype=dt).cuda().contiguous()


trot = gaits.make_phase_batch(B0, "trot", 10, seed=9)
LIB = mpcqp.Library(sys.argv[sys.argv.index("--library") + 1]) if "--library" in sys.argv else mpcqp.product_library()
lines = ["rollout_phase with a disturbance table against the same call without one, ms per tick: median [spread = max - min over %d rounds]; "
         "tools/disturbance_rate.py" % REPS + (", library " + os.path.basename(LIB.path) if "--library" in sys.argv else "")]

for B in SIZES:
    rows = mpcqp.synth.make_plant_rows(B, seed=1, push_force=(5.0, 15.0), push_torque=(0.0, 1.0), push_start=(0, 0), push_len=(T, T))
    push64 = np.ascontiguousarray(rows["push"], dtype=np.float64)
    tables = {"plain": None, "zero_table": disturbance.wrench_rows(B), "told": push64}
    ms = {k: [] for k in tables}
    note, track_ms = {}, []
    for rep in range(REPS + 1):
        for name, table in tables.items():
            # a fresh handle per run: every run starts cold and warms up over its own ticks
            sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed", warm_start=True, warm_shift=True, library=LIB)
            sol.engine.reserve(B)
            d, pb = sol.tdtype, trot
            if table is not None:
                sol.set_disturbance(table)
            out = sol.rollout_phase(tiled(pb["x"], B, d), tiled(pb["ref"], B, d), tiled(pb["feet"], B, d), tiled(pb["gait"], B, torch.int32),
                                    tiled(pb["stand"], B, d), tiled(pb["gain"], B, d), tiled(pb["tick"], B, torch.int32), tiled(pb["mu"], B, d), T,
                                    body=torch.as_tensor(rows["body"], dtype=d).cuda(), push=torch.as_tensor(rows["push"], dtype=d).cuda(),
                                    push_ticks=torch.as_tensor(rows["push_ticks"]).cuda())
            torch.cuda.synchronize()
            if rep > 0:                            # (round 0 is the warm-up)
                ms[name].append(sol.last_kernel_ms() / T)
            note[name] = {"all_ticks_solved": float((out["solved"].cpu().numpy() == T).mean())}
            if name == "plain":                    # the observer over this run's logs: one launch between two device events
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                state = torch.zeros((B, disturbance.STATE), dtype=torch.float64, device="cuda")
                ev0.record()
                tr = sol.disturbance_track(out, state=state)
                ev1.record()
                torch.cuda.synchronize()
                if rep > 0:
                    track_ms.append(ev0.elapsed_time(ev1))
                del tr
            del out
            sol.engine.close()
    for name, v in ms.items():
        v = np.asarray(v)
        base = float(np.median(ms["plain"]))
        row = {"B": B, "T": T, "case": name, "ms_per_tick_median": round(float(np.median(v)), 4), "spread": round(float(v.max() - v.min()), 4),
               "over_plain": round(float(np.median(v)) / base, 4), "extra_us_per_tick": round(1e3 * (float(np.median(v)) - base), 2),
               "M_robot_ticks_per_s": round(B / float(np.median(v)) / 1e3, 3), **note[name]}
        print(json.dumps(row), flush=True)
        lines.append(f"B = {B:6d}  {name:11s} {row['ms_per_tick_median']:8.4f} [{row['spread']:.4f}] ms/tick, x{row['over_plain']:.3f} of the call without "
                     f"a table ({row['extra_us_per_tick']:+.2f} us/tick), {row['M_robot_ticks_per_s']:.3f} M robot-ticks/s, all ticks solved "
                     f"{row['all_ticks_solved']:.4f}")
    v = np.asarray(track_ms)
    row = {"B": B, "T": T, "case": "disturbance_track", "ms_median": round(float(np.median(v)), 4), "spread": round(float(v.max() - v.min()), 4),
           "M_rows_per_s": round(B * T / float(np.median(v)) / 1e3, 2)}
    print(json.dumps(row), flush=True)
    lines.append(f"B = {B:6d}  disturbance_track over {T} rows {row['ms_median']:8.4f} [{row['spread']:.4f}] ms, {row['M_rows_per_s']:.2f} M rows/s")

with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
