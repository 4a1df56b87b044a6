"""Developer tool: what the velocity-aided attitude rule costs (include/mpcqp_attitude.h, mpcqp_rollout_observe_aided and
mpcqp_estimate_track_aided) against mpcqp_rollout_observe and mpcqp_estimate_track in the same run on the same batch, with the set-up
of tools/rollout_gate_rate.py: the named trot (period 10) at v_ref = 0.18 m/s, B = 4096 and 65 536 robots x T = 50 ticks, f32 buffers,
warm-started, heterogeneous bodies and pushes, land = rule, ground 0.3, the foot mass lite3_model.foot_mass(), IMU noise and bias
given, all logs on, the default gains.  Four roll-out cases per size, each timed with mpcqp_last_kernel_ms (device events around all T
ticks):

    observe_truth     rollout_observe, feed = truth: the yardstick, nine launches per tick
    aided_truth       rollout_observe(attitude={}), feed = truth: the same closed loop bit for bit (tests/test_gpu_attitude.py), the same
                      nine launches, so the difference is the two aided kernels' own cost, att_state's 8 doubles and the bias log
    observe_estimate  rollout_observe, feed = estimate
    aided_estimate    rollout_observe(attitude={}), feed = estimate: the MPC reads another estimate, so other QPs

and two log passes over the sensor logs of the size's observe_truth run, timed with device events around ESTIMATE_CALLS calls:

    track             estimate_track
    track_aided       estimate_track(attitude={})

One warm-up round, then REPS rounds that alternate the cases; prints the median and, in brackets, the spread (max - min) over the
rounds, and writes the lines to profiles/r28_attitude.txt (or --out PATH).  A measurement: nothing is asserted.
usage: rollout_attitude_rate.py [--size B] [--out PATH]"""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import gaits, lite3_model

T, REPS, B0, STEP_HEIGHT, GROUND, ESTIMATE_CALLS = 50, 5, 64, 0.06, 0.3, 10
SIZES = (int(sys.argv[sys.argv.index("--size") + 1]),) if "--size" in sys.argv else (65536, 4096)
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r28_attitude.txt")


def tiled(a, B, dt):
    return torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * (B // B0), axis=0)), dtype=dt).cuda().contiguous()


trot = gaits.make_phase_batch(B0, "trot", 10, seed=9)
FOOT_MASS = lite3_model.foot_mass()
mpcqp.product_library()
lines = ["rollout_observe(attitude={}) against rollout_observe, ms per tick, and estimate_track(attitude={}) against estimate_track, ms per "
         "call of %d rows: median [spread = max - min over %d rounds]; tools/rollout_attitude_rate.py" % (T, REPS)]

for B in SIZES:
    rows = mpcqp.synth.make_plant_rows(B, seed=1, push_start=(10, 30))

    def run(sol, feed, attitude):
        d, pb = sol.tdtype, trot
        gen = torch.Generator(device="cuda").manual_seed(25)           # the same draws for every case
        a = [tiled(pb["x"], B, d), tiled(pb["ref"], B, d), tiled(pb["feet"], B, d), torch.zeros((B, 4, 7), dtype=torch.float64, device="cuda"),
             tiled(pb["gait"], B, torch.int32), tiled(pb["stand"], B, d), tiled(pb["gain"], B, d), tiled(pb["tick"], B, torch.int32),
             tiled(pb["mu"], B, d), T, torch.full((B,), STEP_HEIGHT, dtype=d, device="cuda"), torch.full((B,), GROUND, dtype=d, device="cuda"),
             torch.full((B,), FOOT_MASS, dtype=d, device="cuda"), torch.zeros((B, 4, 2), dtype=torch.float64, device="cuda")]
        kw = {"body": sol.rows[0], "push": sol.rows[1], "push_ticks": sol.rows[2]}
        scale = torch.tensor([0.01] * 3 + [0.05] * 3, dtype=d, device="cuda")
        noise = torch.randn((B, T, 6), dtype=d, device="cuda", generator=gen) * scale
        bias = torch.randn((B, 6), dtype=d, device="cuda", generator=gen) * scale * 0.5
        if attitude is not None:
            kw.update(attitude=attitude, att_state=torch.zeros((B, 8), dtype=torch.float64, device="cuda"))
        return sol.rollout_observe(*a, torch.zeros((B, 131), dtype=torch.float64, device="cuda"), feed, bias=bias, noise=noise, land="rule",
                                   drive="limited", **kw)

    def track_ms(sol, logs, attitude):
        init = logs["actual"][:, 0].contiguous()
        kw = {} if attitude is None else {"attitude": attitude}
        call = lambda: sol.estimate_track(logs["imu"], logs["q_enc"], logs["qd_enc"], logs["contact_log"], init, **kw)
        call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ESTIMATE_CALLS):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / ESTIMATE_CALLS

    cases = {"observe_truth": ("truth", None), "aided_truth": ("truth", {}), "observe_estimate": ("estimate", None),
             "aided_estimate": ("estimate", {})}
    ms = {k: [] for k in list(cases) + ["track", "track_aided"]}
    note = {}
    for rep in range(REPS + 1):
        for name, (feed, attitude) in cases.items():
            # a fresh handle per run: every run starts cold and warms up over its own ticks
            sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed", warm_start=True, warm_shift=True)
            sol.engine.reserve(B)
            sol.rows = (torch.as_tensor(rows["body"], dtype=sol.tdtype).cuda(), torch.as_tensor(rows["push"], dtype=sol.tdtype).cuda(),
                        torch.as_tensor(rows["push_ticks"]).cuda())
            out = run(sol, feed, attitude)
            torch.cuda.synchronize()
            if rep > 0:                            # (round 0 is the warm-up)
                ms[name].append(sol.last_kernel_ms() / T)
            note[name] = {"all_ticks_solved": float((out["solved"].cpu().numpy() == T).mean())}
            if name == "observe_truth":            # the two log passes, on this run's sensor logs, alternating
                for k, att in (("track", None), ("track_aided", {})):
                    v = track_ms(sol, out, att)
                    if rep > 0:
                        ms[k].append(v)
            del out
            sol.engine.close()
    for name, v in ms.items():
        v = np.asarray(v)
        if name.startswith("track"):
            base = np.median(ms["track"])
            row = {"B": B, "T": T, "case": name, "ms_per_call_median": round(float(np.median(v)), 4), "spread": round(float(v.max() - v.min()), 4),
                   "over_unaided": round(float(np.median(v) / base), 4), "M_robot_rows_per_s": round(B * T / float(np.median(v)) / 1e3, 3)}
            print(json.dumps(row), flush=True)
            lines.append(f"B = {B:6d}  {name:17s} {row['ms_per_call_median']:8.4f} [{row['spread']:.4f}] ms/call, x{row['over_unaided']:.3f} of the unaided "
                         f"call, {row['M_robot_rows_per_s']:.3f} M robot-rows/s")
            continue
        base = np.median(ms["observe_" + name.split("_")[1]])
        row = {"B": B, "T": T, "case": name, "ms_per_tick_median": round(float(np.median(v)), 4), "spread": round(float(v.max() - v.min()), 4),
               "over_unaided": round(float(np.median(v) / base), 4), "M_robot_ticks_per_s": round(B / float(np.median(v)) / 1e3, 3), **note[name]}
        print(json.dumps(row), flush=True)
        lines.append(f"B = {B:6d}  {name:17s} {row['ms_per_tick_median']:8.4f} [{row['spread']:.4f}] ms/tick, x{row['over_unaided']:.3f} of the unaided "
                     f"call, {row['M_robot_ticks_per_s']:.3f} M robot-ticks/s, all ticks solved {row['all_ticks_solved']:.4f}")

with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
