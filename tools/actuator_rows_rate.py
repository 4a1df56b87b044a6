"""Developer tool: what an actuator table costs (include/mpcqp_actuators.h, mpcqp_set_actuators) inside mpcqp_rollout_drive and in
mpcqp_stance_drive / mpcqp_swing_track alone, in the same run on the batch of tools/rollout_drive_rate.py: the named trot (period 10) at
v_ref = 0.18 m/s, B = 4096 and 65 536 robots x T = 50 ticks, f32 buffers, warm-started, heterogeneous bodies and pushes, land = rule,
drive = limited.  Three cases per size, each timed with mpcqp_last_kernel_ms (device events around all T ticks):

    no_table        the inertia row with tau_max x 0.5: the drive_half case of tools/rollout_drive_rate.py, the parent's kernels
    flat            the same clamp through a table, actuators.actuator_rows(B, scale=0.5): the ACT instantiations, the same closed loop
    curve           the rows (1, 0.05, 0.25) on every robot: other applied torques, other QPs from the first clamped row on

One warm-up round, then REPS rounds that alternate the cases; prints the median, the best and the spread (max - min) over the rounds
in ms per tick and how many swing / stance leg-rows were clamped.  Then, on the logs of the last curve roll-out, stance_drive on the
B T logged rows and swing_track on the B robots, each with and without the table (torch events, median of REPS after a warm-up).
usage: actuator_rows_rate.py [--size B]"""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import actuators, gaits, lite3_model

T, REPS, B0, STEP_HEIGHT = 50, 5, 64, 0.06
SIZES = (int(sys.argv[sys.argv.index("--size") + 1]),) if "--size" in sys.argv else (4096, 65536)
CURVE = (1.0, 0.05, 0.25)


def tiled(a, B, dt):
    return torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * (B // B0), axis=0)), dtype=dt).cuda().contiguous()


def timed(call):
    """Median and spread in ms of REPS runs of call() after one warm-up, by events on the current stream."""
    ms = []
    for rep in range(REPS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if rep > 0:
            ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 4), round(float(max(ms) - min(ms)), 4)


trot = gaits.make_phase_batch(B0, "trot", 10, seed=9)
half = lite3_model.leg_inertia()
half["tau_max"] = half["tau_max"] * 0.5
mpcqp.product_library()

for B in SIZES:
    rows = mpcqp.synth.make_plant_rows(B, seed=1, push_start=(10, 30))
    tables = {"no_table": None, "flat": actuators.actuator_rows(B, None, 0.5), "curve": actuators.actuator_rows(B, None, *CURVE)}

    def run(sol, inertia):
        d, pb = sol.tdtype, trot
        a = [tiled(pb["x"], B, d), tiled(pb["ref"], B, d), tiled(pb["feet"], B, d), torch.zeros((B, 4, 7), dtype=torch.float64, device="cuda"),
             tiled(pb["gait"], B, torch.int32), tiled(pb["stand"], B, d), tiled(pb["gain"], B, d), tiled(pb["tick"], B, torch.int32),
             tiled(pb["mu"], B, d), T, torch.full((B,), STEP_HEIGHT, dtype=d, device="cuda"), "rule"]
        return sol.rollout_drive(*a, "limited", None, body=sol.rows[0], push=sol.rows[1], push_ticks=sol.rows[2], inertia=inertia)

    ms = {k: [] for k in tables}
    note = {}
    for rep in range(REPS + 1):
        for name, table in tables.items():
            # a fresh handle per run: every run starts cold and warms up over its own ticks
            sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed", warm_start=True, warm_shift=True)
            sol.engine.reserve(B)
            sol.rows = (torch.as_tensor(rows["body"], dtype=sol.tdtype).cuda(), torch.as_tensor(rows["push"], dtype=sol.tdtype).cuda(),
                        torch.as_tensor(rows["push_ticks"]).cuda())
            if table is not None:
                sol.set_actuators(table)
            out = run(sol, half if name == "no_table" else None)
            torch.cuda.synchronize()
            if rep > 0:                            # (round 0 is the warm-up)
                ms[name].append(sol.last_kernel_ms() / T)
            live, st = out["flag"] != 0xff, out["contact_log"] != 0
            cl = ((out["flag"] & 2) != 0) & live
            note[name] = {"all_ticks_solved": float((out["solved"].cpu().numpy() == T).mean()), "clamped_swing_rows": int((cl & ~st).sum()),
                          "clamped_stance_rows": int((cl & st).sum())}
            if name == "curve" and rep == REPS:
                logs = out
            else:
                del out
                sol.engine.close()
    for name, v in ms.items():
        v = np.asarray(v)
        print(json.dumps({"B": B, "T": T, "case": name, "ms_per_tick_median": round(float(np.median(v)), 4), "best": round(float(v.min()), 4),
                          "spread": round(float(v.max() - v.min()), 4), "M_robot_ticks_per_s": round(B / float(np.median(v)) / 1e3, 3),
                          **note[name]}), flush=True)
    # the two row calls alone, on the logs of the last curve roll-out (`sol` is its handle, the table still set)
    n = B * T
    flat = lambda k, *s: logs[k].reshape(n, *s)
    drive = lambda: sol.stance_drive(flat("actual", 12), flat("cmd", 12), flat("feet_log", 4, 3), flat("contact_log", 4), None)
    track = lambda: sol.swing_track(logs, logs["swing"], body=sol.rows[0])
    res = {}
    res["swing_track_table"] = timed(track)
    sol.set_actuators(actuators.tile(tables["curve"], T))
    res["stance_drive_table"] = timed(drive)
    sol.clear_actuators()
    res["swing_track"], res["stance_drive"] = timed(track), timed(drive)
    for name, (med, spread) in res.items():
        rows_n = n if name.startswith("stance") else B
        print(json.dumps({"B": B, "T": T, "call": name, "rows": rows_n, "ms_median": med, "spread": spread}), flush=True)
    del logs
    sol.engine.close()
