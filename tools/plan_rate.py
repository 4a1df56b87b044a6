"""Developer tool: rate of the device footstep planner and swing-trajectory generator (include/mpcqp_plan.h) next to the host loop.
B = 4096 and 65 536 robots from synth.make_plan_inputs (every total_steps forced to S, so all rows are planned), S = 50 plan steps,
K = 60 ticks of swing trajectories, fp32 and fp64 I/O.  Times with HIP events around each call (both planner launches; the swing
launch), best of 20 after 3 warm-ups, and reports the effective store bandwidth = bytes of output written / time (the planner's
fp64 workspace, B x S x 40 B written and read back, is not counted).  The host loop is footstep_planner.plan_tables on 256 robots.
usage: plan_rate.py [--quick]"""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp.footstep_planner import plan_tables

S, K = 50, 60
SIZES = (4096,) if "--quick" in sys.argv else (4096, 65536)


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    best = float("inf")
    for _ in range(reps):
        e0.record(); fn(); e1.record(); e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


rows = []
for io in ("f32", "f64"):
    el = 4 if io == "f32" else 8
    sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed")
    for B in SIZES:
        p = mpcqp.synth.make_plan_inputs(B, seed=20250903)
        p["gait"][:, 0] = S
        t = lambda a, dt=sol.tdtype: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()
        feet0, cmd, gait, h = t(p["feet0"]), t(p["cmd"]), t(p["gait"], torch.int32), t(p["step_height"])
        tick = t(np.random.default_rng(1).integers(0, 200, B), torch.int32)
        plan = sol.plan_footsteps(feet0, cmd, gait, S, want_hip=True)
        ms_plan = timed(lambda: sol.plan_footsteps(feet0, cmd, gait, S, want_hip=True))
        ms_swing = timed(lambda: sol.swing_trajectories(plan, tick, K, h))
        by_plan = B * S * (12 * el + 4 + el + 3 * el) + B * 16        # pos, feet_id, ang, hip rows + meta
        by_swing = B * K * 4 * (18 + 3) * el                           # traj + feet_des
        r = {"io": io, "B": B, "S": S, "K": K, "plan_ms": round(ms_plan, 4), "plan_MB": round(by_plan / 1e6, 1),
             "plan_TBps": round(by_plan / ms_plan / 1e9, 3), "plan_M_robot_steps_per_s": round(B * S / ms_plan / 1e3, 1),
             "swing_ms": round(ms_swing, 4), "swing_MB": round(by_swing / 1e6, 1), "swing_TBps": round(by_swing / ms_swing / 1e9, 3),
             "swing_M_leg_ticks_per_s": round(B * K * 4 / ms_swing / 1e3, 1)}
        rows.append(r)
        print(json.dumps(r), flush=True)

# the host loop it replaces: one FootstepPlanner per robot (synth.make_rollout_batch's way of filling the tables)
p = mpcqp.synth.make_plan_inputs(256, seed=20250903)
p["gait"][:, 0] = S
t0 = time.perf_counter()
plan_tables(p["feet0"], p["cmd"], p["gait"], S, 0.03)
host_ms = (time.perf_counter() - t0) * 1e3 / 256
print(json.dumps({"host_plan_tables_ms_per_robot": round(host_ms, 3), "host_s_at_B65536": round(host_ms * 65536 / 1e3, 1)}), flush=True)
