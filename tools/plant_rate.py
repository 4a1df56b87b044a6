"""Developer tool: the device roll-out on the rigid-body plant (include/mpcqp_sim.h, mpcqp_rollout_plant) against the kinematic
roll-out (mpcqp_rollout), B = 4096 and 65 536 robots x T = 100 ticks, f32 buffers, warm-started (engine-side shift) and cold.
Times each call with a host clock around a device synchronise (best of 3 after a warm-up) and prints robot-ticks/s, plus the plant
kernel alone (mpcqp_plant_step, 10 substeps) timed with HIP events.  The plant's share of a tick comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/plant_rate.py --plant-only` run (stable kernel names: mpcqp_rollout_advance_kernel<T, PlantIn<T>>).
usage: plant_rate.py [--quick] [--plant-only]"""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp

T = 100
SIZES = (4096,) if "--quick" in sys.argv else (4096, 65536)
PLANT_ONLY = "--plant-only" in sys.argv
B0 = 64
rb = mpcqp.synth.make_rollout_batch(B0, seed=9)


def inputs(B, sol):
    rep = B // B0
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * rep, axis=0)), dtype=dt).cuda().contiguous()
    d = sol.tdtype
    return (t(rb["x"], d), t(rb["ref"], d), t(rb["plan_pos"], d), t(rb["plan_feet_id"], torch.uint8), t(rb["plan_meta"], torch.int32),
            t(rb["tick"], torch.int32), t(rb["mu"], d))


for B in SIZES:
    rows = mpcqp.synth.make_plant_rows(B, seed=1, push_start=(20, 60))
    for warm in (True, False):
        res = {"B": B, "T": T, "warm": warm}
        for kind in (("plant",) if PLANT_ONLY else ("kinematic", "plant")):
            sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed", warm_start=warm, warm_shift=warm)
            body = torch.as_tensor(rows["body"], dtype=sol.tdtype).cuda()
            push = torch.as_tensor(rows["push"], dtype=sol.tdtype).cuda()
            pt = torch.as_tensor(rows["push_ticks"]).cuda()
            ms = []
            for rep in range(1 if PLANT_ONLY else 4):
                x, rf, pos, fid, meta, tick, mu = inputs(B, sol)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if kind == "plant":
                    out = sol.rollout_plant(x, rf, pos, fid, meta, tick, mu, T, body=body, push=push, push_ticks=pt, substeps=10)
                else:
                    out = sol.rollout(x, rf, pos, fid, meta, tick, mu, T)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            best = min(ms[1:]) if len(ms) > 1 else ms[0]
            res[kind + "_ms_per_tick"] = round(best / T, 4)
            res[kind + "_M_robot_ticks_per_s"] = round(B * T / best / 1e3, 3)
            res[kind + "_all_ticks_solved"] = float((out["solved"].cpu().numpy() == T).mean())
        print(json.dumps(res), flush=True)
    # the plant kernel alone
    sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed")
    x = inputs(B, sol)[0]
    f = torch.tile(torch.tensor([0.0, 0.0, 21.8], dtype=sol.tdtype, device="cuda"), (B, 4)).contiguous()
    feet = torch.as_tensor(np.concatenate([rb["plan_pos"][:, 0]] * (B // B0)), dtype=sol.tdtype).cuda().contiguous()
    ct = torch.ones((B, 4), dtype=torch.uint8, device="cuda")
    body = torch.as_tensor(rows["body"], dtype=sol.tdtype).cuda()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        sol.plant_step(x, f, feet, ct, body, None, 10)
    best = float("inf")
    for _ in range(20):
        e0.record(); sol.plant_step(x, f, feet, ct, body, None, 10); e1.record(); e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    print(json.dumps({"B": B, "plant_step_ms": round(best, 4), "plant_step_G_robot_ticks_per_s": round(B / best / 1e6, 3)}), flush=True)
