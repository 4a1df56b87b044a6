"""Developer tool: what the roll-out on a gait clock costs (include/mpcqp_sim.h, mpcqp_rollout_phase) against the roll-out on a
plan table (mpcqp_rollout_plant), B = 4096 and 65 536 robots x T = 50 ticks, f32 buffers, warm-started, heterogeneous bodies and
pushes.  Four cases per size, each timed with mpcqp_last_kernel_ms (device events around all T ticks):

    plant_stand   rollout_plant on a one-step all-stance plan, v_ref = 0: the yardstick
    phase_stand   rollout_phase on the stand gait (stance = P) on the same feet: the same solves, bit for bit
                  (tests/test_gpu_gaits.py), so the difference is the expand and advance kernels alone
    phase_trot    rollout_phase on the named trot (period 10) at v_ref = 0.18 m/s, landing on reactive footholds
    plant_trot    rollout_plant on the footstep planner's trot (ss 4, ds 2) at the same v_ref, for scale: another contact schedule,
                  so other QPs

One warm-up round, then REPS rounds that alternate the cases; prints the median, the best and the spread (max - min) over the rounds
in ms per tick.  `--yardstick-lib PATH` adds plant_stand / plant_trot through another build of libmpcqp.so (the parent commit's),
loaded next to this one.  `--stand-only` runs the two stand cases alone: under `rocprofv3 --kernel-trace --stats` (a run of its own,
one `--size`) that gives the expand and advance kernels of either path by name.
usage: phase_rollout_rate.py [--size B] [--stand-only] [--yardstick-lib PATH]"""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import gaits

T, REPS, B0 = 50, 5, 64
SIZES = (int(sys.argv[sys.argv.index("--size") + 1]),) if "--size" in sys.argv else (4096, 65536)
STAND_ONLY = "--stand-only" in sys.argv
OTHER = sys.argv[sys.argv.index("--yardstick-lib") + 1] if "--yardstick-lib" in sys.argv else None


def solver(lib=None):
    """A warm-started f32 engine on this build, or on the library `lib`."""
    return mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed", warm_start=True, warm_shift=True, library=lib)


def tiled(a, B, dt):
    return torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * (B // B0), axis=0)), dtype=dt).cuda().contiguous()


stand = gaits.make_phase_batch(B0, "stand", 10, seed=9, v_ref=(0.0, 0.0, 0.0))
trot = gaits.make_phase_batch(B0, "trot", 10, seed=9)
plan = mpcqp.synth.make_rollout_batch(B0, seed=9, gait_names=("trot",))
mpcqp.product_library()
other = mpcqp.Library(OTHER, partial=True) if OTHER else None   # (an older build lacks the newest calls of a header)

for B in SIZES:
    rows = mpcqp.synth.make_plant_rows(B, seed=1, push_start=(10, 30))

    def run_phase(sol, pb):
        d = sol.tdtype
        out = sol.rollout_phase(tiled(pb["x"], B, d), tiled(pb["ref"], B, d), tiled(pb["feet"], B, d), tiled(pb["gait"], B, torch.int32),
                                tiled(pb["stand"], B, d), tiled(pb["gain"], B, d), tiled(pb["tick"], B, torch.int32), tiled(pb["mu"], B, d), T,
                                body=sol.rows[0], push=sol.rows[1], push_ticks=sol.rows[2])
        return out

    def run_plant(sol, x, ref, pos, fid, meta, tick, mu):
        d = sol.tdtype
        return sol.rollout_plant(tiled(x, B, d), tiled(ref, B, d), tiled(pos, B, d), tiled(fid, B, torch.uint8), tiled(meta, B, torch.int32),
                                 tiled(tick, B, torch.int32), tiled(mu, B, d), T, body=sol.rows[0], push=sol.rows[1], push_ticks=sol.rows[2])

    one_step = (stand["x"], stand["ref"], stand["feet"][:, None], np.ones((B0, 1, 4), np.uint8), np.tile(np.array([1, 4, 2, 0], np.int32), (B0, 1)),
                stand["tick"], stand["mu"])
    planned = tuple(plan[k] for k in ("x", "ref", "plan_pos", "plan_feet_id", "plan_meta", "tick", "mu"))
    cases = {"plant_stand": (None, lambda s: run_plant(s, *one_step)), "phase_stand": (None, lambda s: run_phase(s, stand)),
             "phase_trot": (None, lambda s: run_phase(s, trot)), "plant_trot": (None, lambda s: run_plant(s, *planned))}
    if STAND_ONLY:
        cases = {k: v for k, v in cases.items() if k.endswith("_stand")}
    elif other:
        cases["yardstick_plant_stand"] = (other, lambda s: run_plant(s, *one_step))
        cases["yardstick_plant_trot"] = (other, lambda s: run_plant(s, *planned))
    ms = {k: [] for k in cases}
    solved = {}
    for rep in range(REPS + 1):
        for name, (lib, run) in cases.items():
            sol = solver(lib)                      # a fresh handle per run: every run starts cold and warms up over its own ticks
            sol.engine.reserve(B)
            sol.rows = (torch.as_tensor(rows["body"], dtype=sol.tdtype).cuda(), torch.as_tensor(rows["push"], dtype=sol.tdtype).cuda(),
                        torch.as_tensor(rows["push_ticks"]).cuda())
            out = run(sol)
            torch.cuda.synchronize()
            if rep > 0:                            # (round 0 is the warm-up)
                ms[name].append(sol.last_kernel_ms() / T)
            solved[name] = float((out["solved"].cpu().numpy() == T).mean())
            sol.engine.close()
    for name, v in ms.items():
        v = np.asarray(v)
        print(json.dumps({"B": B, "T": T, "case": name, "ms_per_tick_median": round(float(np.median(v)), 4), "best": round(float(v.min()), 4),
                          "spread": round(float(v.max() - v.min()), 4), "M_robot_ticks_per_s": round(B / float(np.median(v)) / 1e3, 3),
                          "all_ticks_solved": solved[name]}), flush=True)
