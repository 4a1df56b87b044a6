"""Developer tool: what the swing legs inside the roll-out cost (include/mpcqp_sim.h, mpcqp_rollout_legs) against the roll-out on the
same gait clock without them (mpcqp_rollout_phase): the named trot (period 10) at v_ref = 0.18 m/s, B = 4096 and 65 536 robots x
T = 50 ticks, f32 buffers, warm-started, heterogeneous bodies and pushes.  Three cases per size, each timed with
mpcqp_last_kernel_ms (device events around all T ticks):

    phase_trot     rollout_phase: the yardstick, three launches per tick
    legs_rule      rollout_legs, land = rule: the same solves, bit for bit (tests/test_gpu_rollout_legs.py), so the difference is the
                   legs step and the landing launch alone
    legs_actual    rollout_legs, land = actual: the feet land where the legs put them, so other QPs from the first landing on

One warm-up round, then REPS rounds that alternate the cases; prints the median, the best and the spread (max - min) over the rounds
in ms per tick.  `--yardstick-lib PATH` adds phase_trot through another build of libmpcqp.so (the parent commit's), loaded next to
this one: the yardstick must not have moved.  `--legs-only` runs legs_rule alone: under `rocprofv3 --kernel-trace --stats` (a run of its
own, one `--size`) that gives the five kernels of a tick by name.
usage: rollout_legs_rate.py [--size B] [--legs-only] [--yardstick-lib PATH]"""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import gaits

T, REPS, B0, STEP_HEIGHT = 50, 5, 64, 0.06
SIZES = (int(sys.argv[sys.argv.index("--size") + 1]),) if "--size" in sys.argv else (4096, 65536)
LEGS_ONLY = "--legs-only" in sys.argv
OTHER = sys.argv[sys.argv.index("--yardstick-lib") + 1] if "--yardstick-lib" in sys.argv else None


def solver(lib=None):
    """A warm-started f32 engine on this build, or on the library `lib`."""
    return mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed", warm_start=True, warm_shift=True, library=lib)


def tiled(a, B, dt):
    return torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * (B // B0), axis=0)), dtype=dt).cuda().contiguous()


trot = gaits.make_phase_batch(B0, "trot", 10, seed=9)
mpcqp.product_library()
other = mpcqp.Library(OTHER, partial=True) if OTHER else None   # (an older build lacks the newest calls of a header)

for B in SIZES:
    rows = mpcqp.synth.make_plant_rows(B, seed=1, push_start=(10, 30))

    def operands(sol):
        d, pb = sol.tdtype, trot
        return [tiled(pb["x"], B, d), tiled(pb["ref"], B, d), tiled(pb["feet"], B, d), tiled(pb["gait"], B, torch.int32), tiled(pb["stand"], B, d),
                tiled(pb["gain"], B, d), tiled(pb["tick"], B, torch.int32), tiled(pb["mu"], B, d)]

    def run_phase(sol):
        return sol.rollout_phase(*operands(sol), T, body=sol.rows[0], push=sol.rows[1], push_ticks=sol.rows[2])

    def run_legs(sol, land):
        a = operands(sol)
        legs = torch.zeros((B, 4, 7), dtype=torch.float64, device="cuda")
        hh = torch.full((B,), STEP_HEIGHT, dtype=sol.tdtype, device="cuda")
        return sol.rollout_legs(*a[:3], legs, *a[3:], T, hh, land, body=sol.rows[0], push=sol.rows[1], push_ticks=sol.rows[2])

    cases = {"phase_trot": (None, run_phase), "legs_rule": (None, lambda s: run_legs(s, "rule")), "legs_actual": (None, lambda s: run_legs(s, "actual"))}
    if LEGS_ONLY:
        cases = {"legs_rule": cases["legs_rule"]}
    elif other:
        cases["yardstick_phase_trot"] = (other, run_phase)
    ms = {k: [] for k in cases}
    solved, miss = {}, {}
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
            if "miss" in out:
                m = out["miss"]
                miss[name] = round(float(m[m > 0].mean()) * 1e3, 3) if bool((m > 0).any()) else 0.0
            sol.engine.close()
    for name, v in ms.items():
        v = np.asarray(v)
        row = {"B": B, "T": T, "case": name, "ms_per_tick_median": round(float(np.median(v)), 4), "best": round(float(v.min()), 4),
               "spread": round(float(v.max() - v.min()), 4), "M_robot_ticks_per_s": round(B / float(np.median(v)) / 1e3, 3),
               "all_ticks_solved": solved[name]}
        if name in miss:
            row["mean_landing_miss_mm"] = miss[name]
        print(json.dumps(row), flush=True)
