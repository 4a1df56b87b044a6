"""Developer tool: what the slip rule costs inside the roll-out (include/mpcqp_slip.h, mpcqp_rollout_slip) against mpcqp_rollout_drive in
the same run on the same batch: the named trot (period 10) at v_ref = 0.18 m/s, B = 4096 and 65 536 robots x T = 50 ticks, f32 buffers,
warm-started, heterogeneous bodies and pushes, land = rule, the foot mass lite3_model.foot_mass().  Four cases per size, each timed
with mpcqp_last_kernel_ms (device events around all T ticks):

    drive_grip      rollout_drive, drive = limited on ground 1e3: the yardstick, seven launches per tick with the logs
    slip_grip       rollout_slip on ground 1e3: the same closed loop bit for bit (tests/test_gpu_slip.py), so the difference is the
                    rule's own cost -- the substep loop and the foot move in the launch that carries the log step
    drive_ground    rollout_drive on ground 0.3 (the controllers believe 0.5 to 1.0)
    slip_ground     rollout_slip on ground 0.3: the feet move, so other QPs from the first slide on

One warm-up round, then REPS rounds that alternate the cases; prints the median, the best and the spread (max - min) over the rounds
in ms per tick, and how many stance leg-rows the ground limited / slid.
usage: rollout_slip_rate.py [--size B]"""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import gaits, lite3_model

T, REPS, B0, STEP_HEIGHT, GROUND, GRIP = 50, 5, 64, 0.06, 0.3, 1e3
SIZES = (int(sys.argv[sys.argv.index("--size") + 1]),) if "--size" in sys.argv else (4096, 65536)


def tiled(a, B, dt):
    return torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * (B // B0), axis=0)), dtype=dt).cuda().contiguous()


trot = gaits.make_phase_batch(B0, "trot", 10, seed=9)
FOOT_MASS = lite3_model.foot_mass()
mpcqp.product_library()

for B in SIZES:
    rows = mpcqp.synth.make_plant_rows(B, seed=1, push_start=(10, 30))

    def run(sol, slip, ground):
        d, pb = sol.tdtype, trot
        a = [tiled(pb["x"], B, d), tiled(pb["ref"], B, d), tiled(pb["feet"], B, d), torch.zeros((B, 4, 7), dtype=torch.float64, device="cuda"),
             tiled(pb["gait"], B, torch.int32), tiled(pb["stand"], B, d), tiled(pb["gain"], B, d), tiled(pb["tick"], B, torch.int32),
             tiled(pb["mu"], B, d), T, torch.full((B,), STEP_HEIGHT, dtype=d, device="cuda")]
        kw = {"body": sol.rows[0], "push": sol.rows[1], "push_ticks": sol.rows[2]}
        g = torch.full((B,), ground, dtype=d, device="cuda")
        if not slip:
            return sol.rollout_drive(*a, "rule", "limited", g, **kw)
        me = torch.full((B,), FOOT_MASS, dtype=d, device="cuda")
        return sol.rollout_slip(*a, g, me, torch.zeros((B, 4, 2), dtype=torch.float64, device="cuda"), "rule", "limited", **kw)

    cases = {"drive_grip": (False, GRIP), "slip_grip": (True, GRIP), "drive_ground": (False, GROUND), "slip_ground": (True, GROUND)}
    ms = {k: [] for k in cases}
    note = {}
    for rep in range(REPS + 1):
        for name, (slip, ground) in cases.items():
            # a fresh handle per run: every run starts cold and warms up over its own ticks
            sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed", warm_start=True, warm_shift=True)
            sol.engine.reserve(B)
            sol.rows = (torch.as_tensor(rows["body"], dtype=sol.tdtype).cuda(), torch.as_tensor(rows["push"], dtype=sol.tdtype).cuda(),
                        torch.as_tensor(rows["push_ticks"]).cuda())
            out = run(sol, slip, ground)
            torch.cuda.synchronize()
            if rep > 0:                            # (round 0 is the warm-up)
                ms[name].append(sol.last_kernel_ms() / T)
            st = (out["contact_log"] != 0) & (out["flag"] != 0xff)
            note[name] = {"all_ticks_solved": float((out["solved"].cpu().numpy() == T).mean()), "stance_rows": int(st.sum()),
                          "ground_rows": int(((out["flag"] & 32) != 0)[st].sum()), "sliding_rows": int(((out["flag"] & 128) != 0)[st].sum())}
            del out
            sol.engine.close()
    for name, v in ms.items():
        v = np.asarray(v)
        print(json.dumps({"B": B, "T": T, "case": name, "ms_per_tick_median": round(float(np.median(v)), 4), "best": round(float(v.min()), 4),
                          "spread": round(float(v.max() - v.min()), 4), "M_robot_ticks_per_s": round(B / float(np.median(v)) / 1e3, 3),
                          **note[name]}), flush=True)
