"""Developer tool: what the trust gate costs inside the roll-out (include/mpcqp_gate.h, mpcqp_rollout_observe_gated) against
mpcqp_rollout_observe in the same run on the same batch, with the set-up of tools/rollout_observe_rate.py: the named trot (period 10)
at v_ref = 0.18 m/s, B = 4096 and 65 536 robots x T = 50 ticks, f32 buffers, warm-started, heterogeneous bodies and pushes, land =
rule, ground 0.3, the foot mass lite3_model.foot_mass(), IMU noise and bias given, all logs on, the default thresholds.  Four cases per
size, each timed with mpcqp_last_kernel_ms (device events around all T ticks):

    observe_truth     rollout_observe, feed = truth: the yardstick, nine launches per tick
    gated_truth       rollout_observe(gate={}), feed = truth: the same closed loop bit for bit (tests/test_gpu_gate.py), the same nine
                      launches, so the difference is the gated update kernel's own cost and the trust log
    observe_estimate  rollout_observe, feed = estimate
    gated_estimate    rollout_observe(gate={}), feed = estimate: the MPC reads another estimate, so other QPs from the first sliding foot on

One warm-up round, then REPS rounds that alternate the cases; prints the median and, in brackets, the spread (max - min) over the
rounds in ms per tick, and writes the lines to profiles/r26_gate.txt (or --out PATH).  A measurement: nothing is asserted.
usage: rollout_gate_rate.py [--size B] [--out PATH]"""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import gaits, lite3_model

T, REPS, B0, STEP_HEIGHT, GROUND = 50, 5, 64, 0.06, 0.3
SIZES = (int(sys.argv[sys.argv.index("--size") + 1]),) if "--size" in sys.argv else (65536, 4096)
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r26_gate.txt")


def tiled(a, B, dt):
    return torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * (B // B0), axis=0)), dtype=dt).cuda().contiguous()


trot = gaits.make_phase_batch(B0, "trot", 10, seed=9)
FOOT_MASS = lite3_model.foot_mass()
mpcqp.product_library()
lines = ["rollout_observe(gate={}) against rollout_observe, ms per tick: median [spread = max - min over %d rounds]; tools/rollout_gate_rate.py" % REPS]

for B in SIZES:
    rows = mpcqp.synth.make_plant_rows(B, seed=1, push_start=(10, 30))

    def run(sol, feed, gate):
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
        return sol.rollout_observe(*a, torch.zeros((B, 131), dtype=torch.float64, device="cuda"), feed, bias=bias, noise=noise, land="rule",
                                   drive="limited", gate=gate, **kw)

    cases = {"observe_truth": ("truth", None), "gated_truth": ("truth", {}), "observe_estimate": ("estimate", None),
             "gated_estimate": ("estimate", {})}
    ms = {k: [] for k in cases}
    note = {}
    for rep in range(REPS + 1):
        for name, (feed, gate) in cases.items():
            # a fresh handle per run: every run starts cold and warms up over its own ticks
            sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed", warm_start=True, warm_shift=True)
            sol.engine.reserve(B)
            sol.rows = (torch.as_tensor(rows["body"], dtype=sol.tdtype).cuda(), torch.as_tensor(rows["push"], dtype=sol.tdtype).cuda(),
                        torch.as_tensor(rows["push_ticks"]).cuda())
            out = run(sol, feed, gate)
            torch.cuda.synchronize()
            if rep > 0:                            # (round 0 is the warm-up)
                ms[name].append(sol.last_kernel_ms() / T)
            note[name] = {"all_ticks_solved": float((out["solved"].cpu().numpy() == T).mean())}
            if gate is not None:
                stance = out["contact_log"] != 0
                note[name]["stance_rows_gated"] = float((out["trust"][stance] < 1).float().mean())
            del out
            sol.engine.close()
    for name, v in ms.items():
        v = np.asarray(v)
        base = np.median(ms["observe_" + name.split("_")[1]])
        row = {"B": B, "T": T, "case": name, "ms_per_tick_median": round(float(np.median(v)), 4), "spread": round(float(v.max() - v.min()), 4),
               "over_ungated": round(float(np.median(v) / base), 4), "M_robot_ticks_per_s": round(B / float(np.median(v)) / 1e3, 3), **note[name]}
        print(json.dumps(row), flush=True)
        lines.append(f"B = {B:6d}  {name:17s} {row['ms_per_tick_median']:8.4f} [{row['spread']:.4f}] ms/tick, x{row['over_ungated']:.3f} of the ungated "
                     f"call, {row['M_robot_ticks_per_s']:.3f} M robot-ticks/s, all ticks solved {row['all_ticks_solved']:.4f}"
                     + (f", stance leg-rows with w < 1: {row['stance_rows_gated']:.4f}" if "stance_rows_gated" in row else ""))

with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
