"""Developer tool: rate of the swing-foot trajectories of the roll-out on a gait clock (include/mpcqp_plan.h, mpcqp_phase_swing) and of the
joint rates that consume them (include/mpcqp_joints.h, mpcqp_joint_rates).  B = 65 536 robots x T = 50 log rows (13.1 M legs), fp32 and
fp64 I/O; the logs are synthetic and made on the device: random torso states and references, feet under the nominal stance, the
eight named gaits at period 12.  Times one call of each with HIP events, median and best of 20 after 3 warm-ups, and reports the
HBM bytes the call has to move (every log read once, every output written once; the per-robot rows are a thousandth of that) over
that time, against the 8 TB/s roof.
usage: phase_swing_rate.py [--quick]"""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import gaits, synth

B, T = (4096, 50) if "--quick" in sys.argv else (65536, 50)
HBM_TBPS = 8.0


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms))


def report(call, io, by, med, best, **more):
    print(json.dumps({"call": call, "io": io, "B": B, "T": T, "legs": 4 * B * T, "ms_median": round(med, 4), "ms_best": round(best, 4),
                      "MB": round(by / 1e6, 1), "TBps": round(by / med / 1e9, 3), "share_of_8TBps_roof": round(by / med / 1e9 / HBM_TBPS, 3),
                      "G_legs_per_s": round(4 * B * T / med / 1e6, 3), **more}), flush=True)


names = tuple(gaits.GAITS)
rows = B * T
for io in ("f32", "f64"):
    el = 4 if io == "f32" else 8
    sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed")
    dt, dev = sol.tdtype, sol.device
    gen = torch.Generator(device=dev).manual_seed(20251018)
    rnd = lambda shape, sd: torch.randn(shape, generator=gen, device=dev, dtype=torch.float64) * sd
    actual = torch.cat([rnd((B, T, 3), 0.1), rnd((B, T, 2), 0.3), rnd((B, T, 1), 0.01) + synth.H_COM, rnd((B, T, 3), 0.5), rnd((B, T, 3), 0.3)],
                       dim=2).to(dt).contiguous()
    desired = rnd((B, T, 12), 0.3).to(dt).contiguous()
    stand64 = torch.as_tensor(np.concatenate([synth.NOMINAL_FEET[:, :2], np.full((4, 1), synth.FOOT_Z)], axis=1), device=dev).expand(B, 4, 3)
    com = actual[:, :, None, 3:6].double() * torch.tensor([1.0, 1.0, 0.0], device=dev, dtype=torch.float64)
    feet_log = (com + stand64[:, None] + rnd((B, T, 4, 3), 0.01) * torch.tensor([1.0, 1.0, 0.0], device=dev, dtype=torch.float64)).to(dt).contiguous()
    forces = rnd((B, T, 12), 30.0).to(dt).contiguous()
    stand = stand64.to(dt).contiguous()
    gait = torch.as_tensor(gaits.gait_rows([names[b % 8] for b in range(B)], 12)).to(dev)
    tick0 = torch.zeros(B, dtype=torch.int32, device=dev)
    gain = torch.full((B,), 0.03, dtype=dt, device=dev)
    hh = torch.full((B,), 0.06, dtype=dt, device=dev)
    logs = {"actual": actual, "desired": desired, "feet_log": feet_log}
    sw = sol.phase_swing(logs, gait, tick0, stand, gain, hh)
    vel = sw["swing"][:, :, :, 1].contiguous()
    jr = sol.joint_rates(actual, forces, sw["feet_des"], vel)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    eng = sol.engine
    # (the raw calls: no allocation in the timed window)
    med, best = timed(lambda: eng.phase_swing_ptr(B, T, p(actual), p(desired), p(feet_log), p(gait), p(tick0), p(stand), p(gain), p(hh),
                                                   p(sw["swing"]), p(sw["feet_des"]), stream=st))
    med_n, _ = timed(lambda: eng.phase_swing_ptr(B, T, p(actual), p(desired), p(feet_log), p(gait), p(tick0), p(stand), p(gain), p(hh),
                                                 p(sw["swing"]), 0, stream=st))
    report("phase_swing", io, rows * (36 + 48 + 12) * el, med, best, ms_median_without_feet_des=round(med_n, 4),
           swing_share=round(float((sw["swing"][:, :, :, 1].abs().sum(dim=3) > 0).double().mean()), 3))
    med, best = timed(lambda: eng.joint_rates_ptr(B, T, p(actual), p(forces), p(sw["feet_des"]), p(vel), p(jr["q"]), p(jr["qd"]), p(jr["tau"]),
                                                   p(jr["power"]), p(jr["reach"]), stream=st))
    med_r, _ = timed(lambda: eng.joint_rates_ptr(B, T, p(actual), p(forces), p(sw["feet_des"]), 0, p(jr["q"]), p(jr["qd"]), p(jr["tau"]),
                                                 p(jr["power"]), p(jr["reach"]), stream=st))
    med_l, _ = timed(lambda: eng.joint_log_ptr(B, T, p(actual), p(forces), p(sw["feet_des"]), p(jr["q"]), p(jr["tau"]), p(jr["reach"]), stream=st))
    report("joint_rates", io, rows * ((48 + 36 + 4) * el + 4), med, best, ms_median_feet_at_rest=round(med_r, 4),
           ms_median_joint_log=round(med_l, 4), reach_share=round(float(jr["reach"].double().mean()), 4))
    del actual, desired, feet_log, forces, sw, vel, jr, logs, com
