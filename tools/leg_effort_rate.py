"""Developer tool: rate of the full joint torques of a roll-out's log (include/mpcqp_joints.h, mpcqp_leg_effort) next to the joint rates
it extends (mpcqp_joint_rates) and of the leg's equations of motion (mpcqp_leg_dynamics).  B = 65 536 robots x T = 50 log rows (13.1 M
legs), fp32 and fp64 I/O; the logs are synthetic and made on the device as in tools/phase_swing_rate.py: random torso states, feet
under the nominal stance, the eight named gaits at period 12, the swing feet's velocities and accelerations from mpcqp_phase_swing.
Times one call with HIP events, median and best of 20 after 3 warm-ups, and reports the HBM bytes the call has to move over that
time against the 8 TB/s roof.  Per robot-tick mpcqp_leg_effort with base_acc = NULL reads 12 + 4 x (3 + 3 + 3 + 3) = 60 values and
writes 4 x (3 + 3 + 3 + 1) = 40 values and 4 bytes: 404 B in fp32, 804 B in fp64 (the plant's right-hand side sums the row's
forces and moments across the four lanes of the row, not from memory).
usage: leg_effort_rate.py [--quick]"""
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
                      "MB": round(by / 1e6, 1), "bytes_per_robot_tick": by // (B * T), "TBps": round(by / med / 1e9, 3),
                      "share_of_8TBps_roof": round(by / med / 1e9 / HBM_TBPS, 3), "G_legs_per_s": round(4 * B * T / med / 1e6, 3), **more}),
          flush=True)


names = tuple(gaits.GAITS)
rows = B * T
for io in ("f32", "f64"):
    el = 4 if io == "f32" else 8
    sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed")
    dt, dev = sol.tdtype, sol.device
    gen = torch.Generator(device=dev).manual_seed(20251019)
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
    sw = sol.phase_swing({"actual": actual, "desired": desired, "feet_log": feet_log}, gait, tick0, stand, gain, hh)
    feet, vel, acc = sw["feet_des"], sw["swing"][:, :, :, 1].contiguous(), sw["swing"][:, :, :, 2].contiguous()
    del sw, desired, feet_log, com
    base_acc = torch.cat([rnd((B, T, 3), 3.0), rnd((B, T, 3), 2.0)], dim=2).to(dt).contiguous()
    out = sol.leg_effort(actual, forces, feet, vel, acc)
    jr = sol.joint_rates(actual, forces, feet, vel)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    eng = sol.engine
    o = [p(out[k]) for k in ("qdd", "tau_dyn", "tau", "power", "limit")]
    # (the raw calls: no allocation in the timed window)
    med, best = timed(lambda: eng.leg_effort_ptr(B, T, p(actual), p(forces), p(feet), p(vel), p(acc), 0, 0, *o, stream=st))
    med_b, _ = timed(lambda: eng.leg_effort_ptr(B, T, p(actual), p(forces), p(feet), p(vel), p(acc), p(base_acc), 0, *o, stream=st))
    med_t, _ = timed(lambda: eng.leg_effort_ptr(B, T, p(actual), p(forces), p(feet), p(vel), p(acc), 0, 0, 0, 0, o[2], 0, o[4], stream=st))
    med_r, _ = timed(lambda: eng.joint_rates_ptr(B, T, p(actual), p(forces), p(feet), p(vel), p(jr["q"]), p(jr["qd"]), p(jr["tau"]),
                                                 p(jr["power"]), p(jr["reach"]), stream=st))
    lim = out["limit"]
    report("leg_effort", io, rows * ((60 + 40) * el + 4), med, best, ms_median_with_base_acc=round(med_b, 4),
           ms_median_tau_and_limit_only=round(med_t, 4), ms_median_joint_rates=round(med_r, 4),
           flagged_share=round(float((lim != 0).double().mean()), 4), nonfinite_share=round(float((lim == 255).double().mean()), 6))
    del out, jr, base_acc
    q = (rnd((rows, 4, 3), 0.3) + torch.tensor([0.0, -1.0, 1.6], device=dev, dtype=torch.float64)).to(dt).contiguous()
    qd, qdd = rnd((rows, 4, 3), 2.0).to(dt).contiguous(), rnd((rows, 4, 3), 20.0).to(dt).contiguous()
    dyn = sol.leg_dynamics(q, qd, qdd)
    torch.cuda.synchronize()
    med, best = timed(lambda: eng.leg_dynamics_ptr(rows, p(q), p(qd), p(qdd), 0, 0, p(dyn["tau"]), p(dyn["mass"]), p(dyn["bias"]), stream=st))
    med_t, _ = timed(lambda: eng.leg_dynamics_ptr(rows, p(q), p(qd), p(qdd), 0, 0, p(dyn["tau"]), 0, 0, stream=st))
    report("leg_dynamics", io, rows * 4 * (9 + 15) * el, med, best, ms_median_tau_only=round(med_t, 4))
    del actual, forces, feet, vel, acc, q, qd, qdd, dyn
