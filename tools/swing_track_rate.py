"""Developer tool: rate of the swing-leg tracker over a roll-out's log (include/mpcqp_joints.h, mpcqp_swing_track) next to the inverse
dynamics of the same log (mpcqp_leg_effort) and of the leg's forward dynamics (mpcqp_leg_accel).  B = 65 536 robots x T = 50 log rows
(13.1 M legs), fp32 and fp64 I/O; the logs are synthetic and made on the device as in tools/leg_effort_rate.py: random torso states,
feet under the nominal stance, the eight named gaits at period 12, the swing operand from mpcqp_phase_swing, the contact mask from
the gait clock.  Times one call with HIP events, median and best of 20 after 3 warm-ups.  Per robot-tick mpcqp_swing_track with
base_acc = NULL reads 12 + 4 x (3 + 3 + 12) = 84 values and 4 bytes and writes 4 x (3 + 3 + 3 + 3 + 1) = 52 values and 4 bytes:
552 B in fp32, 1096 B in fp64; a lane strides by a whole row (12 T values of `actual`) from its neighbour's robot.  The work is in
the control periods: 15 per swing row at delta = 0.03, each one recursion with velocity terms and three without.
usage: swing_track_rate.py [--quick]"""
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
    stand = stand64.to(dt).contiguous()
    gait_np = gaits.gait_rows([names[b % 8] for b in range(8)], 12)
    contact_np = gaits.phase_contact(gait_np, np.zeros(8, np.int32), T)              # [8,T,4]: the clock of the eight gaits
    contact = torch.as_tensor(np.ascontiguousarray(np.tile(contact_np, (B // 8, 1, 1)))).to(dev).contiguous()
    forces = (rnd((B, T, 12), 30.0).view(B, T, 4, 3) * contact[..., None].double()).view(B, T, 12).to(dt).contiguous()   # a swing leg's force is a zero
    gait = torch.as_tensor(np.tile(gait_np, (B // 8, 1))).to(dev).contiguous()
    tick0 = torch.zeros(B, dtype=torch.int32, device=dev)
    gain = torch.full((B,), 0.03, dtype=dt, device=dev)
    hh = torch.full((B,), 0.06, dtype=dt, device=dev)
    logs = {"actual": actual, "desired": desired, "forces": forces, "feet_log": feet_log, "contact_log": contact}
    sw = sol.phase_swing(logs, gait, tick0, stand, gain, hh)
    swing, feet = sw["swing"], sw["feet_des"]
    vel, acc = swing[:, :, :, 1].contiguous(), swing[:, :, :, 2].contiguous()
    del desired, com
    out = sol.swing_track(logs, swing)
    ef = sol.leg_effort(actual, forces, feet, vel, acc)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    eng = sol.engine
    o = [p(out[k]) for k in sol.SWING_OUT]
    ins = (p(actual), p(forces), p(feet_log), p(contact), p(swing))
    # (the raw calls: no allocation in the timed window)
    med, best = timed(lambda: eng.swing_track_ptr(B, T, *ins, 0, 0, 0, 0, 0, *o, stream=st))
    med_1, _ = timed(lambda: eng.swing_track_ptr(B, T, *ins, 0, 0, 0, 0, 1, *o, stream=st))
    med_e, _ = timed(lambda: eng.leg_effort_ptr(B, T, p(actual), p(forces), p(feet), p(vel), p(acc), 0, 0, *[p(ef[k]) for k in
                                                ("qdd", "tau_dyn", "tau", "power", "limit")], stream=st))
    flag = out["flag"]
    periods = float((contact == 0).double().sum()) * 15
    report("swing_track", io, rows * ((84 + 52) * el + 8), med, best, ms_median_one_period_per_tick=round(med_1, 4),
           ms_median_leg_effort=round(med_e, 4), times_leg_effort=round(med / med_e, 2), swing_share=round(float((flag & 1).double().mean()), 4),
           G_control_periods_per_s=round(periods / med / 1e6, 3), clamped_share=round(float(((flag & 2) != 0).double().mean()), 4),
           nonfinite_share=round(float((flag == 255).double().mean()), 6))
    del out, ef, swing, vel, acc, feet, logs
    q = (rnd((rows, 4, 3), 0.3) + torch.tensor([0.0, -1.0, 1.6], device=dev, dtype=torch.float64)).to(dt).contiguous()
    qd, tau = rnd((rows, 4, 3), 2.0).to(dt).contiguous(), rnd((rows, 4, 3), 2.0).to(dt).contiguous()
    fa = sol.leg_accel(q, tau, qd)
    torch.cuda.synchronize()
    med, best = timed(lambda: eng.leg_accel_ptr(rows, p(q), p(qd), p(tau), 0, 0, p(fa["qdd"]), p(fa["det"]), stream=st))
    report("leg_accel", io, rows * 4 * (9 + 4) * el, med, best)
    del actual, forces, feet_log, contact, q, qd, tau, fa
