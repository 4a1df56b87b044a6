"""Developer tool: rate of the state estimator over a roll-out's log (include/mpcqp_estimate.h, mpcqp_estimate_track and mpcqp_imu_log)
next to the inverse dynamics of the same log (mpcqp_leg_effort) in the same run.  B = 65 536 and 4096 robots x T = 50 log rows, fp32
and fp64 I/O; the logs are synthetic and made on the device as in tools/swing_track_rate.py: random torso states, feet under the
nominal stance, the contact mask from the clock of the eight named gaits at period 12, the encoders from mpcqp_joint_rates with the
feet at rest, the IMU rows from mpcqp_imu_log.  Times one call with HIP events: median, best and worst of 20 after 3 warm-ups.
Per robot-row mpcqp_estimate_track reads 6 + 24 values and 4 bytes and writes 12 + 12 + 6 + 1 values: 248 B in fp32, 492 B in fp64; the
filter is serial in T, four lanes per robot, and a lane strides by a whole robot (T rows) from its neighbour's.
usage: estimate_rate.py [--quick]   (--quick: the 4096-robot size only)"""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import gaits, synth

SIZES = (4096,) if "--quick" in sys.argv else (65536, 4096)
T = 50


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


names = tuple(gaits.GAITS)
for io in ("f32", "f64"):
    el = 4 if io == "f32" else 8
    sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed")
    dt, dev = sol.tdtype, sol.device
    for B in SIZES:
        rows = B * T
        gen = torch.Generator(device=dev).manual_seed(20251020)
        rnd = lambda shape, sd: torch.randn(shape, generator=gen, device=dev, dtype=torch.float64) * sd
        actual = torch.cat([rnd((B, T, 3), 0.1), rnd((B, T, 2), 0.3), rnd((B, T, 1), 0.01) + synth.H_COM, rnd((B, T, 3), 0.5), rnd((B, T, 3), 0.3)],
                           dim=2).to(dt).contiguous()
        stand64 = torch.as_tensor(np.concatenate([synth.NOMINAL_FEET[:, :2], np.full((4, 1), synth.FOOT_Z)], axis=1), device=dev).expand(B, 4, 3)
        com = actual[:, :, None, 3:6].double() * torch.tensor([1.0, 1.0, 0.0], device=dev, dtype=torch.float64)
        feet_log = (com + stand64[:, None] + rnd((B, T, 4, 3), 0.01) * torch.tensor([1.0, 1.0, 0.0], device=dev, dtype=torch.float64)).to(dt).contiguous()
        gait_np = gaits.gait_rows([names[b % 8] for b in range(8)], 12)
        contact_np = gaits.phase_contact(gait_np, np.zeros(8, np.int32), T)
        contact = torch.as_tensor(np.ascontiguousarray(np.tile(contact_np, (B // 8, 1, 1)))).to(dev).contiguous()
        forces = (rnd((B, T, 12), 30.0).view(B, T, 4, 3) * contact[..., None].double()).view(B, T, 12).to(dt).contiguous()
        logs = {"actual": actual, "forces": forces, "feet_log": feet_log, "contact_log": contact}
        jr = sol.joint_rates(actual, forces, feet_log)
        q, qd = jr["q"], jr["qd"]
        imu = sol.imu_log(logs)
        init = actual[:, 0].contiguous()
        state = torch.zeros((B, mpcqp._capi.EST_STATE), dtype=torch.float64, device=dev)
        out = sol.estimate_track(imu, q, qd, contact, init, state=state)
        ef = sol.leg_effort(actual, forces, feet_log)
        torch.cuda.synchronize()
        st = torch.cuda.current_stream().cuda_stream
        p = lambda t: t.data_ptr()
        eng = sol.engine
        o = [p(out[k]) for k in sol.EST_OUT]
        # (the raw calls: no allocation in the timed window; state = NULL, so that every call does the same work)
        med, best, worst = timed(lambda: eng.estimate_track_ptr(B, T, p(imu), p(q), p(qd), p(contact), 0, 0, p(init), 0, *o, stream=st))
        med_i, best_i, worst_i = timed(lambda: eng.imu_log_ptr(B, T, p(actual), p(forces), p(feet_log), 0, 0, 0, 0, p(imu), stream=st))
        med_e, best_e, worst_e = timed(lambda: eng.leg_effort_ptr(B, T, p(actual), p(forces), p(feet_log), 0, 0, 0, 0, *[p(ef[k]) for k in
                                                                 ("qdd", "tau_dyn", "tau", "power", "limit")], stream=st))
        by = rows * ((30 + 31) * el + 4)
        print(json.dumps({"call": "estimate_track", "io": io, "B": B, "T": T, "ms_median": round(med, 4), "ms_best": round(best, 4),
                          "ms_worst": round(worst, 4), "MB": round(by / 1e6, 1), "GBps": round(by / med / 1e6, 1),
                          "M_robot_rows_per_s": round(rows / med / 1e3, 2), "ms_median_imu_log": round(med_i, 4), "ms_best_imu_log": round(best_i, 4),
                          "ms_worst_imu_log": round(worst_i, 4), "ms_median_leg_effort": round(med_e, 4), "ms_best_leg_effort": round(best_e, 4),
                          "ms_worst_leg_effort": round(worst_e, 4), "times_leg_effort": round(med / med_e, 2),
                          "nonfinite_share": round(float((~torch.isfinite(out["nis"])).double().mean()), 6)}), flush=True)
        del actual, forces, feet_log, contact, logs, jr, q, qd, imu, init, state, out, ef, com
