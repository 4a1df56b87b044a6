"""Developer tool: rate of the joint-space log (include/mpcqp_joints.h, mpcqp_joint_log) next to the host code it replaces.
B = 65 536 robots x T = 50 ticks (13.1 M legs), fp32 and fp64 I/O; the logs are synthetic: random torso poses, feet = CoM + R FK(q) of
in-box joint angles (made with the device's own forward map), random forces.  Times one call with HIP events, median and best of 20
after 3 warm-ups, and reports the HBM bytes the call has to move (actual, forces, feet read once; q, tau, reach written) over that
time.  The host side: lite3_model.joint_log_host on 1/64 of the batch and the Newton loop lite3_model.leg_ik on 1/4096 of it, both
scaled up to the whole batch.
usage: joint_log_rate.py [--quick]"""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import lite3_model
from scipy.spatial.transform import Rotation

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


rng = np.random.default_rng(20251018)
rows = B * T
q = np.stack([rng.uniform(-0.5, 0.5, (rows, 4)), rng.uniform(-1.5, -0.2, (rows, 4)), rng.uniform(0.5, 2.3, (rows, 4))], axis=2)
actual = np.zeros((rows, 12))
actual[:, 0:3] = rng.normal(0.0, 0.15, (rows, 3))
actual[:, 3:6] = rng.normal(0.0, 0.5, (rows, 3)) + [0.0, 0.0, 0.285]
forces = rng.normal(0.0, 30.0, (rows, 12))
R = Rotation.from_rotvec(actual[:, :3]).as_matrix()
host = None
for io in ("f32", "f64"):
    el = 4 if io == "f32" else 8
    sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=sol.tdtype).cuda().contiguous()
    ta, tf = t(actual).view(B, T, 12), t(forces).view(B, T, 12)
    _, foot = sol.leg_jacobians(t(q), t(R))
    feet = (foot + ta.view(rows, 12)[:, None, 3:6]).view(B, T, 4, 3).contiguous()
    del foot
    out = sol.joint_log(ta, tf, feet)
    torch.cuda.synchronize()
    err = float((out["q"].view(rows, 4, 3).double().cpu() - torch.as_tensor(q)).abs().max())
    ptrs = (ta.data_ptr(), tf.data_ptr(), feet.data_ptr(), out["q"].data_ptr(), out["tau"].data_ptr(), out["reach"].data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    med, best = timed(lambda: sol.engine.joint_log_ptr(B, T, *ptrs, stream=st))      # (the raw call: no allocation in the timed window)
    med_q, _ = timed(lambda: sol.engine.joint_log_ptr(B, T, ptrs[0], ptrs[1], ptrs[2], ptrs[3], 0, ptrs[5], stream=st))
    by = rows * (12 * el + 12 * el + 12 * el + 12 * el + 12 * el + 4)
    r = {"io": io, "B": B, "T": T, "legs": 4 * rows, "ms_median": round(med, 4), "ms_best": round(best, 4), "MB": round(by / 1e6, 1),
         "TBps": round(by / med / 1e9, 3), "share_of_8TBps_roof": round(by / med / 1e9 / HBM_TBPS, 3),
         "G_legs_per_s": round(4 * rows / med / 1e6, 3), "ms_median_without_tau": round(med_q, 4),
         "reach_all": bool(out["reach"].all()), "max_q_error_vs_drawn": err}
    print(json.dumps(r), flush=True)
    if io == "f64":
        n = max(1, B // 64)
        host = [a[:n].cpu().numpy() for a in (ta, tf, feet)]
    del ta, tf, feet, out

# the host code it replaces
n = host[0].shape[0]
t0 = time.perf_counter()
lite3_model.joint_log_host(*host)
s_log = time.perf_counter() - t0
m = max(1, B // 4096)
Rm = R.reshape(B, T, 3, 3)[:m]
pb = np.einsum("btji,btlj->btli", Rm, host[2][:m] - host[0][:m, :, None, 3:6])
t0 = time.perf_counter()
for b in range(m):
    for k in range(T):
        for l in range(4):
            lite3_model.leg_ik(l, pb[b, k, l])
s_newton = time.perf_counter() - t0
print(json.dumps({"host_joint_log_robots": n, "host_joint_log_s": round(s_log, 2), "host_joint_log_s_at_B": round(s_log * B / n, 1),
                  "newton_ik_robots": m, "newton_ik_s": round(s_newton, 2), "newton_ik_s_at_B": round(s_newton * B / m, 1),
                  "newton_ik_us_per_leg": round(s_newton / (m * T * 4) * 1e6, 1)}), flush=True)
