"""Diagnostic: where a stage-wise solve spends its time, from the -DMPCQP_STAMPS build (never the product library).
usage: python tools/stage_stamps.py [N] [B] [mixed|f64] [logged]"""
import ctypes, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, os.path.join(REPO, "oracle"))
import mpcqp
from mpcqp import _capi
lib = _capi.Library(os.path.join(REPO, "mpc-for-dynamic-locomotion-in-the-mit-cheetah-3_amd", "csrc", "libmpcqp_stamps.so"))
_capi._product = lib
N = int(sys.argv[1]) if len(sys.argv) > 1 else 60
B = int(sys.argv[2]) if len(sys.argv) > 2 else 256
prec = sys.argv[3] if len(sys.argv) > 3 else "mixed"
if len(sys.argv) > 4 and sys.argv[4] == "logged":
    from test_gpu_reference_horizon import logged_run_inputs
    g = {k: np.load(os.path.join(REPO, "tests", "golden", k + ".npz")) for k in ("ref_log", "planner_golden", "qp_inputs", "qp_optima")}
    batch = logged_run_inputs(g, N, np.arange(B)); delta = 0.01
else:
    delta = 0.01 if N == 60 else 0.03
    batch = mpcqp.synth.make_batch(B, N, delta, 5, ("trot", "pronk", "amble", "gallop"), (0.3, 0.5, 0.7, 1.0))
sol = mpcqp.MPCBatch(N=N, delta=delta, precision=prec, flags=mpcqp.FLAG_POLISH | mpcqp.FLAG_STAGE_KERNEL)
dev = sol.upload(batch)
names = ["setup", "admm: E + factorisation", "admm: iterations", "admm: rho check", "polish: E + factorisation", "polish: gradient", "polish: solve",
         "polish: rule / kkt / rest", "output", "(rounds, total)"]
buf = (ctypes.c_ulonglong * 32)()
for rep in range(2):
    out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"])
    torch.cuda.synchronize()
    lib.lib.mpcqp_debug_read_stamps(buf)
v = np.array(list(buf), dtype=np.float64)
it = out["iters"].cpu().numpy()
tot = v[0] + v[8] + v[9]
print(f"N={N} B={B} {prec}: kernel {sol.last_kernel_ms():.2f} ms; iterations mean {mpcqp.split_iters(it)[0].mean():.0f}, polish steps mean {mpcqp.split_iters(it)[1].mean():.2f}; "
      f"cycles/QP {tot / B:.0f} (100 MHz? no: shader clock)")
for i, nme in enumerate(names):
    print(f"  {nme:28s} share {v[i] / tot:6.1%}  cycles/QP {v[i] / B:10.0f}  events/QP {v[16 + i] / B:7.2f}  cycles/event {v[i] / max(v[16 + i], 1):9.0f}")
