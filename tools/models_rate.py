"""Developer tool: what per-robot model rows (include/mpcqp_model.h) cost.

1. The headline workload WITHOUT a table (bench.py's configuration: config 3, B = 4096, N = 10, f32 buffers, MIXED) on this
   library and on another build of it (`--parent PATH`, e.g. the parent commit's libmpcqp.so), alternating the two libraries,
   `--repeats` repeats each of `--steps` solves (host clock around a device synchronise).  Requirement: this library's median QP/s
   is not below the parent's by more than the parent's own min-max spread.
2. The same batch with synth.make_model_rows set and with the configuration's row set (recorded only).
3. mpcqp_set_models at B = 65 536 (recorded only).
usage: models_rate.py [--parent PATH] [--repeats 7] [--steps 30]"""
import argparse, json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import _capi, models

ap = argparse.ArgumentParser()
ap.add_argument("--parent"); ap.add_argument("--repeats", type=int, default=7); ap.add_argument("--steps", type=int, default=30)
args = ap.parse_args()
B, N = 4096, 10
batch = mpcqp.synth.config3(B=B)
t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()
dev = {k: t(batch[k]) for k in ("x0", "r", "xdes", "mu")}
dev["contact"] = t(batch["contact"], torch.uint8)
out = {"u": torch.zeros((B, N, 12), device="cuda"), "status": torch.zeros(B, dtype=torch.int32, device="cuda"),
       "iters": torch.zeros(B, dtype=torch.int32, device="cuda")}


def engine(lib):
    e = _capi.Engine(lib, lib.default_config(N=N, delta=0.03, dtype=_capi.DTYPE_F32, precision=_capi.PREC_MIXED,
                                             flags=_capi.FLAG_POLISH | _capi.FLAG_NO_TIMING))
    e.reserve(B)
    return e


def rate(e, steps):
    call = lambda: e.solve_batch_ptr(B, dev["x0"].data_ptr(), dev["r"].data_ptr(), dev["contact"].data_ptr(), dev["xdes"].data_ptr(),
                                     dev["mu"].data_ptr(), out["u"].data_ptr(), 0, out["status"].data_ptr(), out["iters"].data_ptr(), 0,
                                     torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    return B * steps / (time.perf_counter() - t0)


libs = {"this": mpcqp.product_library()}
if args.parent:
    libs["parent"] = _capi.Library(args.parent)
engines = {k: engine(l) for k, l in libs.items()}
runs = {k: [] for k in engines}
for _ in range(args.repeats):
    for k, e in engines.items():
        runs[k].append(rate(e, args.steps))
res = {k: {"median_MQPs": round(float(np.median(v)) / 1e6, 3), "min": round(min(v) / 1e6, 3), "max": round(max(v) / 1e6, 3)} for k, v in runs.items()}
res["solved"] = float(np.isin(out["status"].cpu().numpy(), (1, 2)).mean())
if args.parent:
    spread = (max(runs["parent"]) - min(runs["parent"])) / 1e6
    res["parent_spread_MQPs"] = round(spread, 3)
    res["no_table_within_parent_spread"] = bool(res["this"]["median_MQPs"] >= res["parent"]["median_MQPs"] - spread)
print(json.dumps({"no_table": res}), flush=True)

e = engines["this"]
for name, rows in (("make_model_rows", mpcqp.synth.make_model_rows(B)), ("configuration_row", models.model_rows(e.cfg, B))):
    rd = torch.as_tensor(rows).cuda()
    e.set_models_ptr(B, rd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    v = [rate(e, args.steps) for _ in range(args.repeats)]
    print(json.dumps({name: {"median_MQPs": round(float(np.median(v)) / 1e6, 3), "min": round(min(v) / 1e6, 3), "max": round(max(v) / 1e6, 3),
                             "solved": float(np.isin(out["status"].cpu().numpy(), (1, 2)).mean())}}), flush=True)
e.clear_models()

Bs = 65536
rd = torch.as_tensor(mpcqp.synth.make_model_rows(Bs)).cuda()
st = torch.cuda.current_stream().cuda_stream
e.set_models_ptr(Bs, rd.data_ptr(), st)   # (the first call at a size allocates)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
best = float("inf")
for _ in range(20):
    e0.record(); e.set_models_ptr(Bs, rd.data_ptr(), st); e1.record(); e1.synchronize()
    best = min(best, e0.elapsed_time(e1))
print(json.dumps({"set_models_B65536_ms": round(best, 4)}), flush=True)
