#!/usr/bin/env python3
"""Record the fixtures of the bitwise identity test of the structured leg maps: tests/golden/legmap_identity_<case>.npz.

Run ONCE, on the GPU, at the commit whose outputs are the contract (the parent of the change to csrc/mpcqp_leg.h's leg maps):

    python tools/record_legmap_identity.py --commit $(git rev-parse HEAD) [--out tests/golden]

The layout is that of tools/record_accel_identity.py (inputs in the io dtype, kwargs as JSON, u / X / status / iters / res, the
commit); a case with per-robot model rows also stores them (`models`, fp64 [B,6]).  The cases reach the instantiations that the
seven accel_identity cases do not:
  n10_perleg   per-leg timing, N = 10 MIXED fp32 buffers, polish, B = 64: quads that mix swing and stance legs, one- and
               three-foot stages (where a zero's sign could travel); must hold a QP with more than 100 ADMM iterations
  n10_f64      precision f64, polish, B = 32: the ADMM-kind solve and E build in fp64
  n10_io64     MIXED with fp64 buffers, B = 32: the other MIXED instantiation
  n10_models   MIXED with set_models rows of differing mass, inertia and box, B = 32: the MODEL kernel, cm differs per QP
  n10_alpha0   alpha = 0 (continuation), B = 32: many fp64 polish solves; must hold a QP with more than one polish step
  n10_refine   flags = 0, precision f64, eps_abs = 1e-9, B = 16: the kernel with a refinement step per linear solve
  n20_f64      N = 20, precision f64, B = 16: four waves per QP in fp64
  n60_stage    N = 60, delta = 0.01, MIXED, B = 8: the stage-wise engine at the reference's own horizon
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import mpcqp  # noqa: E402
from record_accel_identity import GAITS, INPUTS, MUS, OUTPUTS  # noqa: E402

P = mpcqp.FLAG_POLISH


def solve(kw, b, models=None):
    """One solve on a fresh engine: (the inputs as the engine saw them, the outputs)."""
    import torch
    sol = mpcqp.MPCBatch(device=0, **kw)
    if models is not None:
        sol.set_models(models)
    npdt = np.float32 if kw["io_dtype"] == "f32" else np.float64
    dev = sol.upload(b)
    out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True)
    torch.cuda.synchronize()
    ins = {k: np.ascontiguousarray(b[k], dtype=np.uint8 if k == "contact" else npdt) for k in INPUTS}
    outs = {k: out[k].cpu().numpy().copy() for k in OUTPUTS}
    sol.engine.close()
    return ins, outs


def first_seed(kw, make, want, seeds=range(7, 60)):
    """The first seed whose batch `make(seed)`, solved with `kw`, satisfies want(batch, outputs)."""
    for seed in seeds:
        b = make(seed)
        if want(b, solve(kw, b)[1]):
            return seed, b
    raise SystemExit(f"no seed in {seeds} gives the batch that {kw} needs")


def stance_counts(contact):
    return np.unique(np.asarray(contact).sum(axis=2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)

    mk = lambda B, N, s, delta=0.03: mpcqp.synth.make_batch(B, N, delta, s, GAITS, MUS)
    n10 = dict(N=10, delta=0.03, io_dtype="f32", precision="mixed")
    f64 = dict(io_dtype="f64", precision="f64")

    def perleg_hard(b, out):
        n = stance_counts(b["contact"])
        return 1 in n and 3 in n and mpcqp.split_iters(out["iters"])[0].max() > 100
    kw_perleg = dict(n10, flags=P)
    s_perleg, b_perleg = first_seed(kw_perleg, lambda s: mpcqp.synth.make_perleg_batch(64, 10, 0.03, s), perleg_hard)
    kw_alpha0 = dict(n10, flags=P, alpha=0.0)
    s_alpha0, b_alpha0 = first_seed(kw_alpha0, lambda s: mk(32, 10, s), lambda b, out: mpcqp.split_iters(out["iters"])[1].max() > 1)

    cases = {
        "n10_perleg": (kw_perleg, b_perleg, None, s_perleg),
        "n10_f64": (dict(N=10, delta=0.03, flags=P, **f64), mk(32, 10, 7), None, 7),
        "n10_io64": (dict(N=10, delta=0.03, io_dtype="f64", precision="mixed", flags=P), mk(32, 10, 7), None, 7),
        "n10_models": (dict(n10, flags=P), mk(32, 10, 7), mpcqp.synth.make_model_rows(32), 7),
        "n10_alpha0": (kw_alpha0, b_alpha0, None, s_alpha0),
        "n10_refine": (dict(N=10, delta=0.03, flags=0, eps_abs=1e-9, **f64), mk(16, 10, 7), None, 7),
        "n20_f64": (dict(N=20, delta=0.03, flags=P, **f64), mk(16, 20, 7), None, 7),
        "n60_stage": (dict(N=60, delta=0.01, io_dtype="f32", precision="mixed", flags=P), mk(8, 60, 7, 0.01), None, 7),
    }
    for name, (kw, b, models, seed) in cases.items():
        ins, outs = solve(kw, b, models)
        data = {"commit": np.array(a.commit), "kwargs": np.array(json.dumps(kw)), "solves": np.array(1), "seed": np.array(seed)}
        if models is not None:
            data["models"] = np.ascontiguousarray(models, dtype=np.float64)
        data.update({f"in0_{k}": v for k, v in ins.items()})
        data.update({f"out0_{k}": v for k, v in outs.items()})
        path = os.path.join(a.out, f"legmap_identity_{name}.npz")
        np.savez_compressed(path, **data)
        admm, pol = mpcqp.split_iters(outs["iters"])
        st = outs["status"]
        print(f"{name:11s} seed {seed} B {len(st)} solved {int(((st == 1) | (st == 2)).sum())} admm max {int(admm.max())} "
              f"mean {admm.mean():.1f} over-100 {int((admm > 100).sum())} polish max {int(pol.max())} "
              f"stance feet per stage {stance_counts(ins['contact']).tolist()} {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
