#!/usr/bin/env python3
"""Record the fixtures of a bitwise identity test of solve_batch: tests/golden/accel_identity_<case>.npz.

Run ONCE, on the GPU, at the commit whose outputs are the contract (the parent of the change under test):

    python tools/record_accel_identity.py --commit $(git rev-parse HEAD) [--out tests/golden]

Every fixture holds the inputs of its solves (in the engine's io dtype), the engine's keyword arguments as JSON, the outputs
u / X / status / iters / res of every solve, and the commit they were recorded at.  The test feeds the stored inputs to the
engine built from the tree under test and compares the outputs bit for bit; it need not regenerate a batch.

The cases are the smallest that reach every path an Anderson step runs on (csrc/mpcqp_leg.h: w_aa_step):
  n10_mixed       N = 10 MIXED, polish, B = 96, four gaits, mu in {0.3, 0.5, 0.7, 1.0}: one wave per QP, history in registers;
                  must hold QPs with more than 100 ADMM iterations (a second round, whose segment start clears the history)
  n10_natural     the same batch with MPCQP_FLAG_NATURAL_ORDER (one workgroup per QP)
  n20_mixed       N = 20 MIXED, B = 32: four waves per QP, history parked in LDS between extrapolations
  n10_stage       N = 10 with MPCQP_FLAG_STAGE_KERNEL, B = 32: stage-wise engine, one-level chain (fp32 buffers, like the dense cases)
  n24_stage       N = 24, delta = 0.03, B = 16: stage-wise engine, two-level chain (fp64 buffers: the other instantiation)
  n10_warm        N = 10 warm start, two consecutive control ticks, B = 32: short first block next to the segment-end rule
  n10_admm_only   N = 10 without MPCQP_FLAG_POLISH, B = 32: acceleration off
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp  # noqa: E402

GAITS, MUS = ("trot", "pronk", "amble", "gallop"), (0.3, 0.5, 0.7, 1.0)
INPUTS, OUTPUTS = ("x0", "r", "contact", "xdes", "mu"), ("u", "X", "status", "iters", "res")
P = mpcqp.FLAG_POLISH


def next_tick(b, X, N):
    """The QP one control tick later (as tests/test_gpu_warm_start.py builds it): the robot at the first predicted state."""
    nb = {k: np.array(v, copy=True) for k, v in b.items()}
    nb["x0"] = np.array(X[:, 1, :], dtype=np.float64)
    nb["x0"][:, 12] = b["x0"][:, 12]
    step = b["xdes"][:, 1, :] - b["xdes"][:, 0, :]
    nb["xdes"] = b["xdes"] + step[:, None, :]
    nb["xdes"][:, :, 12] = b["xdes"][:, :, 12]
    nb["t0"] = b["t0"] + 1
    nb["contact"] = mpcqp.synth.contact_schedule(b["gait_ids"], nb["t0"], N, gaits=mpcqp.synth.gait_patterns(GAITS))
    feet = b["r"][:, 1] + b["xdes"][:, 1, None, 3:6]
    nb["r"] = feet[:, None, :, :] - nb["xdes"][:, :-1, None, 3:6]
    nb["r"][:, 0] = feet - nb["x0"][:, None, 3:6]
    return nb


def first_seed(B, want):
    """The first seed from 7 on whose batch holds a QP with more than 100 ADMM iterations (a second round) -- `want(out)`."""
    for seed in range(7, 40):
        b = mpcqp.synth.make_batch(B, 10, 0.03, seed, GAITS, MUS)
        out = solve(dict(N=10, delta=0.03, io_dtype="f32", precision="mixed", flags=P), [b])[1][0]
        if want(b, out):
            return seed, b
    raise SystemExit("no seed in 7..39 gives a batch with a second round")


def solve(kw, batches, chain=False):
    """Solves on ONE engine, in order.  chain: batch i + 1 is the next control tick of batch i's answer (warm start).
    Returns (the inputs as the engine saw them, the outputs), one entry per solve."""
    import torch
    sol = mpcqp.MPCBatch(device=0, **kw)
    npdt = np.float32 if kw["io_dtype"] == "f32" else np.float64
    ins, outs = [], []
    b = batches[0]
    for i in range(len(batches) if not chain else 2):
        if i and not chain:
            b = batches[i]
        dev = sol.upload(b)
        out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True)
        torch.cuda.synchronize()
        ins.append({k: np.ascontiguousarray(b[k], dtype=np.uint8 if k == "contact" else npdt) for k in INPUTS})
        outs.append({k: out[k].cpu().numpy().copy() for k in OUTPUTS})
        if chain:
            b = next_tick(b, outs[-1]["X"], kw["N"])
    sol.engine.close()
    return ins, outs


def two_leg_low_mu(b):
    return bool(np.any((b["contact"].sum(axis=2) == 2).any(axis=1) & (b["mu"] == 0.3)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)

    def hard(b, out):
        admm = mpcqp.split_iters(out["iters"])[0]
        return two_leg_low_mu(b) and admm.max() > 100
    seed, b96 = first_seed(96, hard)
    mk = lambda B, N, s: mpcqp.synth.make_batch(B, N, 0.03, s, GAITS, MUS)
    n10 = dict(N=10, delta=0.03, io_dtype="f32", precision="mixed")
    cases = {
        "n10_mixed": (dict(n10, flags=P), [b96], False),
        "n10_natural": (dict(n10, flags=P | mpcqp.FLAG_NATURAL_ORDER), [b96], False),
        "n20_mixed": (dict(N=20, delta=0.03, io_dtype="f32", precision="mixed", flags=P), [mk(32, 20, 7)], False),
        "n10_stage": (dict(n10, flags=P | mpcqp.FLAG_STAGE_KERNEL), [mk(32, 10, 7)], False),
        "n24_stage": (dict(N=24, delta=0.03, io_dtype="f64", precision="mixed", flags=P), [mk(16, 24, 7)], False),
        "n10_warm": (dict(n10, flags=P, warm_start=True), [mk(32, 10, 7)], True),
        "n10_admm_only": (dict(n10, flags=0), [mk(32, 10, 7)], False),
    }
    for name, (kw, batches, chain) in cases.items():
        ins, outs = solve(kw, batches, chain)
        data = {"commit": np.array(a.commit), "kwargs": np.array(json.dumps(kw)), "solves": np.array(len(outs)),
                "seed": np.array(seed if batches[0] is b96 else 7)}
        for i, (bi, oi) in enumerate(zip(ins, outs)):
            data.update({f"in{i}_{k}": v for k, v in bi.items()})
            data.update({f"out{i}_{k}": v for k, v in oi.items()})
        path = os.path.join(a.out, f"accel_identity_{name}.npz")
        np.savez_compressed(path, **data)
        admm, pol = mpcqp.split_iters(outs[-1]["iters"])
        st = outs[-1]["status"]
        print(f"{name:14s} seed {int(data['seed'])} B {len(st)} solved {int(((st == 1) | (st == 2)).sum())} admm max {int(admm.max())} "
              f"mean {admm.mean():.1f} over-100 {int((admm > 100).sum())} polish max {int(pol.max())} {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
