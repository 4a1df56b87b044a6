#!/usr/bin/env python3
"""Record the fixtures of the bitwise identity test of the ADMM projection: tests/golden/projection_identity_<case>.npz.

Run ONCE, on the GPU, at the commit whose outputs are the contract (the parent of the change to the clamp in w_admm and
leg_admm_project):

    python tools/record_projection_identity.py --commit $(git rev-parse HEAD) [--out tests/golden]

The layout is that of tools/record_accel_identity.py (inputs in fp32 / uint8, kwargs as JSON, u / X / status / iters / res of every
solve, the commit), with three additions that keep every file of 64 QPs under 135 KB:
  inputs_of   a case may name another case whose stored inputs are its own first solve's inputs (widened to the io dtype, which is
              exact: every case's inputs are fp32 values);
  models      per-robot model rows (fp64 [B,6]) where a case sets them;
  box         the configuration's (f_min, f_max), for the self-checks of the test.
The warm case stores the second tick's inputs and, of the first tick, u / status / iters / res (its X is where the second tick's x0
comes from; the second tick's outputs are stored in full).

Every case is N = 10, B = 64, MIXED (fp32 iteration tile: the kernels whose projection changes).  The cases sit where a clamp can go wrong:
  lowmu       trot at mu = 0.3: two-leg support with the friction rows active; must hold a QP with more than 100 ADMM iterations
  swingmix    per-leg timing with one- and three-foot stages: quads that mix lo = hi = 0 with stance bounds
  fzbox       model rows with a tight f_z box (f_min 8 - 12 N, f_max 25 - 40 N): lo0 and hi0 are both hit
  admm_only   polish off: the ADMM iterate's own bits are the output
  warm        warm start plus shift, two consecutive control ticks
  io64        the lowmu batch through MIXED with fp64 buffers
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
from record_accel_identity import GAITS, INPUTS, MUS, OUTPUTS, next_tick  # noqa: E402

P = mpcqp.FLAG_POLISH
B, N, DELTA = 64, 10, 0.03


def as_f32(b):
    """The batch with every float input rounded to fp32 (kept in fp64): what an fp32 engine sees, and exact in an fp64 one."""
    return {k: (np.asarray(v, dtype=np.float32).astype(np.float64) if k in INPUTS and k != "contact" else v) for k, v in b.items()}


def solve(kw, batches, models=None, chain=False):
    """Solves on ONE engine, in order (chain: the second batch is the next control tick of the first one's answer).
    Returns (inputs, outputs, (f_min, f_max)), one entry per solve."""
    import torch
    sol = mpcqp.MPCBatch(device=0, **kw)
    if models is not None:
        sol.set_models(models)
    ins, outs = [], []
    b = batches[0]
    for i in range(2 if chain else len(batches)):
        if i and not chain:
            b = batches[i]
        dev = sol.upload(b)
        out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True)
        torch.cuda.synchronize()
        ins.append({k: np.ascontiguousarray(b[k], dtype=np.uint8 if k == "contact" else np.float32) for k in INPUTS})
        outs.append({k: out[k].cpu().numpy().copy() for k in OUTPUTS})
        if chain:
            b = as_f32(next_tick(b, outs[-1]["X"], kw["N"]))
    box = (float(sol.cfg.f_min), float(sol.cfg.f_max))
    sol.engine.close()
    return ins, outs, box


def first_seed(kw, make, want, seeds=range(7, 60)):
    for seed in seeds:
        b = as_f32(make(seed))
        if want(b, solve(kw, [b])[1][0]):
            return seed, b
    raise SystemExit(f"no seed in {seeds} gives the batch that {kw} needs")


def bound_counts(u, contact, mu, lo, hi):
    """Leg-stages of a solve whose force ends exactly on a bound, per bound kind: f_z on lo0 / hi0, a tangential component on the
    zero bound of an upper-bounded row (f_t = +mu f_z) or of a lower-bounded row (f_t = -mu f_z), and swing legs (lo = hi = 0)."""
    f = np.asarray(u).reshape(len(u), -1, 4, 3)
    st = np.asarray(contact) != 0
    m = np.asarray(mu, dtype=f.dtype)[:, None, None]
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=f.dtype).reshape(-1, 1, 1), st.shape) for v in (lo, hi))
    cone = m * f[..., 2]
    return {"lo0": int((st & (f[..., 2] == lo)).sum()), "hi0": int((st & (f[..., 2] == hi)).sum()),
            "upper0": int((st & (cone > 0) & ((f[..., 0] == cone) | (f[..., 1] == cone))).sum()),
            "lower0": int((st & (cone > 0) & ((f[..., 0] == -cone) | (f[..., 1] == -cone))).sum()),
            "swing": int((~st & (f == 0).all(axis=-1)).sum()), "swing_legs": int((~st).sum())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)

    n10 = dict(N=N, delta=DELTA, io_dtype="f32", precision="mixed")
    over100 = lambda b, out: mpcqp.split_iters(out["iters"])[0].max() > 100

    def two_leg_hard(b, out):
        return bool((b["contact"].sum(axis=2) == 2).any()) and over100(b, out)
    s_low, b_low = first_seed(dict(n10, flags=P), lambda s: mpcqp.synth.make_batch(B, N, DELTA, s, ("trot",), (0.3,)), two_leg_hard)

    def one_and_three(b, out):
        n = np.unique(b["contact"].sum(axis=2))
        return 1 in n and 3 in n
    s_mix, b_mix = first_seed(dict(n10, flags=P), lambda s: mpcqp.synth.make_perleg_batch(B, N, DELTA, s), one_and_three)

    b7 = as_f32(mpcqp.synth.make_batch(B, N, DELTA, 7, GAITS, MUS))
    rows = mpcqp.synth.make_model_rows(B, f_min=(8.0, 12.0), f_max=(25.0, 40.0))
    cases = {   # kwargs, batches, model rows, chain, seed, the case whose inputs these are
        "lowmu": (dict(n10, flags=P), [b_low], None, False, s_low, None),
        "swingmix": (dict(n10, flags=P), [b_mix], None, False, s_mix, None),
        "fzbox": (dict(n10, flags=P), [b7], rows, False, 7, None),
        "admm_only": (dict(n10, flags=0), [b7], None, False, 7, "fzbox"),
        "warm": (dict(n10, flags=P, warm_start=True, warm_shift=True), [b7], None, True, 7, "fzbox"),
        "io64": (dict(N=N, delta=DELTA, io_dtype="f64", precision="mixed", flags=P), [b_low], None, False, s_low, "lowmu"),
    }
    for name, (kw, batches, models, chain, seed, inputs_of) in cases.items():
        ins, outs, box = solve(kw, batches, models, chain)
        data = {"commit": np.array(a.commit), "kwargs": np.array(json.dumps(kw)), "solves": np.array(len(outs)), "seed": np.array(seed),
                "box": np.array(box)}
        if models is not None:
            data["models"] = np.ascontiguousarray(models, dtype=np.float64)
        if inputs_of is not None:
            data["inputs_of"] = np.array(inputs_of)
        for i, (bi, oi) in enumerate(zip(ins, outs)):
            if i or inputs_of is None:
                data.update({f"in{i}_{k}": v for k, v in bi.items()})
            data.update({f"out{i}_{k}": v for k, v in oi.items() if not (chain and i == 0 and k == "X")})
        path = os.path.join(a.out, f"projection_identity_{name}.npz")
        np.savez_compressed(path, **data)
        admm, pol = mpcqp.split_iters(outs[-1]["iters"])
        st = outs[-1]["status"]
        lo, hi = (models[:, 4], models[:, 5]) if models is not None else (np.full(B, box[0]), np.full(B, box[1]))
        print(f"{name:10s} seed {seed} B {len(st)} solved {int(((st == 1) | (st == 2)).sum())} admm max {int(admm.max())} "
              f"mean {admm.mean():.1f} over-100 {int((admm > 100).sum())} polish max {int(pol.max())} "
              f"on bounds {bound_counts(outs[-1]['u'], ins[-1]['contact'], ins[-1]['mu'], lo, hi)} {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
