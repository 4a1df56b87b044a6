#!/usr/bin/env python3
"""Record the fixtures of the bitwise identity test of the operand-path trims of the MIXED horizon-10 solve:
tests/golden/trim_identity_<case>.npz.

Run ONCE, on the GPU, at the commit whose outputs are the contract (the parent of the change to rs8's first step, to the scale of
the fp32 sweep and to the index arithmetic of w_tile_init):

    python tools/record_trim_identity.py --commit $(git rev-parse HEAD) [--out tests/golden]

Layout and commit stamp are those of tools/record_projection_identity.py (inputs in fp32 / uint8, kwargs as JSON, `inputs_of`,
`models`, `box`, u / X / status / iters / res of every solve; the warm case stores the second tick's inputs and, of the first tick,
everything but X), every file of 64 QPs under 135 KB.

Every case is N = 10, B = 64, MIXED.  None of the three changes touches an operand's value, so a wrong word can only come from a
wrong lane, slot or mask -- the cases put every kind of E block and every build / sweep path through them:
  perleg      per-leg timing, all 16 support patterns among the stages, one- and three-foot stages: E blocks of every rank pass
              through the run masks of the build (fp32 and fp64 tile)
  tworound    trot at mu = 0.3, two-foot support, a QP with more than 100 ADMM iterations: a second round, i.e. two builds and two
              sweeps per QP and several hundred mat-vecs through the reduce-scatter
  models      model rows set: the other pair of kernel instantiations
  io64        the tworound batch through MIXED with fp64 buffers
  warm        warm start plus shift, two consecutive control ticks
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
from record_accel_identity import GAITS, MUS  # noqa: E402
from record_projection_identity import B, DELTA, N, P, as_f32, first_seed, solve  # noqa: E402


def patterns(contact):
    """The support patterns among the stages of a batch, as 4-bit codes (bit l: leg l in stance)."""
    return np.unique((np.asarray(contact) != 0).astype(np.int64) @ (1 << np.arange(4)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)

    n10 = dict(N=N, delta=DELTA, io_dtype="f32", precision="mixed")

    def every_pattern(b, out):
        return len(patterns(b["contact"])) == 16
    s_leg, b_leg = first_seed(dict(n10, flags=P), lambda s: mpcqp.synth.make_perleg_batch(B, N, DELTA, s), every_pattern)

    def two_rounds(b, out):
        return bool((b["contact"].sum(axis=2) == 2).any()) and mpcqp.split_iters(out["iters"])[0].max() > 100
    s_two, b_two = first_seed(dict(n10, flags=P), lambda s: mpcqp.synth.make_batch(B, N, DELTA, s, ("trot",), (0.3,)), two_rounds)

    b7 = as_f32(mpcqp.synth.make_batch(B, N, DELTA, 7, GAITS, MUS))
    rows = mpcqp.synth.make_model_rows(B)
    cases = {   # kwargs, batches, model rows, chain, seed, the case whose inputs these are
        "perleg": (dict(n10, flags=P), [b_leg], None, False, s_leg, None),
        "tworound": (dict(n10, flags=P), [b_two], None, False, s_two, None),
        "models": (dict(n10, flags=P), [b7], rows, False, 7, None),
        "io64": (dict(N=N, delta=DELTA, io_dtype="f64", precision="mixed", flags=P), [b_two], None, False, s_two, "tworound"),
        "warm": (dict(n10, flags=P, warm_start=True, warm_shift=True), [b7], None, True, 7, "models"),
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
        path = os.path.join(a.out, f"trim_identity_{name}.npz")
        np.savez_compressed(path, **data)
        admm, pol = mpcqp.split_iters(outs[-1]["iters"])
        st = outs[-1]["status"]
        feet = np.unique(ins[-1]["contact"].sum(axis=2))
        print(f"{name:10s} seed {seed} B {len(st)} solved {int(((st == 1) | (st == 2)).sum())} admm max {int(admm.max())} "
              f"mean {admm.mean():.1f} over-100 {int((admm > 100).sum())} polish max {int(pol.max())} patterns {len(patterns(ins[-1]['contact']))} "
              f"feet {feet.tolist()} {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
