"""Bitwise identity of solve_batch across a change of the Anderson step (csrc/mpcqp_leg.h: w_aa_step).

The fixtures tests/golden/accel_identity_<case>.npz were recorded by tools/record_accel_identity.py at the commit each of them names
(`commit`): the inputs of every solve in the engine's io dtype, the engine's keyword arguments, and u / X / status / iters / res of
every solve.  The engine built from this tree must return the same bits.  The cases are the smallest that reach every path an
extrapolation runs on: one wave per QP (listed and natural order), four waves with the history parked in LDS, the stage-wise engine
with a one-level and a two-level chain, a warm-started pair of solves (short first block), and an ADMM-only run (no acceleration)."""
import json
import os

import numpy as np
import pytest
import torch

import mpcqp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = ("n10_mixed", "n10_natural", "n20_mixed", "n10_stage", "n24_stage", "n10_warm", "n10_admm_only")
INPUTS, OUTPUTS = ("x0", "r", "contact", "xdes", "mu"), ("u", "X", "status", "iters", "res")


def load(case):
    return np.load(os.path.join(GOLDEN, f"accel_identity_{case}.npz"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@pytest.mark.parametrize("case", CASES)
def test_outputs_are_the_recorded_bits(case):
    fx = load(case)
    assert len(str(fx["commit"])) == 40
    sol = mpcqp.MPCBatch(device=0, **json.loads(str(fx["kwargs"])))
    for i in range(int(fx["solves"])):   # on ONE engine, in order: the second solve of the warm case starts from the first one's answer
        dev = sol.upload({k: fx[f"in{i}_{k}"] for k in INPUTS})
        out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True)
        torch.cuda.synchronize()
        for k in OUTPUTS:
            got, want = out[k].cpu().numpy(), fx[f"out{i}_{k}"]
            assert got.dtype == want.dtype and got.shape == want.shape, (case, i, k)
            diff = bits(got) != bits(want)
            assert not diff.any(), f"{case} solve {i} {k}: {int(diff.sum())} of {diff.size} words differ, first at {np.argwhere(diff)[0].tolist()}"


def test_the_headline_fixture_reaches_second_rounds_and_low_friction_double_support():
    """The N = 10 MIXED batch must exercise several extrapolations, a second round (a block is at most 100 iterations) and two-legged
    support at mu = 0.3; the natural-order case is the same batch."""
    fx, nat = load("n10_mixed"), load("n10_natural")
    admm = mpcqp.split_iters(fx["out0_iters"])[0]
    assert (fx["out0_iters"] % 1000).max() > 100
    assert int((admm > 100).sum()) >= 1
    two_legs = (fx["in0_contact"].sum(axis=2) == 2).any(axis=1)
    assert (two_legs & (fx["in0_mu"] == np.float32(0.3))).any()
    assert fx["in0_x0"].shape[0] == 96 and all(np.array_equal(fx[f"in0_{k}"], nat[f"in0_{k}"]) for k in INPUTS)


def test_the_admm_only_fixture_ran_no_polish():
    assert (mpcqp.split_iters(load("n10_admm_only")["out0_iters"])[1] == 0).all()
