"""Bitwise identity of solve_batch across the three operand-path trims of the MIXED horizon-10 kernels (csrc/mpcqp_wrench.h: W_TRIM_RS8,
W_TRIM_PKMUL, W_TRIM_ROWTAB): the reduce-scatter's first step on DPP write masks, the packed scale of the fp32 sweep's pivot row, and
the tile builds from the lane-order row table.  None of them changes an operand's value or the order of a sum, so every output word
is the parent's.

The fixtures tests/golden/trim_identity_<case>.npz were recorded by tools/record_trim_identity.py at the commit each of them names
(the parent of the change): inputs (fp32 values; a case may take its first solve's inputs from the case `inputs_of` names), the
engine's keyword arguments, model rows where set, and u / X / status / iters / res.  The engine built from this tree must return the
same words.  Every case is 64 QPs at horizon 10 on the fp32 iteration tile, placed where a wrong lane, slot or mask would show: per-leg
timing with all 16 support patterns (E blocks of every rank through the build masks), two-foot support at mu = 0.3 with second
rounds (two builds and sweeps per QP), model rows, fp64 buffers, a warm-started and shifted second tick."""
import json
import os

import numpy as np
import pytest
import torch

import mpcqp
from conftest import GOLDEN

CASES = ("perleg", "tworound", "models", "io64", "warm")
INPUTS, OUTPUTS = ("x0", "r", "contact", "xdes", "mu"), ("u", "X", "status", "iters", "res")


def load(case):
    return np.load(os.path.join(GOLDEN, f"trim_identity_{case}.npz"))


def inputs(fx, i):
    """Inputs of solve i: the fixture's own, or (first solve) those of the case it names."""
    src = fx if f"in{i}_x0" in fx.files else load(str(fx["inputs_of"]))
    return {k: src[f"in{i}_{k}"] for k in INPUTS}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_outputs_are_the_recorded_bits(case):
    fx = load(case)
    assert len(str(fx["commit"])) == 40
    sol = mpcqp.MPCBatch(device=0, **json.loads(str(fx["kwargs"])))
    if "models" in fx.files:
        sol.set_models(fx["models"])
    compared = 0
    for i in range(int(fx["solves"])):   # on ONE engine, in order: the second tick of the warm case starts from the first one's answer
        dev = sol.upload(inputs(fx, i))
        out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True)
        torch.cuda.synchronize()
        for k in OUTPUTS:
            if f"out{i}_{k}" not in fx.files:   # (X of the warm case's first tick: not stored)
                continue
            got, want = out[k].cpu().numpy(), fx[f"out{i}_{k}"]
            assert got.dtype == want.dtype and got.shape == want.shape, (case, i, k)
            diff = bits(got) != bits(want)
            assert not diff.any(), f"{case} solve {i} {k}: {int(diff.sum())} of {diff.size} words differ, first at {np.argwhere(diff)[0].tolist()}"
            compared += 1
    assert compared == {"warm": 9}.get(case, 5)


def test_the_fixtures_reach_what_they_are_for():
    leg, two = load("perleg"), load("tworound")
    c = leg["in0_contact"] != 0
    assert len(np.unique(c.astype(np.int64) @ (1 << np.arange(4)))) == 16   # every support pattern among the stages
    feet = c.sum(axis=2)
    assert (feet == 1).any() and (feet == 3).any()
    assert (two["in0_mu"] == np.float32(0.3)).all() and (two["in0_contact"].sum(axis=2) == 2).any()
    assert mpcqp.split_iters(two["out0_iters"])[0].max() > 100          # a second round: two builds and sweeps
    assert mpcqp.split_iters(leg["out0_iters"])[0].max() > 100
    for case in ("perleg", "tworound", "models"):                       # the polish ran: the fp64 tile was built from the table too
        assert mpcqp.split_iters(load(case)["out0_iters"])[1].max() > 0, case
    models = load("models")["models"]
    assert models.shape == (64, 6) and len(np.unique(models, axis=0)) > 1
    io64 = load("io64")
    assert io64["out0_u"].dtype == np.float64 and str(io64["inputs_of"]) == "tworound" and json.loads(str(io64["kwargs"]))["precision"] == "mixed"
    warm = load("warm")
    kw = json.loads(str(warm["kwargs"]))
    assert int(warm["solves"]) == 2 and kw["warm_start"] and kw["warm_shift"] and "out0_X" not in warm.files and "in1_x0" in warm.files


def test_every_fixture_is_64_qps_mixed_at_horizon_10_solved_and_small():
    commits = set()
    for case in CASES:
        fx = load(case)
        st, kw = fx["out0_status"], json.loads(str(fx["kwargs"]))
        assert st.shape == (64,) and kw["N"] == 10 and kw["precision"] == "mixed", case
        assert ((st == 1) | (st == 2)).all(), case
        assert os.path.getsize(os.path.join(GOLDEN, f"trim_identity_{case}.npz")) <= 135000, case
        commits.add(str(fx["commit"]))
    assert len(commits) == 1   # one recording, at one commit
