"""Bitwise identity of solve_batch across the change from the dense 3 x 6 leg map to the structured maps (csrc/mpcqp_legmap.h).

The fixtures tests/golden/legmap_identity_<case>.npz were recorded by tools/record_legmap_identity.py at the commit each of them
names, in the layout of the accel_identity fixtures (tests/test_gpu_accel_identity.py), plus the model rows where a case sets them.
The engine built from this tree must return the same words.  The cases reach the instantiations the accel_identity cases do not:
per-leg timing (quads that mix swing and stance legs), all-fp64, MIXED with fp64 buffers, per-robot model rows, the alpha = 0
continuation, the refinement kernel, horizon 20 in fp64 and the stage-wise engine at N = 60."""
import json
import os

import numpy as np
import pytest
import torch

import mpcqp
from conftest import GOLDEN

CASES = ("n10_perleg", "n10_f64", "n10_io64", "n10_models", "n10_alpha0", "n10_refine", "n20_f64", "n60_stage")
INPUTS, OUTPUTS = ("x0", "r", "contact", "xdes", "mu"), ("u", "X", "status", "iters", "res")


def load(case):
    return np.load(os.path.join(GOLDEN, f"legmap_identity_{case}.npz"))


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
    dev = sol.upload({k: fx[f"in0_{k}"] for k in INPUTS})
    out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True)
    torch.cuda.synchronize()
    for k in OUTPUTS:
        got, want = out[k].cpu().numpy(), fx[f"out0_{k}"]
        assert got.dtype == want.dtype and got.shape == want.shape, (case, k)
        diff = bits(got) != bits(want)
        assert not diff.any(), f"{case} {k}: {int(diff.sum())} of {diff.size} words differ, first at {np.argwhere(diff)[0].tolist()}"


def test_the_perleg_fixture_mixes_swing_and_stance_and_reaches_a_second_round():
    """Stages with one and with three stance feet (quads that mix swing and stance legs) and a QP with more than 100 ADMM iterations."""
    fx = load("n10_perleg")
    feet = fx["in0_contact"].sum(axis=2)
    assert (feet == 1).any() and (feet == 3).any()
    assert fx["in0_x0"].shape[0] == 64 and mpcqp.split_iters(fx["out0_iters"])[0].max() > 100


def test_the_alpha0_fixture_takes_more_than_one_polish_step():
    assert mpcqp.split_iters(load("n10_alpha0")["out0_iters"])[1].max() > 1


def test_the_model_fixture_has_rows_that_differ():
    m = load("n10_models")["models"]
    assert m.shape == (32, 6) and all(len(np.unique(m[:, c])) > 1 for c in (0, 1, 4, 5))


def test_every_fixture_solved_something_and_is_small():
    for case in CASES:
        st = load(case)["out0_status"]
        assert ((st == 1) | (st == 2)).any(), case
        assert os.path.getsize(os.path.join(GOLDEN, f"legmap_identity_{case}.npz")) <= 135000, case
