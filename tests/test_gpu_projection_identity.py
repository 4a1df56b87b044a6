"""Bitwise identity of solve_batch across the change of the ADMM row projection from fmin(fmax(t, lo), hi) to the median of the three
(csrc/mpcqp_leg.h: leg_clip) in the MIXED horizon-10 kernels.

The fixtures tests/golden/projection_identity_<case>.npz were recorded by tools/record_projection_identity.py at the commit each of
them names: inputs (fp32 values; a case may take its first solve's inputs from the case `inputs_of` names), the engine's keyword
arguments, model rows where set, and u / X / status / iters / res.  The engine built from this tree must return the same words.
Every case is 64 QPs at horizon 10 on the fp32 iteration tile, placed where a clamp can go wrong: friction rows active at mu = 0.3,
quads that mix swing legs (lo = hi = 0) with stance legs, a tight f_z box whose two ends are both hit, the ADMM iterate as the
output, a warm-started and shifted second tick, fp64 buffers.  (A QP with a non-finite input is answered with zeros before any
iteration -- w_setup's `bad`, held by tests/test_gpu_reference_horizon.py and tests/test_gpu_gaits.py -- and a non-finite warm-start
guess is dropped entry by entry (tests/test_gpu_warm_start.py): no output word of such a QP passes through a clamp of a non-finite t.)"""
import json
import os

import numpy as np
import pytest
import torch

import mpcqp
from conftest import GOLDEN

CASES = ("lowmu", "swingmix", "fzbox", "admm_only", "warm", "io64")
INPUTS, OUTPUTS = ("x0", "r", "contact", "xdes", "mu"), ("u", "X", "status", "iters", "res")


def load(case):
    return np.load(os.path.join(GOLDEN, f"projection_identity_{case}.npz"))


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


def on_bounds(fx, i=0):
    """Counts of leg-stages whose force ends the solve exactly on a bound, per bound kind (as tools/record_projection_identity.py prints them)."""
    ins = inputs(fx, i)
    u = fx[f"out{i}_u"]
    f = u.reshape(len(u), -1, 4, 3)
    st = ins["contact"] != 0
    box = fx["models"][:, 4:6] if "models" in fx.files else np.broadcast_to(fx["box"], (len(u), 2))
    lo, hi = (np.asarray(box[:, c], dtype=f.dtype)[:, None, None] for c in (0, 1))
    cone = np.asarray(ins["mu"], dtype=f.dtype)[:, None, None] * f[..., 2]
    return {"lo0": int((st & (f[..., 2] == lo)).sum()), "hi0": int((st & (f[..., 2] == hi)).sum()),
            "upper0": int((st & (cone > 0) & ((f[..., 0] == cone) | (f[..., 1] == cone))).sum()),
            "lower0": int((st & (cone > 0) & ((f[..., 0] == -cone) | (f[..., 1] == -cone))).sum()),
            "swing": int((~st & (f == 0).all(axis=-1)).sum()), "swing_legs": int((~st).sum())}


def test_some_leg_stage_ends_on_every_bound_kind():
    """lo0 / hi0 (the f_z box), the zero bound of an upper-bounded friction row (f_t = mu f_z) and of a lower-bounded one
    (f_t = -mu f_z), and swing legs (lo = hi = 0): each is where some leg-stage of the polished fixtures ends."""
    low, box, mix = on_bounds(load("lowmu")), on_bounds(load("fzbox")), on_bounds(load("swingmix"))
    assert low["upper0"] > 0 and low["lower0"] > 0 and low["lo0"] > 0
    assert box["lo0"] > 0 and box["hi0"] > 0
    assert mix["swing_legs"] > 0 and mix["swing"] == mix["swing_legs"]
    m = load("fzbox")["models"]
    assert (m[:, 5] - m[:, 4]).max() <= 32.0   # a tight box: the default is 3 .. 100 N


def test_the_fixtures_reach_what_they_are_for():
    low, mix = load("lowmu"), load("swingmix")
    assert (low["in0_mu"] == np.float32(0.3)).all() and (low["in0_contact"].sum(axis=2) == 2).any()
    assert mpcqp.split_iters(low["out0_iters"])[0].max() > 100          # a second round
    feet = mix["in0_contact"].sum(axis=2)
    assert (feet == 1).any() and (feet == 3).any()
    assert (mpcqp.split_iters(load("admm_only")["out0_iters"])[1] == 0).all()   # no polish: the iterate is the answer
    warm = load("warm")
    kw = json.loads(str(warm["kwargs"]))
    assert int(warm["solves"]) == 2 and kw["warm_start"] and kw["warm_shift"]
    io64 = load("io64")
    assert io64["out0_u"].dtype == np.float64 and str(io64["inputs_of"]) == "lowmu" and json.loads(str(io64["kwargs"]))["precision"] == "mixed"


def test_every_fixture_is_64_qps_solved_something_and_is_small():
    for case in CASES:
        fx = load(case)
        st = fx["out0_status"]
        assert st.shape == (64,) and json.loads(str(fx["kwargs"]))["N"] == 10, case
        assert ((st == 1) | (st == 2)).any(), case
        assert os.path.getsize(os.path.join(GOLDEN, f"projection_identity_{case}.npz")) <= 135000, case
