"""What the parity tests used to skip: QPs the engine reports unsolved, the `iters` count past 1000 ADMM iterations, the `res`
output, and swing-leg lever arms (inputs the optimum does not depend on)."""
import ctypes

import numpy as np
import pytest
import torch

import mpcqp
import qp_spec as S
from batch_checks import check_batch
from conftest import rel_err
from test_gpu_parity import gpu_solve
from test_iters_encoding import WIDE, swing_twins

pytestmark = pytest.mark.gpu
G, M = ("trot", "pronk", "amble", "gallop"), (0.3, 0.5, 0.7, 1.0)


def _subset(b, idx):
    return {k: b[k][idx] for k in ("x0", "r", "contact", "xdes", "mu")}


# (N, seed, io, QPs at the cap, force band, state band) -- default configuration, mixed distribution, 4096 QPs; counts and errors
# measured on an MI355X (the engine is bitwise deterministic).  At N = 10 the cap's iterate is within 2 % of the checker's forces;
# its states can be further off (seed 91: 0.22), and at N = 20 the forces are 17-33 % off.
CAP_BATCHES = [
    (10, 26, "f64", 1, 0.1, 1e-2),    # measured: forces 2.0e-2, states 1.3e-4
    (10, 51, "f32", 1, 0.1, 1e-2),    # measured: forces 2.3e-3, states 4.5e-4
    (10, 91, "f32", 1, 0.1, 0.5),     # measured: forces 1.5e-2, states 0.22
    (20, 18, "f64", 1, 0.5, 6.0),     # measured: forces 0.33, states 4.4
]


@pytest.mark.parametrize("N,seed,io,count,ftol,xtol", CAP_BATCHES)
def test_max_iter_band(oracle_solve, N, seed, io, count, ftol, xtol):
    """Default-config batches that leave QPs at the iteration cap: exactly `count` of them, each one the checker solves, returned
    with finite forces and states, zero swing forces, the exact cap, and within the stated band of the checker's optimum."""
    b = mpcqp.synth.make_batch(4096, N, 0.03, seed, G, M)
    out = gpu_solve(b, N=N, io=io, precision="mixed")
    check_batch(out, b, None, max_iter=out["max_iter"], allowed=count, what=f"N={N} seed {seed} {io}")
    cap = np.nonzero(out["status"] == 3)[0]
    assert len(cap) == count and np.all(out["status"] != 2)
    ref = oracle_solve(_subset(b, cap), N=N)
    assert np.all(ref["status"] == 1)
    ef = rel_err(out["u"][cap], ref["u"])
    eX = np.abs(out["X"][cap].astype(np.float64) - ref["X"]).max(axis=(1, 2))
    assert ef.max() <= ftol and eX.max() <= xtol, (ef, eX)


@pytest.mark.parametrize("max_iter,count", [(40, 268), (60, 115)])
def test_reduced_cap_accounting(max_iter, count):
    """A cap inside the first ADMM block (60 iterations at N = 10): many QPs end at it, every one of them with the structural
    properties of batch_checks (finite, zero swing forces, ADMM count == cap); the count is the measured one."""
    b = mpcqp.synth.config3(4096)
    out = gpu_solve(b, io="f32", precision="mixed", max_iter=max_iter)
    check_batch(out, b, None, max_iter=max_iter, allowed=count, what=f"max_iter={max_iter}")
    assert int((out["status"] == 3).sum()) == count >= 20


# The polish acceptance of the dense engine (mpcqp_wrench.h, the KKT check of a polish step; TV = double on every path), at the
# default alpha = 1e-2 and uscale = max(1, |u|_inf):
#   primal violation    viol[0] <= ftol * uscale,                          ftol = 1e-7
#   dual sign / station max(viol[1], stat) <= 2 alpha * 2e-5 * uscale      (the curvature-scaled bound `a2f * 2e-5f * uscale`)
# and res = (viol[0], max(viol[1], stat)) of the accepted step.
FTOL, DUAL_SCALE = 1e-7, 2e-5


@pytest.mark.parametrize("which,io", [("config2", "f32"), ("config2", "f64"), ("config3", "f32")])
def test_res_is_honest(which, io):
    """For every polished QP: res is under the acceptance threshold, and the constraint violation of the returned u, recomputed
    in fp64 from qp_spec's rows (box, friction pyramid, swing), is at most res[:, 0] plus the rounding of the output dtype."""
    b = mpcqp.synth.config2(1024) if which == "config2" else mpcqp.synth.config3(512)
    out = gpu_solve(b, io=io, precision="mixed")
    cfg = S.QPConfig(N=10, delta=0.03, alpha=1e-2)
    pol = np.nonzero(out["status"] == 1)[0]
    assert len(pol) == len(b["mu"])
    u = out["u"].astype(np.float64).reshape(len(b["mu"]), -1)
    res = out["res"].astype(np.float64)
    uscale = np.maximum(1.0, np.abs(u).max(axis=1)) * (1 + 1e-6)
    assert np.all(res[pol, 0] <= FTOL * uscale[pol]), (res[:, 0] / uscale).max()
    assert np.all(res[pol, 1] <= 2 * cfg.alpha * DUAL_SCALE * uscale[pol]), (res[:, 1] / uscale).max()
    eps = np.finfo(np.float32 if io == "f32" else np.float64).eps
    for i in pol:
        _, _, _, Gm, lo, hi, _, _ = S.condensed_qp(b["x0"][i], b["r"][i], b["contact"][i], b["xdes"][i], float(b["mu"][i]), cfg)
        gu = Gm @ u[i]
        viol = max(0.0, float(np.max(np.maximum(lo - gu, gu - hi))))
        rounding = (1 + float(b["mu"][i])) * np.abs(u[i]).max() * eps
        assert viol <= res[i, 0] + rounding, (i, viol, res[i, 0], rounding)


def test_admm_iterate_past_1000_iterations(oracle_lib):
    """test_admm_iterate_is_the_oracles_osqp_iterate at K = 1200 (polish off, eps 0): both engines report (1200, 0) -- the old
    encoding read that as 200 iterations and one polish step -- and the all-fp64 dense engine still follows the checker's iterate."""
    kw = dict(flags=0, eps_abs=0.0, eps_rel=0.0, max_iter=1200, check_every=1200)
    b = mpcqp.synth.config3(64)
    ref = mpcqp.Engine(oracle_lib, oracle_lib.default_config(N=10, delta=0.03, **kw)).solve_batch_host(
        b["x0"], b["r"], b["contact"], b["xdes"], b["mu"])
    assert np.all(ref["iters"] == WIDE + 1200)
    out = gpu_solve(b, N=10, io="f64", precision="f64", adapt_thr=1e30, **kw)   # (no early rho change at iteration 25: the checker has none)
    assert np.all(out["iters"] == WIDE + 1200) and np.all((out["status"] == 3) | (out["status"] == 2))
    assert mpcqp.split_iters(out["iters"])[0].tolist() == [1200] * 64
    e = rel_err(out["u"], ref["u"]).max()
    assert e <= 1e-6, e
    # the stage-wise engine at the reference's horizon
    b60 = mpcqp.synth.make_batch(8, 60, 0.03, 11, ("trot", "gallop"), (0.5, 1.0))
    o60 = gpu_solve(b60, N=60, io="f64", precision="f64", **dict(kw, flags=mpcqp.FLAG_STAGE_KERNEL))
    assert np.all(o60["iters"] == WIDE + 1200) and np.all((o60["status"] == 3) | (o60["status"] == 2))
    # and caps that do not fit the encoding are refused
    lib = mpcqp.product_library()
    for bad in (WIDE, 2**31 - 1):
        h = ctypes.c_void_p()
        assert lib.lib.mpcqp_create(ctypes.byref(lib.default_config(max_iter=bad)), ctypes.byref(h)) == -1


def _gait60(B):
    g = mpcqp.synth.make_gait_batch(B, N=60, delta=0.01, steps=5, seed=3, gait_names=("trot", "gallop"), mus=(0.7, 1.0))
    return mpcqp.synth.expand_gait_batch(g, N=60, delta=0.01)


@pytest.mark.parametrize("N,io", [(10, "f64"), (10, "f32"), (20, "f64"), (20, "f32"), (60, "f64"), (60, "f32")])
def test_swing_lever_arms_are_dont_care(N, io):
    """Each QP next to twins whose swing-leg lever arms are random finite values, 1e30 and the largest finite magnitudes of the I/O
    type: every twin returns the bits of the copy with zero swing lever arms (status, iters, u, X, res).  The engines once masked
    the swing columns of B by multiplying with 0, and 0 x inf (a lever arm of 1e308 times 1 / 0.24) put NaN into B."""
    big = 1e308 if io == "f64" else 3e38
    base = mpcqp.synth.make_batch(8, N, 0.03, 20250830 + N, G, M) if N != 60 else _gait60(8)
    b, B, T = swing_twins(base, ["rand", 1e30, big, -big], seed=N)
    delta = 0.03 if N != 60 else 0.01
    out = gpu_solve(b, N=N, delta=delta, io=io, precision="mixed")
    for k in ("status", "iters", "u", "X", "res"):
        a = np.ascontiguousarray(out[k]).reshape(B, T, -1)
        for j in range(1, T):
            assert np.array_equal(a[:, 0].view(np.uint8), a[:, j].view(np.uint8)), (k, j, out["status"].reshape(B, T).tolist())
    check_batch({k: out[k][0::T] for k in ("u", "X", "status", "iters")}, {k: b[k][0::T] for k in b}, None,
                max_iter=out["max_iter"], allowed=0, what=f"twins N={N} {io}")
