"""The `iters` output (include/mpcqp.h, MPCQP_ITERS) and the swing-leg lever arms on the CPU checker -- no GPU needed.

`iters` packs ADMM iterations and polish steps.  The old `admm + 1000 * polish` read 1200 ADMM iterations as 200 + one polish
step; values of 1000 ADMM iterations or more now use a range of their own (>= 1e6), decoded by mpcqp.split_iters.
"""
import ctypes

import numpy as np
import pytest

import mpcqp

WIDE = 1000000


def encode(admm, polish):
    """MPCQP_ITERS, restated."""
    if admm < 1000 and polish < 1000:
        return admm + 1000 * polish
    return WIDE * (min(polish, 2145) + 1) + admm


EDGES = [(0, 0), (1, 0), (0, 1), (999, 0), (0, 999), (999, 999), (1000, 0), (0, 1000), (999, 1000), (1000, 999), (1200, 0),
         (1200, 1), (999999, 0), (0, 2145), (999999, 2145)]


@pytest.mark.parametrize("admm,polish", EDGES)
def test_split_iters_round_trip(admm, polish):
    v = encode(admm, polish)
    assert 0 <= v <= 2**31 - 1
    assert mpcqp.split_iters(v) == (admm, polish)
    a, p = mpcqp.split_iters(np.array([v, v], np.int32))
    assert a.tolist() == [admm, admm] and p.tolist() == [polish, polish]


def test_split_iters_keeps_the_narrow_values():
    """Below 1000 / 1000 the value is what it always was (bench.py's N = 10 decode at a cap of 400 keeps its meaning)."""
    for admm, polish in ((0, 0), (400, 3), (999, 999), (37, 12)):
        assert encode(admm, polish) == admm + 1000 * polish
    assert mpcqp.split_iters(1200) == (200, 1)          # a narrow value: 200 iterations and one polish step
    assert mpcqp.split_iters(1001200) == (1200, 0)      # 1200 iterations, no polish


def test_split_iters_clamps_polish_and_is_elementwise():
    assert mpcqp.split_iters(encode(5, 3000)) == (5, 2145)
    v = np.array([[encode(a, p) for a, p in EDGES[:5]], [encode(a, p) for a, p in EDGES[5:10]]])
    a, p = mpcqp.split_iters(v)
    assert a.shape == p.shape == (2, 5)
    assert [(int(x), int(y)) for x, y in zip(a.ravel(), p.ravel())] == EDGES[:10]


@pytest.mark.parametrize("N", [10, 60])
def test_checker_past_1000_iterations(oracle_lib, N):
    """Polish off, eps 0, max_iter = check_every = 1200: the checker runs exactly 1200 ADMM iterations and reports (1200, 0) --
    the old encoding returned 1200, i.e. (200, 1)."""
    b = mpcqp.synth.make_batch(2, N, 0.03, 11, ("trot", "gallop"), (0.5, 1.0))
    cfg = oracle_lib.default_config(N=N, delta=0.03, flags=0, eps_abs=0.0, eps_rel=0.0, max_iter=1200, check_every=1200)
    out = mpcqp.Engine(oracle_lib, cfg).solve_batch_host(b["x0"], b["r"], b["contact"], b["xdes"], b["mu"])
    assert np.all(out["status"] == mpcqp._capi.STATUS_MAX_ITER), out["status"]
    assert out["iters"].tolist() == [WIDE + 1200] * 2
    admm, polish = mpcqp.split_iters(out["iters"])
    assert admm.tolist() == [1200, 1200] and polish.tolist() == [0, 0]


def test_checker_rejects_caps_that_do_not_fit(oracle_lib):
    for bad in (0, WIDE, WIDE + 1, 2**31 - 1):
        cfg = oracle_lib.default_config(max_iter=bad)
        h = ctypes.c_void_p()
        assert oracle_lib.lib.mpcqp_create(ctypes.byref(cfg), ctypes.byref(h)) == -1, bad
    mpcqp.Engine(oracle_lib, oracle_lib.default_config(max_iter=WIDE - 1)).close()


def swing_twins(base, values, seed=0):
    """Each QP of `base` followed by one twin per entry of `values`; the first copy has its swing-leg lever arms set to 0, each twin
    to the value ("rand": uniform finite values in [-5, 5]).  Swing forces are pinned to zero (src/mpc.py:138-144), so a swing leg's
    lever arm cannot change the optimum: every twin must return what the first copy returns."""
    rng = np.random.default_rng(seed)
    B = len(base["x0"])
    T = 1 + len(values)
    b = {k: np.repeat(base[k], T, axis=0) for k in ("x0", "r", "contact", "xdes", "mu")}
    swing = np.repeat((b["contact"] == 0)[..., None], 3, axis=-1)
    for i, v in enumerate([0.0] + list(values)):
        r = b["r"][i::T]
        sw = swing[i::T]
        r[sw] = rng.uniform(-5.0, 5.0, int(sw.sum())) if v == "rand" else v
    assert np.isfinite(b["r"]).all() and swing.any()
    return b, B, T


def test_checker_swing_lever_arms_are_dont_care(oracle_solve):
    base = mpcqp.synth.config3(12)
    b, B, T = swing_twins(base, ["rand", 1e30, 1e308, -1e308])
    out = oracle_solve(b)
    assert np.all(out["status"] == 1)
    for k in ("status", "iters", "u", "X", "res"):
        a = out[k].reshape(B, T, -1)
        for j in range(1, T):
            assert np.array_equal(a[:, 0].view(np.uint8), a[:, j].view(np.uint8)), (k, j)
