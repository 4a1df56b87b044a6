"""Whole-batch accounting of one engine output (a helper module of the suite, not a conftest).

`check_batch` holds EVERY QP of a batch to the status contract of include/mpcqp.h, not only the ones the engine reports solved:

* status is one of SOLVED_POLISHED (1), SOLVED_ADMM (2), MAX_ITER (3), NONFINITE (-1) -- never UNSOLVED (0);
* -1 exactly where an input of the QP is non-finite, and its outputs are exactly zero;
* solved QPs meet the parity band against the checker's answer (1e-4 relative on the forces, 1e-4 absolute on the states);
* MAX_ITER QPs return finite forces and states, exactly zero force on every swing leg, and an ADMM count equal to the cap
  (the cap is exact; with a regulariser continuation, alpha < 1e-2, at most the cap);
* at most `allowed` QPs with finite inputs are not solved.  The engine is bitwise deterministic, so `allowed` is the exact count
  measured on an MI355X, written into each test: a regression that sends a few QPs to the cap fails it.
"""
import numpy as np

import mpcqp
from conftest import rel_err

STATUSES = (1, 2, 3, -1)


def _np(a):
    if a is None:
        return None
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def finite_inputs(batch):
    """Per QP: every entry of x0, r, xdes and mu is finite."""
    B = len(batch["x0"])
    ok = np.ones(B, bool)
    for k in ("x0", "r", "xdes", "mu"):
        ok &= np.isfinite(np.asarray(batch[k], np.float64).reshape(B, -1)).all(axis=1)
    return ok


def check_batch(out, batch, ref=None, *, max_iter, allowed=0, tol=1e-4, x_tol=1e-4, cap_exact=True, what=""):
    """Assert the contract above for every QP of `out` (engine outputs, numpy or torch) solved from `batch` (mpcqp.synth layout:
    x0, r, contact, xdes, mu); `ref` is the checker's answer of the same batch, or None where the caller compares something else.
    `cap_exact=False` where alpha < 1e-2: a regulariser continuation that cannot reach its next level within three bisected steps
    ends with MAX_ITER before the cap, so the ADMM count is only bounded by it.  Returns the mask of the solved QPs."""
    st = _np(out["status"])
    u = _np(out["u"]).astype(np.float64)
    X = _np(out.get("X"))
    it = _np(out["iters"])
    B = len(st)
    N = u.shape[1]
    assert u.shape == (B, N, 12), (what, u.shape)
    bad = set(np.unique(st).tolist()) - set(STATUSES)
    assert not bad, f"{what}: status values {sorted(bad)} outside {STATUSES}"
    fin = finite_inputs(batch)
    nonfin = st == -1
    assert np.array_equal(nonfin, ~fin), f"{what}: status -1 at {np.nonzero(nonfin)[0].tolist()}, non-finite inputs at {np.nonzero(~fin)[0].tolist()}"
    assert np.all(u[nonfin] == 0), what
    if X is not None:
        X = X.astype(np.float64)
        assert np.all(X[nonfin] == 0), what
    ok = (st == 1) | (st == 2)
    if ref is not None and ok.any():
        e = rel_err(u, ref["u"])[ok]
        assert e.max() <= tol, f"{what}: solved QP {np.nonzero(ok)[0][e.argmax()]} force error {e.max():.3e} > {tol:g}"
        if X is not None and ref.get("X") is not None:
            eX = np.abs(X[ok] - np.asarray(ref["X"], np.float64)[ok]).max()
            assert eX <= x_tol, f"{what}: solved QP state error {eX:.3e} > {x_tol:g}"
    cap = st == 3
    if cap.any():
        assert np.isfinite(u[cap]).all(), what
        if X is not None:
            assert np.isfinite(X[cap]).all(), what
        swing = np.repeat(np.asarray(batch["contact"]) == 0, 3, axis=2).reshape(B, N, 12)
        assert np.all(u[cap][swing[cap]] == 0), f"{what}: MAX_ITER QP with force on a swing leg"
        admm = mpcqp.split_iters(it[cap])[0]
        assert np.all(admm == max_iter) if cap_exact else np.all(admm <= max_iter), f"{what}: MAX_ITER QPs report ADMM counts {np.unique(admm).tolist()}, cap {max_iter}"
    n = int((fin & ~ok).sum())
    assert n <= allowed, f"{what}: {n} QPs with finite inputs not solved (allowed {allowed}): {np.nonzero(fin & ~ok)[0].tolist()[:20]}"
    return ok


def kkt_certificate(H, g, G, lo, hi, u, act_tol=1e-7):
    """Optimality certificate of `u` for the convex QP min 1/2 u'Hu + g'u s.t. lo <= Gu <= hi (oracle/qp_spec.py layout).

    Multipliers come from a SIGN-CONSTRAINED least-squares fit on the active rows (y >= 0 on rows at their upper bound, y <= 0 at
    their lower bound, free on equality rows), then qp_spec.kkt_report gives stationarity, primal feasibility, dual sign and
    complementarity: stationarity with multipliers of the right sign IS optimality of the convex QP -- an unconstrained fit would
    certify stationary points of the wrong active set too.  A row is active within `act_tol` relative to its bound."""
    from scipy.optimize import lsq_linear
    import qp_spec as S
    Gu = G @ u
    lo0, hi0 = np.where(np.isfinite(lo), lo, 0.0), np.where(np.isfinite(hi), hi, 0.0)
    at_lo = np.isfinite(lo) & (np.abs(Gu - lo0) <= act_tol * np.maximum(1, np.abs(lo0)))
    at_hi = np.isfinite(hi) & (np.abs(Gu - hi0) <= act_tol * np.maximum(1, np.abs(hi0)))
    act = at_lo | at_hi
    y = np.zeros(len(lo))
    if act.any():
        lb = np.where(at_lo[act], -np.inf, 0.0)
        ub = np.where(at_hi[act], np.inf, 0.0)
        fit = lsq_linear(G[act].T, -(H @ u + g), bounds=(lb, ub), method="bvls", tol=1e-14, max_iter=2000)
        y[act] = fit.x
    return S.kkt_report(H, g, G, lo, hi, u, y)
