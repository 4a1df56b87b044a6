"""Inputs the two-beat gaits never produce, on the CPU checker: one- and three-foot support (crawl patterns, per-leg timing), friction
from 0.05 to 3 and exactly 0, force bounds at their edges, and primal-infeasible QPs (mu < 0 with a stance leg).

These tests pin the generators (the batches really contain what the GPU tests in tests/test_gpu_support_patterns.py claim to cover)
and certify the checker's answers with the KKT certificate of tests/batch_checks.py before the GPU tests trust them.
"""
import numpy as np
import pytest

import mpcqp
import qp_spec as S
from batch_checks import kkt_certificate

SY = mpcqp.synth


def _support_counts(contact):
    """Fraction of stages with 0..4 stance legs, and the set of 4-leg patterns that occur."""
    n = np.asarray(contact).sum(axis=-1).ravel()
    return np.bincount(n, minlength=5) / n.size, set(map(tuple, np.asarray(contact).reshape(-1, 4).tolist()))


def _certify(b, ref, idx, N, delta, alpha=1e-2, f_min=3.0, f_max=100.0):
    """The thresholds of tests/test_oracle_pinning.py::test_c_oracle_matches_numpy_restatement_and_kkt, QP by QP."""
    cfg = S.QPConfig(N=N, delta=delta, alpha=alpha, f_min=f_min, f_max=f_max)
    for i in idx:
        H, g, c0, G, lo, hi, *_ = S.condensed_qp(b["x0"][i], b["r"][i], b["contact"][i], b["xdes"][i], b["mu"][i], cfg)
        u = ref["u"][i].reshape(-1)
        k = kkt_certificate(H, g, G, lo, hi, u)
        scale = max(1.0, np.abs(g).max())
        assert k["stationarity"] <= 1e-7 * scale, (i, k)
        assert k["primal"] <= 1e-7 * max(1.0, np.abs(u).max()), (i, k)
        assert k["dual_sign"] <= 1e-9 * scale, (i, k)
        assert k["complementarity"] <= 1e-6 * scale, (i, k)
        assert np.abs(S.predict_states(b["x0"][i], u, b["r"][i], b["contact"][i], cfg) - ref["X"][i]).max() <= 1e-10


# ---------------------------------------------------------------------------------------------------------------- vacuity guards
@pytest.mark.parametrize("N,delta,B", [(10, 0.03, 512), (20, 0.03, 128), (33, 0.03, 48), (60, 0.01, 48)])
def test_new_batches_cover_one_and_three_foot_support(N, delta, B):
    """Per-leg timing: all 16 support patterns; crawl: three-foot and one-foot stages.  Each >= 10 % of the stages."""
    frac, pats = _support_counts(SY.make_perleg_batch(B, N=N, delta=delta)["contact"])
    assert len(pats) == 16, sorted(pats)
    assert frac[1] >= 0.1 and frac[3] >= 0.1, frac
    frac, pats = _support_counts(SY.make_crawl_batch(B, N=N, delta=delta)["contact"])
    assert frac[1] >= 0.1 and frac[3] >= 0.1 and frac[2] == 0, frac
    assert {p for p in pats if sum(p) == 1} == {tuple(1 - np.array(c)) for c in SY.CRAWLS.values()}
    # (the two-beat gaits never have them: what the batches of the rest of the suite cover)
    frac, _ = _support_counts(SY.config3(512)["contact"])
    assert frac[1] == 0 and frac[3] == 0


def test_new_batches_span_the_friction_range():
    for b in (SY.make_perleg_batch(512), SY.make_crawl_batch(512)):
        mu = b["mu"]
        assert mu.min() >= 0.05 and mu.max() <= 3.0
        assert (mu < 0.1).sum() >= 5 and (mu > 2.0).sum() >= 5


def test_perleg_timing_advances_one_tick():
    """The returned timing reproduces the batch's schedule, and the schedule one tick later is the same one shifted by a stage."""
    b = SY.make_perleg_batch(256, N=10)
    assert np.array_equal(SY.perleg_contact(b["timing"], b["t0"], 10), b["contact"])
    nxt = SY.perleg_contact(b["timing"], b["t0"] + 1, 10)
    assert np.array_equal(nxt[:, :-1], b["contact"][:, 1:])
    assert not np.array_equal(nxt, b["contact"])


def test_gait_and_rollout_generators_take_crawl_patterns():
    """make_gait_batch / make_rollout_batch accept patterns as well as names, so crawl plans reach both device entry points."""
    crawls = tuple(SY.CRAWLS.values())
    g = SY.make_gait_batch(256, N=10, gait_names=crawls, mu_range=(0.05, 3.0))
    assert np.array_equal(SY.make_gait_batch(64, N=10, gait_names=tuple(SY.CRAWLS))["feet_id"],
                          SY.make_gait_batch(64, N=10, gait_names=crawls)["feet_id"])
    frac, _ = _support_counts(SY.expand_gait_batch(g, N=10)["contact"])
    assert frac[1] >= 0.1 and frac[3] >= 0.1, frac
    assert set(g["feet_id"].sum(axis=-1).ravel().tolist()) == {1, 3}
    rb = SY.make_rollout_batch(8, gait_names=crawls[:2], total_steps=6)
    counts = rb["plan_feet_id"][:, :4].sum(axis=-1)       # the planner's first step is all four feet, then pattern and complement alternate
    assert np.all(counts[:, 0] == 4) and set(counts[:, 1:].ravel().tolist()) == {1, 3}, counts
    # the named gaits give the same batches as before
    assert np.array_equal(SY.make_gait_batch(32)["feet_id"], SY.make_gait_batch(32, gait_names=tuple(SY.GAITS.values()))["feet_id"])


# ---------------------------------------------------------------------------------------------------------------- the checker
def test_checker_answers_load_single_feet_and_cone_faces(oracle_solve):
    """Single feet carry the robot at f_max, and stance legs sit on their friction-cone faces: the active sets the GPU tests are to
    meet (the N = 10 batches of tests/test_gpu_support_patterns.py)."""
    at_fmax = face = 0
    for b in (SY.make_crawl_batch(512), SY.make_perleg_batch(512)):
        ref = oracle_solve(b)
        assert np.all(ref["status"] == 1)
        u = ref["u"].reshape(512, 10, 4, 3)
        c = b["contact"].astype(bool)
        single = c & (c.sum(axis=-1, keepdims=True) == 1)
        fz = u[..., 2]
        at_fmax += int((single & (np.abs(fz - 100.0) <= 1e-6)).sum())
        mu = b["mu"][:, None, None]
        face += int((c & (fz > 3.0 + 1e-6) & ((np.abs(np.abs(u[..., 0]) - mu * fz) <= 1e-6) |
                                              (np.abs(np.abs(u[..., 1]) - mu * fz) <= 1e-6))).sum())
        assert np.all(u[~c] == 0)
    assert at_fmax >= 10 and face >= 1000, (at_fmax, face)


@pytest.mark.parametrize("kind,N,delta,B", [("perleg", 10, 0.03, 512), ("crawl", 10, 0.03, 512), ("perleg", 20, 0.03, 128),
                                            ("crawl", 20, 0.03, 128), ("perleg", 60, 0.01, 24), ("crawl", 60, 0.01, 24)])
def test_checker_solves_and_is_certified_on_new_batches(oracle_solve, kind, N, delta, B):
    b = (SY.make_perleg_batch if kind == "perleg" else SY.make_crawl_batch)(B, N=N, delta=delta)
    ref = oracle_solve(b, N=N, delta=delta)
    assert np.all(ref["status"] == 1)
    _certify(b, ref, range(0, B, max(1, B // 8)), N, delta)


EDGES = {"mu0": {}, "fmin0": {"f_min": 0.0}, "fmin_eq_fmax": {"f_min": 25.0, "f_max": 25.0}, "fmax30": {"f_max": 30.0}}


def edge_batch(case, B=128, N=10):
    """The batches of the friction / force-bound edges: config 3 and per-leg timing, half and half; mu = 0 on every fourth QP ("mu0")."""
    a, p = SY.config3(B // 2), SY.make_perleg_batch(B - B // 2, N=N) if N != 10 else SY.make_perleg_batch(B - B // 2)
    if N != 10:
        a = SY.make_batch(B // 2, N, 0.03, 20250809, ("trot", "pronk", "amble", "gallop"), (0.3, 0.5, 0.7, 1.0))
    b = {k: np.ascontiguousarray(np.concatenate([a[k], p[k]])) for k in ("x0", "r", "contact", "xdes", "mu")}
    if case == "mu0":
        b["mu"][::4] = 0.0
    return b


@pytest.mark.parametrize("case", list(EDGES))
def test_checker_certified_at_friction_and_bound_edges(oracle_solve, case):
    """mu = 0 (the two cone rows of a leg coincide: fx = fy = 0 exactly), f_min = 0 (the vertex fz = 0 where the box and both cone
    faces meet; the checker's polish can fail there and it returns SOLVED_ADMM), f_min = f_max and f_max below the robot's weight."""
    b = edge_batch(case)
    kw = EDGES[case]
    ref = oracle_solve(b, **kw)
    assert np.all((ref["status"] == 1) | (ref["status"] == 2)), np.unique(ref["status"], return_counts=True)
    if case in ("mu0", "fmin0"):
        # (degenerate vertices: at mu = 0 the two cone rows of a leg coincide, at f_min = 0 the box and both cone faces meet at fz = 0;
        #  the checker's polish fails on some of these QPs and it returns its ADMM answer at eps 1e-10 -- certified below like the rest)
        assert (ref["status"] == 2).sum() >= 1
        if case == "mu0":
            assert np.all(ref["status"][b["mu"] != 0] == 1)
    else:
        assert np.all(ref["status"] == 1)
    adm = np.nonzero(ref["status"] == 2)[0].tolist()
    _certify(b, ref, sorted(set(range(0, 128, 16)) | set(adm)), 10, 0.03, **kw)
    u = ref["u"].reshape(128, 10, 4, 3)
    c = b["contact"].astype(bool)
    if case == "mu0":
        z = b["mu"] == 0
        pol = z & (ref["status"] == 1)
        assert np.all(u[pol][..., :2] == 0)                        # exactly, where the checker polished
        assert np.abs(u[z][..., :2]).max() <= 1e-7                 # and to its ADMM primal tolerance (1e-10 + 1e-10 |Gu|) where not
        assert (c[z].sum() >= 100)
    if case == "fmin_eq_fmax":
        assert np.all(u[c][:, 2] == 25.0)
    if case == "fmax30":
        assert (np.abs(u[c][:, 2] - 30.0) <= 1e-6).sum() >= 100


def test_checker_never_solves_infeasible_qps(oracle_solve):
    """mu < 0 with a stance leg asks for |fx| <= mu fz < 0: primal infeasible, never reported solved.  With every leg in swing the
    cone rows are all [0, 0] and mu < 0 is harmless: solved, zero forces."""
    b = SY.make_perleg_batch(16)
    b["mu"][:] = -0.3
    assert np.all(b["contact"].reshape(16, -1).any(axis=1))
    ref = oracle_solve(b, max_iter=20000)
    assert not np.any((ref["status"] == 1) | (ref["status"] == 2)), ref["status"]
    assert np.all(ref["status"] == 3) and np.all(ref["res"][:, 0] >= 0.1), ref["res"][:, 0]
    b["contact"][:] = 0
    ref = oracle_solve(b)
    assert np.all(ref["status"] == 1) and np.all(ref["u"] == 0)
