"""Both HIP engines on the inputs the two-beat gaits never produce (tests/test_support_coverage.py pins the batches and certifies
the checker on them): one- and three-foot support from crawl patterns and per-leg timing, friction log-uniform on [0.05, 3] and
exactly 0, force bounds at their edges, and primal-infeasible QPs (mu < 0 with a stance leg).

Every batch goes through tests/batch_checks.check_batch: solved QPs within 1e-4 of the checker (forces relative, states absolute),
every other QP finite with no swing force, and at most ALLOWED[...] QPs unsolved -- the count measured on an MI355X.
"""
import numpy as np
import pytest
import torch

import mpcqp
from batch_checks import check_batch
from conftest import rel_err
from test_gpu_warm_start import next_tick
from test_support_coverage import EDGES, edge_batch

pytestmark = pytest.mark.gpu
SY = mpcqp.synth
STAGE = mpcqp.FLAG_POLISH | mpcqp.FLAG_STAGE_KERNEL

# QPs left unsolved (MAX_ITER) at the default caps, measured on an MI355X (the engines are bitwise deterministic).  Every other batch
# of this file is solved in full.  mu = 0 and f_min = 0 leave far more than 1 % at the cap: DESIGN.md section 6.
ALLOWED = {"mu=0 dense": 32, "mu=0 stage": 31, "fmin0 dense": 38, "fmin0 stage": 62, "fmin_eq_fmax stage": 1, "fmax30 stage": 2}


def allowed(key):
    return ALLOWED.get(key, 0)


def make(kind, B, N=10, delta=0.03):
    return (SY.make_perleg_batch if kind == "perleg" else SY.make_crawl_batch)(B, N=N, delta=delta)


_REFS = {}


def checker(oracle_solve, key, b, N=10, delta=0.03, **kw):
    """The checker's answer of batch `b`, computed once per module (`key` names the batch)."""
    if key not in _REFS:
        _REFS[key] = oracle_solve(b, N=N, delta=delta, **kw)
    return _REFS[key]


def gpu_solve(batch, N=10, delta=0.03, io="f64", precision="mixed", **kw):
    sol = mpcqp.MPCBatch(N=N, delta=delta, io_dtype=io, precision=precision, **kw)
    dev = sol.upload(batch)
    out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True)
    torch.cuda.synchronize()
    res = {k: (v.cpu().numpy().copy() if v is not None else None) for k, v in out.items()}
    res["max_iter"] = sol.cfg.max_iter
    return res


def solved(st):
    return (st == 1) | (st == 2)


def checked(out, b, ref, what, key=None):
    """check_batch against the checker, exact zeros on every swing leg of every QP; prints the measured figures."""
    ok = check_batch(out, b, ref, max_iter=out["max_iter"], allowed=allowed(key or what), what=what)
    B, N = out["u"].shape[:2]
    swing = np.repeat(np.asarray(b["contact"]) == 0, 3, axis=2).reshape(B, N, 12)
    assert np.all(out["u"][swing] == 0), f"{what}: force on a swing leg"
    eu = rel_err(out["u"], ref["u"])[ok].max() if ok.any() else 0.0
    eX = np.abs(out["X"][ok] - ref["X"][ok]).max() if ok.any() else 0.0
    print(f"\nMEASURED {what}: B={B} unsolved={int((~ok).sum())} worst force {eu:.2e} worst state {eX:.2e}")
    if (~ok).any():
        nst = np.bincount(np.asarray(b["contact"])[~ok].sum(axis=-1).ravel(), minlength=5)
        mu = np.asarray(b["mu"])[~ok]
        print(f"MEASURED {what}: unsolved mu {mu.min():.3g}..{mu.max():.3g} (mu = 0: {int((mu == 0).sum())}), stages with 0..4 feet {nst.tolist()}, "
              f"force error at the cap {rel_err(out['u'], ref['u'])[~ok].max():.2e}")
    return ok


# ------------------------------------------------------------------------------------------------------- support patterns
@pytest.mark.parametrize("precision,io", [("mixed", "f32"), ("mixed", "f64"), ("f64", "f64")])
@pytest.mark.parametrize("kind", ["crawl", "perleg"])
def test_dense_engine_one_and_three_foot_support_n10(oracle_solve, kind, precision, io):
    b = make(kind, 512)
    ref = checker(oracle_solve, (kind, 10, 512), b)
    out = gpu_solve(b, io=io, precision=precision)
    checked(out, b, ref, f"dense N=10 {kind} {precision}/{io}")


@pytest.mark.parametrize("kind", ["crawl", "perleg"])
def test_dense_engine_one_and_three_foot_support_n20(oracle_solve, kind):
    b = make(kind, 128, N=20)
    ref = checker(oracle_solve, (kind, 20, 128), b, N=20)
    out = gpu_solve(b, N=20, io="f64", precision="mixed")
    checked(out, b, ref, f"dense N=20 {kind}")


@pytest.mark.parametrize("N,delta,B", [(10, 0.03, 128), (33, 0.03, 48), (60, 0.01, 24)])
@pytest.mark.parametrize("kind", ["crawl", "perleg"])
def test_stage_engine_one_and_three_foot_support(oracle_solve, kind, N, delta, B):
    """The stage-wise engine (explicitly at N = 10, by dispatch at 33 and at the reference's N = 60, delta = 0.01); at N = 10 the two
    engines agree with each other within 1e-4 where both solved."""
    b = make(kind, B, N=N, delta=delta)
    ref = checker(oracle_solve, (kind, N, B), b, N=N, delta=delta)
    out = gpu_solve(b, N=N, delta=delta, io="f64", precision="mixed", flags=STAGE)
    ok = checked(out, b, ref, f"stage N={N} {kind}")
    if N == 10:
        dense = gpu_solve(b, io="f64", precision="mixed")
        both = ok & solved(dense["status"])
        e = rel_err(out["u"], dense["u"])[both].max()
        print(f"MEASURED dense vs stage N=10 {kind}: {e:.2e}")
        assert e <= 1e-4, e


# ------------------------------------------------------------------------------------------------------- friction, force bounds
@pytest.mark.parametrize("engine", ["dense", "stage"])
def test_friction_zero_and_log_uniform(oracle_solve, engine):
    """mu log-uniform on [0.05, 3] (the per-leg half of the batch) and mu = 0 on every fourth QP: at mu = 0 the checker's fx = fy = 0
    exactly (where it polished), and solved QPs meet the band against those zeros."""
    b = edge_batch("mu0")
    ref = checker(oracle_solve, ("edge", "mu0"), b)
    out = gpu_solve(b, io="f64", precision="mixed", flags=STAGE if engine == "stage" else mpcqp.FLAG_POLISH)
    ok = checked(out, b, ref, f"mu=0 {engine}")
    assert ok[b["mu"] != 0].all()                                      # (what stays at the cap is the mu = 0 QPs)
    z = ok & (b["mu"] == 0)
    if z.any():
        u, ur = out["u"].reshape(128, 10, 4, 3)[z], ref["u"].reshape(128, 10, 4, 3)[z]
        scale = np.maximum(np.abs(ur).reshape(int(z.sum()), -1).max(axis=1), 1.0)[:, None, None]
        assert np.all(np.abs(u[..., :2]) <= 1e-4 * scale)


@pytest.mark.parametrize("engine", ["dense", "stage"])
@pytest.mark.parametrize("case", ["fmin0", "fmin_eq_fmax", "fmax30"])
def test_force_bound_edges(oracle_solve, case, engine):
    """f_min = 0, f_min = f_max = 25, f_max = 30 (configuration fields: one handle per case).  Where the checker returns SOLVED_ADMM
    (f_min = 0, the degenerate vertex fz = 0) its answer is the certified one of tests/test_support_coverage.py, at eps 1e-10."""
    b = edge_batch(case)
    kw = EDGES[case]
    ref = checker(oracle_solve, ("edge", case), b, **kw)
    out = gpu_solve(b, io="f64", precision="mixed", flags=STAGE if engine == "stage" else mpcqp.FLAG_POLISH, **kw)
    checked(out, b, ref, f"{case} {engine}")


# ------------------------------------------------------------------------------------------------------- infeasible QPs
@pytest.mark.parametrize("engine", ["dense", "stage"])
def test_infeasible_qps_are_capped_and_leave_the_others_alone(engine):
    """mu < 0 on QPs with stance legs (primal infeasible) inside an ordinary batch: MAX_ITER, never solved nor -1; finite outputs, no
    swing force, res[0] reports the violation; every other QP bitwise what it is without them.  An all-swing QP with mu < 0 is
    feasible and solved with zero forces."""
    B = 256 if engine == "dense" else 128
    b = SY.config3(B)
    flags = STAGE if engine == "stage" else mpcqp.FLAG_POLISH
    base = gpu_solve(b, io="f64", precision="mixed", flags=flags)
    bad = {k: np.array(v, copy=True) for k, v in b.items()}
    idx = np.arange(3, B, 17)
    assert np.all(bad["contact"][idx].reshape(len(idx), -1).any(axis=1))
    bad["mu"][idx] = -np.linspace(0.05, 1.0, len(idx))
    fl = B - 2
    bad["mu"][fl] = -0.5
    bad["contact"][fl] = 0
    out = gpu_solve(bad, io="f64", precision="mixed", flags=flags)
    st = out["status"]
    assert np.all(st[idx] == 3), st[idx]
    assert np.isfinite(out["u"][idx]).all() and np.isfinite(out["X"][idx]).all() and np.isfinite(out["res"][idx]).all()
    assert np.all(out["res"][idx, 0] >= 0.1), out["res"][idx, 0]
    swing = np.repeat(bad["contact"] == 0, 3, axis=2).reshape(B, 10, 12)
    assert np.all(out["u"][swing] == 0)
    assert solved(st[fl:fl + 1]).all() and np.all(out["u"][fl] == 0)
    keep = np.ones(B, bool)
    keep[idx] = False
    keep[fl] = False
    for k in ("u", "X", "status", "iters", "res"):
        assert np.array_equal(out[k][keep], base[k][keep]), k
    check_batch(out, bad, None, max_iter=out["max_iter"], allowed=len(idx) + allowed(f"infeasible {engine}"), what=f"infeasible {engine}")
    print(f"\nMEASURED infeasible {engine}: res[0] {out['res'][idx, 0].min():.3f}..{out['res'][idx, 0].max():.3f}")


# ------------------------------------------------------------------------------------------------------- dispatch pre-pass
def test_dispatch_prepass_on_any_support_is_a_pure_reordering():
    """The pre-pass scores one-foot stages (support_demand, nst == 1) and three-foot stages: queued outputs are bitwise those of the
    plain blockIdx = QP form, through the tuple entry (per-leg timing) and the gait entry (crawl plans)."""
    B = 2500
    b = SY.make_perleg_batch(B)
    plain = gpu_solve(b, io="f32", precision="mixed", flags=mpcqp.FLAG_POLISH | mpcqp.FLAG_NATURAL_ORDER)
    queued = gpu_solve(b, io="f32", precision="mixed")
    for k in ("u", "X", "status", "iters", "res"):
        assert np.array_equal(plain[k], queued[k], equal_nan=True), k
    check_batch(queued, b, None, max_iter=queued["max_iter"], allowed=allowed("prepass perleg"), what="prepass perleg")
    g = SY.make_gait_batch(B, gait_names=tuple(SY.CRAWLS), mu_range=(0.05, 3.0))
    outs = []
    for flags in (mpcqp.FLAG_POLISH | mpcqp.FLAG_NATURAL_ORDER, mpcqp.FLAG_POLISH):
        sol = mpcqp.MPCBatch(N=10, io_dtype="f32", precision="mixed", flags=flags)
        dev = sol.upload_gait(g)
        o = sol.solve_batch_gait(dev["x0"], dev["ref"], dev["feet0"], dev["footholds"], dev["gait"], dev["feet_id"], dev["mu"])
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy().copy() for k, v in o.items() if v is not None})
    for k in ("u", "status", "iters", "res"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    check_batch(outs[1], SY.expand_gait_batch(g), None, max_iter=sol.cfg.max_iter, allowed=allowed("prepass crawl gait"), what="prepass crawl gait")


# ------------------------------------------------------------------------------------------------------- polish updates
@pytest.mark.parametrize("N,B", [(10, 512), (20, 128)])
@pytest.mark.parametrize("kind", ["crawl", "perleg"])
def test_inverse_updates_on_one_and_three_foot_support(kind, N, B):
    """tests/test_gpu_parity.py::test_inverse_updates_give_the_rebuilds_answers where leg-stages gain or lose their only foot: the
    Sherman-Morrison updates of the polish give the rebuilds' statuses, step counts and forces (1e-8)."""
    b = make(kind, B, N=N)
    upd = gpu_solve(b, N=N, io="f64", precision="mixed", polish_cheap_steps=-1)
    reb = gpu_solve(b, N=N, io="f64", precision="mixed", polish_cheap_steps=-1, incr_legs=-1)
    assert np.array_equal(upd["status"], reb["status"]) and np.array_equal(upd["iters"], reb["iters"])
    assert mpcqp.split_iters(upd["iters"])[1].max() >= 3
    e = rel_err(upd["u"], reb["u"]).max()
    print(f"\nMEASURED updates vs rebuilds N={N} {kind}: {e:.2e}")
    assert e <= 1e-8, e


# ------------------------------------------------------------------------------------------------------- gait entry, warm start
def test_gait_entry_with_crawl_plans(oracle_solve):
    """mpcqp_solve_batch_gait_steps with crawl feet_id (three- and one-foot steps): the device expansion == the host expansion
    through the tuple entry == the checker."""
    g = SY.make_gait_batch(512, N=10, gait_names=tuple(SY.CRAWLS), mu_range=(0.05, 3.0))
    t = SY.expand_gait_batch(g)
    ref = oracle_solve(t)
    sol = mpcqp.MPCBatch(io_dtype="f64", precision="mixed")
    dg = sol.upload_gait(g)
    o = sol.solve_batch_gait(dg["x0"], dg["ref"], dg["feet0"], dg["footholds"], dg["gait"], dg["feet_id"], dg["mu"], want_X=True)
    torch.cuda.synchronize()
    og = {k: v.cpu().numpy().copy() for k, v in o.items() if v is not None}
    og["max_iter"] = sol.cfg.max_iter
    ok = checked(og, t, ref, "gait entry crawl")
    ot = gpu_solve(t, io="f64", precision="mixed")
    assert np.array_equal(og["status"], ot["status"])
    assert rel_err(og["u"], ot["u"])[ok].max() <= 5e-5


@pytest.mark.parametrize("kind", ["crawl", "perleg"])
def test_next_tick_warm_start_on_one_and_three_foot_support(oracle_solve, kind):
    """One engine solves tick t, then tick t+1 warm-started (carried over, shifted by a stage): the cold optimum of tick t+1."""
    b = make(kind, 256)
    gaits = tuple(SY.CRAWLS)
    cold = gpu_solve(b, io="f64", precision="mixed")
    nb = next_tick(b, cold["X"], gaits=gaits)
    assert not np.array_equal(nb["contact"], b["contact"])
    ref = oracle_solve(nb)
    c1 = gpu_solve(nb, io="f64", precision="mixed")
    checked(c1, nb, ref, f"next tick cold {kind}")
    eng = mpcqp.MPCBatch(N=10, io_dtype="f64", precision="mixed", warm_start=True, warm_shift=True)
    outs = []
    for batch in (b, nb):
        dev = eng.upload(batch)
        o = eng.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy().copy() for k, v in o.items() if v is not None})
    assert np.array_equal(outs[0]["u"], cold["u"])                      # first call: nothing to start from
    w1 = dict(outs[1], max_iter=eng.cfg.max_iter)
    ok = checked(w1, nb, ref, f"next tick warm {kind}")
    both = ok & solved(c1["status"])
    e = rel_err(w1["u"], c1["u"])[both].max()
    print(f"MEASURED warm vs cold {kind}: {e:.2e}")
    assert e <= 1e-4
