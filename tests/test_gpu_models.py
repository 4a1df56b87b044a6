"""Per-robot model rows on the device (include/mpcqp_model.h): parity per model against the host checker of mpcqp.models on both
engines, a row re-read for every QP a resident workgroup takes, the configuration's row as a no-op, invalid rows, the other
entry points, and handles without a table left alone.

Every solve runs with max_iter at ten times the host layer's default for its horizon and is held to check_batch(allowed=0) with
the tolerances of tests/batch_checks.py (1e-4 relative on the forces, 1e-4 on the states); "bitwise" tests use fp64 I/O."""
import numpy as np
import pytest

import mpcqp
from batch_checks import check_batch
from conftest import ORACLE_SO, rel_err
from mpcqp import models as M

pytestmark = pytest.mark.gpu
STAGE = mpcqp.FLAG_POLISH | mpcqp.FLAG_STAGE_KERNEL
KEYS = ("u", "X", "status", "iters", "res")


def _cap(N, flags=mpcqp.FLAG_POLISH):
    return 10 * mpcqp.product_library().default_config(N=N, flags=flags).max_iter


def _oracle_lib():
    return mpcqp.Library(ORACLE_SO)


def _solve(sol, dev, want_X=True):
    import torch
    out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=want_X)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().copy() if v is not None else None) for k, v in out.items()}


def _engine(N, precision="mixed", flags=mpcqp.FLAG_POLISH, **kw):
    return mpcqp.MPCBatch(N=N, delta=0.03, io_dtype="f64", precision=precision, flags=flags, max_iter=_cap(N, flags), **kw)


def _same(a, b, what, idx=slice(None)):
    for k in KEYS:
        assert np.array_equal(a[k][idx], b[k][idx], equal_nan=True), (what, k)


def _batch(B, N):
    return mpcqp.synth.make_batch(B, N, 0.03, 20250809, ("trot", "pronk", "amble", "gallop"), (0.3, 0.5, 0.7, 1.0))   # config3's distribution


@pytest.mark.parametrize("N,B,precision,flags", [(10, 64, "mixed", mpcqp.FLAG_POLISH), (10, 64, "f64", mpcqp.FLAG_POLISH),
                                                 (20, 16, "mixed", mpcqp.FLAG_POLISH), (10, 64, "mixed", STAGE), (12, 32, "mixed", STAGE)])
def test_parity_per_model(N, B, precision, flags):
    b = mpcqp.synth.config3(B=B) if N == 10 else _batch(B, N)
    rows = mpcqp.synth.make_model_rows(B)
    cap = _cap(N, flags)
    ref = M.solve_batch_models_host(_oracle_lib(), dict(N=N, delta=0.03, max_iter=100000, eps_abs=1e-10, eps_rel=1e-10, polish_max=30), rows, b)
    assert np.all(ref["status"] == 1)
    sol = _engine(N, precision, flags)
    sol.set_models(rows)
    out = _solve(sol, sol.upload(b))
    ok = check_batch(out, b, ref, max_iter=cap, allowed=0, what=f"models N={N} {precision} flags={flags}")
    low = ok & (np.arange(B) % 4 == 3)   # the class with 2 f_max < m |g|: its upper bound is active somewhere
    fz = out["u"].reshape(B, N, 4, 3)[:, :, :, 2]
    assert np.all(fz <= rows[:, 5][:, None, None] + 1e-6)
    assert np.any(np.abs(fz[low] - rows[low, 5][:, None, None]) <= 1e-6)
    plain = _solve(_engine(N, precision, flags), sol.upload(b))
    assert rel_err(plain["u"], ref["u"]).max() > 1e-2   # (the rows matter: the configuration's answer is another one)


@pytest.mark.parametrize("N,B,flags", [(10, 2560, mpcqp.FLAG_POLISH), (20, 640, mpcqp.FLAG_POLISH), (12, 320, STAGE)])
def test_row_is_read_again_for_every_qp_of_a_resident_workgroup(N, B, flags):
    """Resident workgroups take several QPs each (dense engines: the queued form, listed_max = -1, 2048 / 512 slots; stage-wise
    engine: 256 workgroups).  With four classes cycling through the slots a workgroup that kept its previous QP's row would solve
    another QP: the results must be bitwise those of one workgroup per QP (FLAG_NATURAL_ORDER; the stage-wise engine at B <= 256)."""
    b = mpcqp.synth.config3(B=B) if N == 10 else _batch(B, N)
    rows = mpcqp.synth.make_model_rows(B)
    kw = {} if flags & mpcqp.FLAG_STAGE_KERNEL else {"listed_max": -1}
    sol = _engine(N, "mixed", flags, **kw)
    sol.set_models(rows)
    res = _solve(sol, sol.upload(b))
    if flags & mpcqp.FLAG_STAGE_KERNEL:
        # The stage-wise launch ignores FLAG_NATURAL_ORDER: it always runs min(B, slots) persistent workgroups, slots = one per CU
        # (its LDS block fills a CU).  One workgroup per QP is therefore a launch of at most `slots` QPs: two launches of 160, each
        # with its slice of the table (160 % 4 == 0 keeps the classes aligned).  Both halves of the argument depend on the CU count:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert 160 <= cus < B, f"{cus} CUs: the resident launch needs B > CUs, the reference launches at most CUs QPs"
        one = _engine(N, "mixed", flags)
        parts = []
        for lo in range(0, B, 160):
            sl = {k: v[lo:lo + 160] for k, v in b.items()}
            one.set_models(rows[lo:lo + 160])
            parts.append(_solve(one, one.upload(sl)))
        nat = {k: np.concatenate([p[k] for p in parts]) for k in KEYS}
    else:
        one = _engine(N, "mixed", flags | mpcqp.FLAG_NATURAL_ORDER)
        one.set_models(rows)
        nat = _solve(one, one.upload(b))
    _same(res, nat, f"resident N={N}")
    assert np.isin(res["status"], (1, 2)).all()
    if N == 10:   # ... and the first 64 against the checker
        h = {k: v[:64] for k, v in b.items()}
        ref = M.solve_batch_models_host(_oracle_lib(), dict(N=N, delta=0.03, max_iter=100000, eps_abs=1e-10, eps_rel=1e-10, polish_max=30), rows[:64], h)
        assert np.all(ref["status"] == 1)
        check_batch({k: v[:64] for k, v in res.items()}, h, ref, max_iter=_cap(N, flags), allowed=0, what="resident N=10, first 64")


@pytest.mark.parametrize("flags", [mpcqp.FLAG_POLISH, STAGE])
def test_configuration_row_changes_nothing(flags):
    """m = 8 and Ibody_inv = (4, 1, 0.5) invert exactly, so a table of the configuration's own row must give bit for bit what no
    table gives -- before it is set, while it is set and after clear_models."""
    B = 96
    b = mpcqp.synth.config3(B=B)
    sol = _engine(10, "mixed", flags, m=8.0, Ibody_inv=(4.0, 1.0, 0.5))
    dev = sol.upload(b)
    base = _solve(sol, dev)
    rows = np.tile([8.0, 0.25, 1.0, 2.0, sol.cfg.f_min, sol.cfg.f_max], (B, 1))
    assert np.array_equal(rows, M.model_rows(sol.cfg, B))
    sol.set_models(rows)
    _same(_solve(sol, dev), base, "configuration row")
    sol.set_models(mpcqp.synth.make_model_rows(B))
    other = _solve(sol, dev)
    assert not np.array_equal(other["u"], base["u"])
    sol.clear_models()
    _same(_solve(sol, dev), base, "after clear_models")
    assert np.isin(base["status"], (1, 2)).all()


def test_bad_rows_fail_alone_and_sizes_are_checked():
    B = 16
    b = mpcqp.synth.config3(B=B)
    rows = mpcqp.synth.make_model_rows(B)
    sol = _engine(10)
    dev = sol.upload(b)
    sol.set_models(rows)
    good = _solve(sol, dev)
    bad_rows = rows.copy()
    bad_rows[2, 0] = np.nan          # NaN mass
    bad_rows[7, 0] = 0.0             # m = 0
    bad_rows[11, 5] = bad_rows[11, 4] - 0.5   # f_max < f_min
    bad = np.zeros(B, bool); bad[[2, 7, 11]] = True
    for flags in (mpcqp.FLAG_POLISH, STAGE):
        s2 = sol if flags == mpcqp.FLAG_POLISH else _engine(10, "mixed", flags)
        if s2 is not sol:
            s2.set_models(rows)
            good = _solve(s2, dev)
        s2.set_models(bad_rows)
        out = _solve(s2, dev)
        assert np.all(out["status"][bad] == -1) and np.all(out["iters"][bad] == 0)
        assert np.all(out["u"][bad] == 0) and np.all(out["X"][bad] == 0) and np.all(out["res"][bad] == 0)
        _same(out, good, "rows next to invalid ones", ~bad)
        assert np.isin(out["status"][~bad], (1, 2)).all()
    small = {k: v[:8].contiguous() for k, v in dev.items()}
    with pytest.raises(mpcqp.MpcQpError, match=r"(?s)\b8\b.*\b16\b"):
        sol.solve_batch(small["x0"], small["r"], small["contact"], small["xdes"], small["mu"])
    with pytest.raises(ValueError):
        sol.set_models(np.zeros((4, 5)))
    with pytest.raises(mpcqp.MpcQpError, match="mpcqp_set_models"):
        sol.engine.set_models_ptr(0, 1)
    with pytest.raises(mpcqp.MpcQpError, match="mpcqp_set_models"):
        sol.engine.set_models_ptr(4, 0)
    sol.clear_models()
    _solve(sol, small)   # without a table any batch size goes again


def test_gait_entry_and_warm_start_read_the_table():
    import torch
    B, N = 64, 10
    g = mpcqp.synth.make_gait_batch(B, N=N)
    t = mpcqp.synth.expand_gait_batch(g, N=N)
    rows = mpcqp.synth.make_model_rows(B)
    sol = _engine(N)
    sol.set_models(rows)
    gd = sol.upload_gait(g)
    og = sol.solve_batch_gait(gd["x0"], gd["ref"], gd["feet0"], gd["footholds"], gd["gait"], gd["feet_id"], gd["mu"], want_X=True)
    torch.cuda.synchronize()
    og = {k: v.cpu().numpy().copy() for k, v in og.items()}
    ot = _solve(sol, sol.upload(t))
    ref = M.solve_batch_models_host(_oracle_lib(), dict(N=N, delta=0.03, max_iter=100000, eps_abs=1e-10, eps_rel=1e-10, polish_max=30), rows, t)
    assert np.all(ref["status"] == 1)
    ok = check_batch(og, t, ref, max_iter=_cap(N), allowed=0, what="gait entry with a table")
    ok &= check_batch(ot, t, ref, max_iter=_cap(N), allowed=0, what="tuple entry with a table")
    assert rel_err(og["u"], ot["u"])[ok].max() <= 5e-5   # (the band tests/test_gpu_parity.py holds the two entries to)
    # warm start: a garbage guess and then the optimum as the guess both end at the cold optimum of the robot's own model
    warm = mpcqp.MPCBatch(N=N, delta=0.03, io_dtype="f64", precision="mixed", warm_start=True, max_iter=_cap(N))
    warm.set_models(rows)
    dev = warm.upload(t)
    rng = np.random.default_rng(5)
    guess = torch.as_tensor(rng.normal(0.0, 30.0, (B, N, 12))).cuda()
    w1 = warm.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True, u_init=guess)
    torch.cuda.synchronize()
    w1 = {k: v.cpu().numpy().copy() for k, v in w1.items()}
    check_batch(w1, t, ref, max_iter=_cap(N), allowed=0, what="warm start, garbage guess, with a table")
    w2 = _solve(warm, dev)   # (the output buffer now holds the optimum)
    check_batch(w2, t, ref, max_iter=_cap(N), allowed=0, what="warm start from the optimum, with a table")
    assert mpcqp.split_iters(w2["iters"])[0].mean() < mpcqp.split_iters(w1["iters"])[0].mean()


def test_rollout_plant_with_matched_rows_matches_the_checker():
    import torch
    B, T, N = 4, 20, 10
    rb = mpcqp.synth.make_rollout_batch(B, seed=11)
    body = mpcqp.synth.make_plant_rows(B, seed=11, offdiag=0.0, mass_scale=(1.1, 1.4))["body"]
    rows = M.models_from_bodies(body, 3.0, 100.0)
    kw = dict(N=N, delta=0.03, max_iter=_cap(N))
    ref = M.rollout_plant_models_host(_oracle_lib(), kw, rows, rb["x"], rb["ref"], rb["plan_pos"], rb["plan_feet_id"], rb["plan_meta"],
                                      rb["tick"], rb["mu"], T, body=body)
    sol = _engine(N)
    sol.set_models(rows)
    f = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()
    x, rf, tk = f(rb["x"]), f(rb["ref"]), f(rb["tick"], torch.int32)
    out = sol.rollout_plant(x, rf, f(rb["plan_pos"]), f(rb["plan_feet_id"], torch.uint8), f(rb["plan_meta"], torch.int32), tk, f(rb["mu"]), T,
                            body=f(body))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.all(out["solved"] == T) and np.all(ref["solved"] == T) and np.all(tk.cpu().numpy() == T)
    sc = max(1.0, np.abs(ref["forces"]).max())
    assert np.abs(out["forces"] - ref["forces"]).max() <= 1e-4 * sc
    assert np.abs(out["actual"] - ref["actual"]).max() <= 1e-5
    assert np.abs(out["desired"] - ref["desired"]).max() <= 1e-12
    assert np.abs(rf.cpu().numpy() - ref["ref"]).max() <= 1e-12 and np.abs(x.cpu().numpy() - ref["x"]).max() <= 1e-5
    with pytest.raises(mpcqp.MpcQpError, match=r"(?s)\b2\b.*\b4\b"):
        sol.rollout_plant(x[:2].contiguous(), rf[:2].contiguous(), f(rb["plan_pos"][:2]), f(rb["plan_feet_id"][:2], torch.uint8),
                          f(rb["plan_meta"][:2], torch.int32), tk[:2].contiguous(), f(rb["mu"][:2]), 1)


def test_handles_without_a_table_are_left_alone():
    """A handle that never set a table gives bit for bit the same results before and after another handle on the device set one."""
    B = 256
    b = mpcqp.synth.config3(B=B)
    plain = _engine(10)
    dev = plain.upload(b)
    before = _solve(plain, dev)
    other = _engine(10)
    other.set_models(mpcqp.synth.make_model_rows(B))
    with_rows = _solve(other, dev)
    after = _solve(plain, dev)
    _same(after, before, "handle without a table")
    assert not np.array_equal(with_rows["u"], before["u"])
    check_batch(before, b, None, max_iter=_cap(10), allowed=0, what="config3 256")
