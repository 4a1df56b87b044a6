"""Disturbance wrench rows and the wrench observer on the device (include/mpcqp_disturb.h) against the host counterparts of
mpcqp.disturbance: the shift kernel element by element, every solving path with a table against the CPU checker through
DisturbedEngine, the table's lifecycle, the observer against its host twin, piece boundaries, poison, the argument checks, and the
closed loop of compensated_rollout against its host twin.

Bands: the shift and the observer hold the project's band (disturbance_cases / estimate_cases.error), the observer's times the growth
recorded in tests/golden/disturbance_fixture.npz; solves hold tests/batch_checks.py's 1e-4 / 1e-4; roll-outs hold the band of
tests/test_gpu_gaits.py (forces 1e-4 of their scale, states 1e-5)."""
import functools

import numpy as np
import pytest

import disturbance_cases as C
import mpcqp
from batch_checks import check_batch
from mpcqp import disturbance, gaits

pytestmark = pytest.mark.gpu
STAGE = mpcqp.FLAG_POLISH | mpcqp.FLAG_STAGE_KERNEL
DISC = {"euler": mpcqp.DISC_EULER, "zoh": mpcqp.DISC_ZOH}
TIGHT = dict(eps_abs=1e-10, eps_rel=1e-10, max_iter=100000, polish_max=30)
KEYS = ("u", "X", "status", "iters")


def _t(a, dt):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().copy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def _cap(N, flags=mpcqp.FLAG_POLISH):
    return 10 * mpcqp.product_library().default_config(N=N, flags=flags).max_iter


@functools.lru_cache(maxsize=None)
def _solver(N=10, io="f64", disc="euler", flags=mpcqp.FLAG_POLISH):
    return mpcqp.MPCBatch(N=N, delta=C.DELTA, io_dtype=io, precision="mixed", flags=flags, disc=DISC[disc], max_iter=_cap(N, flags))


def _solve(sol, dev):
    return _host(sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True))


# ------------------------------------------------------------------------------------------------- 8. the shift kernel against the host
@pytest.mark.parametrize("disc", ["euler", "zoh"])
@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("B,N", [(1, 10), (63, 10), (64, 10), (65, 10), (257, 10), (8, 60)])
def test_shift_matches_host(B, N, io, disc):
    sol = _solver(N, io, disc)
    b, rows, mod = C.shift_case(B, N, models=True)
    x0, xdes = (b["x0"], b["xdes"]) if io == "f64" else (C.r32(b["x0"]), C.r32(b["xdes"]))
    d0, dd = _t(x0, sol.tdtype), _t(xdes, sol.tdtype)
    try:
        for models in ((None, mod) if B == 65 or N == 60 else (None,)):          # once per horizon with a model table of rows that differ
            if models is not None:
                sol.set_models(models)
            sol.set_disturbance(rows)
            dev = _host({"s": sol.disturbance_shift(d0, dd)})["s"]
            host = disturbance.shift_host(x0, xdes, rows, sol.cfg, models)
            err, band = C.error(dev, host, io)
            print(f"shift B={B} N={N} {io} {disc} models={'yes' if models is not None else 'no'}: error {err:.3e}, band {band:.3e}")
            assert err <= band
            assert np.abs(host - xdes).max() > 1e-3                                # the rows move xdes
    finally:
        sol.clear_disturbance()
        sol.clear_models()


# ------------------------------------------------------------------------------------------------ 9. every solving path reads the table
def _tuple_with_table(flags, what):
    B = 16
    b, rows, _ = C.shift_case(B, seed=1)
    sol = _solver(flags=flags)
    dev = sol.upload(b)
    keep = dev["xdes"].clone()
    try:
        sol.set_disturbance(rows)
        out = _solve(sol, dev)
        assert bool((dev["xdes"] == keep).all()) and np.array_equal(dev["xdes"].cpu().numpy(), b["xdes"])   # the caller's xdes: bit for bit
    finally:
        sol.clear_disturbance()
    plain = _solve(sol, dev)
    ref = disturbance.DisturbedEngine(C.checker(**TIGHT), rows).solve_batch_host(b["x0"], b["r"], b["contact"], b["xdes"], b["mu"])
    assert np.all(ref["status"] == 1)
    check_batch(out, b, ref, max_iter=_cap(10, flags), allowed=0, what=what)
    s, _ = disturbance.offsets_host(b["x0"], rows, sol.cfg)
    assert np.abs(s).max() > 1e-2 and np.abs(out["X"] - plain["X"]).max() > 1e-3     # X_out includes s: far outside the band without it
    return out


def test_solve_batch_reads_the_table_dense():
    _tuple_with_table(mpcqp.FLAG_POLISH, "solve_batch with a disturbance table, dense engine")


def test_solve_batch_reads_the_table_stagewise():
    _tuple_with_table(STAGE, "solve_batch with a disturbance table, stage-wise engine")


def test_gait_and_phase_entries_read_the_table():
    B, N = 16, 10
    sol = _solver()
    _, rows, _ = C.shift_case(B, seed=2)
    eng = disturbance.DisturbedEngine(C.checker(**TIGHT), rows)
    g = mpcqp.synth.make_gait_batch(B, N=N)
    t = mpcqp.synth.expand_gait_batch(g, N=N)
    pb = gaits.make_phase_batch(B, tuple(gaits.GAITS), 10, seed=9)
    pb["tick"] = np.arange(B, dtype=np.int32)
    e = gaits.phase_expand_host(pb["x"], pb["ref"], pb["feet"], pb["gait"], pb["tick"], pb["stand"], pb["gain"], N, C.DELTA)
    tp = {"x0": pb["x"], "r": e["r"], "contact": e["contact"], "xdes": e["xdes"], "mu": pb["mu"]}
    import torch
    try:
        sol.set_disturbance(rows)
        gd = sol.upload_gait(g)
        og = _host(sol.solve_batch_gait(gd["x0"], gd["ref"], gd["feet0"], gd["footholds"], gd["gait"], gd["feet_id"], gd["mu"], want_X=True))
        dt = sol.tdtype
        d = {k: _t(pb[k], torch.int32 if k in ("gait", "tick") else dt) for k in ("x", "ref", "feet", "gait", "tick", "stand", "gain", "mu")}
        op = _host(sol.solve_batch_phase(d["x"], d["ref"], d["feet"], d["gait"], d["tick"], d["stand"], d["gain"], d["mu"], want_X=True))
    finally:
        sol.clear_disturbance()
    for out, tup, what in ((og, t, "solve_batch_gait"), (op, tp, "solve_batch_phase")):
        ref = eng.solve_batch_host(tup["x0"], tup["r"], tup["contact"], tup["xdes"], tup["mu"])
        assert np.all(ref["status"] == 1)
        check_batch(out, tup, ref, max_iter=_cap(N), allowed=0, what=what + " with a disturbance table")


def _device_fixture(sol, B=C.B_FIX):
    """The fixture's state on the device (tiled to B robots) and the closure that rolls n ticks in place."""
    import torch
    pb, idx, dt = C.fixture_batch(), np.arange(B) % C.B_FIX, sol.tdtype
    st = {k: _t(pb[k][idx], dt) for k in ("x", "ref", "feet")}
    st["tick"] = _t(pb["tick"][idx], torch.int32)
    const = {"gait": _t(pb["gait"][idx], torch.int32), "stand": _t(pb["stand"][idx], dt), "gain": _t(pb["gain"][idx], dt), "mu": _t(pb["mu"][idx], dt),
             "push": _t(C.PUSH[idx], dt), "push_ticks": _t(C.PUSH_TICKS[idx], torch.int32)}
    step = lambda n: sol.rollout_phase(st["x"], st["ref"], st["feet"], const["gait"], const["stand"], const["gain"], st["tick"], const["mu"], n,
                                       push=const["push"], push_ticks=const["push_ticks"])
    return st, step


def _rollout_band(out, ref, what):
    sc = max(1.0, np.abs(ref["forces"]).max())
    figures = {"forces": (np.abs(out["forces"] - ref["forces"]).max(), 1e-4 * sc), "actual": (np.abs(out["actual"] - ref["actual"]).max(), 1e-5)}
    for k, (err, band) in figures.items():
        print(f"{what}: {k} err {err:.3e} band {band:.3e}")
    for k, (err, band) in figures.items():
        assert err <= band, (what, k, err, band)


def test_rollout_phase_reads_the_table():
    """Six ticks of the pushed fixture, 16 robots, told the true push: the checker through DisturbedEngine, tick by tick."""
    B, T = 16, 6
    sol = _solver()
    idx = np.arange(B) % C.B_FIX
    st, step = _device_fixture(sol, B)
    try:
        sol.set_disturbance(C.PUSH[idx])
        out = _host(step(T))
    finally:
        sol.clear_disturbance()
    ref = C.fixture_run("told", T)
    assert np.all(out["solved"] == T) and np.all(ref["solved"] == T)
    _rollout_band(out, {k: ref[k][idx] for k in ("forces", "actual")}, "rollout_phase with a disturbance table vs the checker")
    untold = C.fixture_run("untold", T)
    assert np.abs(ref["forces"] - untold["forces"]).max() > 1e-2 * np.abs(ref["forces"]).max()       # the table moves the forces


# ------------------------------------------------------------------------------------------------------------- 10. the table's lifecycle
def test_zero_table_cleared_table_and_no_table_are_identical():
    B = 96
    b = mpcqp.synth.config3(B=B)
    sol = mpcqp.MPCBatch(N=10, delta=C.DELTA, io_dtype="f64", precision="mixed", max_iter=_cap(10))   # a handle of its own: never had a table
    other = _solver()                                                                                # ... next to one that has had them
    dev = sol.upload(b)
    none = _solve(sol, dev)
    sol.set_disturbance(disturbance.wrench_rows(B))
    zero = _solve(sol, dev)
    sol.clear_disturbance()
    cleared = _solve(sol, dev)
    sol.clear_disturbance()                                                                          # (twice: nothing to clear)
    elsewhere = _solve(other, other.upload(b))
    for k in KEYS:
        assert np.array_equal(none[k], zero[k]), ("zero table", k)
        assert np.array_equal(none[k], cleared[k]), ("cleared table", k)
        assert np.array_equal(none[k], elsewhere[k]), ("another handle", k)
    assert ((none["status"] == 1) | (none["status"] == 2)).all()


def test_a_wrong_batch_size_names_the_entry_point_and_a_nan_row_fails_alone():
    import torch
    B = 16
    b, rows, _ = C.shift_case(B, seed=1)
    sol = _solver()
    dev = sol.upload(b)
    small = sol.upload({k: v[:8] for k, v in b.items()})
    with pytest.raises(mpcqp.MpcQpError, match="mpcqp_disturbance_shift: no disturbance table is set"):
        sol.disturbance_shift(dev["x0"], dev["xdes"])
    try:
        sol.set_disturbance(rows)
        good = _solve(sol, dev)
        with pytest.raises(mpcqp.MpcQpError, match=r"(?s)mpcqp_solve_batch:.*\b8\b.*disturbance.*\b16\b"):
            sol.solve_batch(small["x0"], small["r"], small["contact"], small["xdes"], small["mu"])
        with pytest.raises(mpcqp.MpcQpError, match=r"(?s)mpcqp_disturbance_shift:.*\b8\b.*\b16\b"):
            sol.disturbance_shift(small["x0"], small["xdes"])
        st, step = _device_fixture(sol, 4)
        with pytest.raises(mpcqp.MpcQpError, match=r"(?s)mpcqp_rollout_phase:.*\b4\b.*\b16\b"):
            step(1)
        bad = rows.copy()
        bad[5, 3] = np.nan
        bad[11, 0] = np.inf
        sol.set_disturbance(bad)
        out = _solve(sol, dev)
        sh = _host({"s": sol.disturbance_shift(dev["x0"], dev["xdes"])})["s"]
    finally:
        sol.clear_disturbance()
    with pytest.raises(ValueError):
        sol.set_disturbance(np.zeros((4, 5)))
    for call in (lambda: sol.engine.set_disturbance_ptr(0, 1), lambda: sol.engine.set_disturbance_ptr(4, 0)):
        with pytest.raises(mpcqp.MpcQpError, match="mpcqp_set_disturbance"):
            call()
    hit = np.zeros(B, bool); hit[[5, 11]] = True
    assert np.array_equal(out["status"] == -1, hit) and np.all(out["u"][hit] == 0) and np.all(out["X"][hit] == 0)
    assert np.isnan(sh[hit]).all() and np.isfinite(sh[~hit]).all()
    for k in KEYS:
        assert np.array_equal(out[k][~hit], good[k][~hit]), k                                        # no other QP changes
    _solve(sol, small)                                                                               # without a table any batch size goes again


# ----------------------------------------------------------------------------------------------- 11. the observer against the host
@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("T", [1, 2, 36])
@pytest.mark.parametrize("B", [1, 64, 65])
def test_track_matches_host(B, T, io):
    sol = _solver(io=io)
    logs = C.as_io(C.track_case(B, T), io)
    d = {k: _t(v, sol.tdtype) for k, v in logs.items()}
    dev = _host(sol.disturbance_track(d))
    host = C.host_track(B, T, io)
    _, g = C.recorded()
    for k in disturbance.OUT:
        err, band = C.error(dev[k], host[k], io)
        print(f"track B={B} T={T} {io} {k}: error {err:.3e}, band {band * g:.3e} (growth {g:.1f})")
        assert err <= band * g, (k, err)
    err, band = C.error(dev["state"], host["state"], "f64")                                          # (fp64 in both I/O dtypes)
    assert err <= band * g, ("state", err)
    if T == 36:   # pieces through `state` on the device: bit for bit the unsplit call, at a split after every row and at 1 | 35
        for cuts in (list(range(1, T)), [1]):
            state, parts = None, []
            for a, z in zip([0] + cuts, cuts + [T]):
                o = sol.disturbance_track({k: v[:, a:z].contiguous() for k, v in d.items()}, state=state)
                state = o["state"]; parts.append(o)
            got = _host({"dist": np.concatenate([_host(p)["dist"] for p in parts], axis=1),
                         "resid": np.concatenate([_host(p)["resid"] for p in parts], axis=1), "state": state})
            for k in ("dist", "resid", "state"):
                assert np.array_equal(got[k], dev[k]), (k, len(cuts))


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_track_poison_and_body_rows(io):
    sol = _solver(io=io)
    logs, body, first_bad = C.poison_case()
    cfg = C.checker().cfg
    d = {k: _t(v, sol.tdtype) for k, v in logs.items()}
    dev = _host(sol.disturbance_track(d, body=_t(body, sol.tdtype)))
    host = disturbance.disturbance_track_host(C.as_io(logs, io), cfg, body=body if io == "f64" else C.r32(body))
    _, g = C.recorded()
    for k in disturbance.OUT:
        err, band = C.error(dev[k], host[k], io)                                                      # (asserts the NaN pattern)
        assert err <= band * g, (k, err)
        for b, t0 in first_bad.items():
            assert np.array_equal(np.isnan(dev[k][b]).all(axis=1), np.arange(C.POISON_T) >= (C.POISON_T if t0 is None else t0)), (k, b)
    assert np.array_equal(np.isnan(dev["state"]).all(axis=1), np.array([t0 is not None for t0 in first_bad.values()]))
    assert np.array_equal(np.isnan(dev["state"]).any(axis=1), np.isnan(dev["state"]).all(axis=1))
    # a heavier body row is read: the force residual moves by the payload's weight and inertia
    heavy = mpcqp.plant.model_body(cfg.m, list(cfg.Ibody_inv), C.POISON_B); heavy[:, 0] += 2.0
    clean = {k: _t(v, sol.tdtype) for k, v in C.as_io(C.track_case(C.POISON_B, C.POISON_T), io).items()}
    a, b = _host(sol.disturbance_track(clean, want=("resid",))), _host(sol.disturbance_track(clean, body=_t(heavy, sol.tdtype), want=("resid",)))
    assert a["dist"] is None and abs(float((b["resid"] - a["resid"])[:, 1:, 2].mean()) - 2.0 * 9.81) < 0.5


def test_track_argument_checks():
    import ctypes
    sol = _solver()
    d = {k: _t(v, sol.tdtype) for k, v in C.track_case(4, 3).items()}
    a, f, ft = d["actual"].data_ptr(), d["forces"].data_ptr(), d["feet_log"].data_ptr()
    out = _t(np.zeros((4, 3, 6)), sol.tdtype).data_ptr()
    eng = sol.engine
    with pytest.raises(mpcqp.MpcQpError, match="mpcqp_disturbance_track: no output buffer"):
        eng.disturbance_track_ptr(4, 3, a, f, ft, 0, 0, 0, 0)
    for args in ((0, f, ft), (a, 0, ft), (a, f, 0)):
        with pytest.raises(mpcqp.MpcQpError, match="mpcqp_disturbance_track: null buffer"):
            eng.disturbance_track_ptr(4, 3, *args, 0, 0, out, 0)
    with pytest.raises(mpcqp.MpcQpError, match="mpcqp_disturbance_track: size out of range"):
        eng.disturbance_track_ptr(-1, 3, a, f, ft, 0, 0, out, 0)
    with pytest.raises(mpcqp.MpcQpError, match="mpcqp_disturbance_track: size out of range"):
        eng.disturbance_track_ptr(1 << 20, 1 << 10, a, f, ft, 0, 0, out, 0)
    par = sol.engine.library.default_wrench_observer()
    assert (par.size, par.gravity, par.kappa, par.f_lim, par.t_lim) == (ctypes.sizeof(mpcqp._capi.MpcQpWrenchObserver), -9.81, 0.2, np.inf, np.inf)
    for field, value, said in (("size", 8, "struct size mismatch"), ("gravity", 1.0, "gravity"), ("kappa", 1.5, "kappa"), ("kappa", float("nan"), "kappa"),
                               ("f_lim", -1.0, "f_lim"), ("t_lim", float("nan"), "t_lim")):
        par = sol.engine.library.default_wrench_observer()
        setattr(par, field, value)
        with pytest.raises(mpcqp.MpcQpError, match="mpcqp_disturbance_track: wrench observer.*" + said):
            eng.disturbance_track_ptr(4, 3, a, f, ft, 0, 0, out, 0, observer=par)
    eng.disturbance_track_ptr(0, 3, 0, 0, 0, 0, 0, out, 0)                                            # the empty batch needs no buffer
    eng.disturbance_track_ptr(4, 0, 0, 0, 0, 0, 0, out, 0)
    with pytest.raises(ValueError, match="want must name"):
        sol.disturbance_track(d, want=())
    with pytest.raises(ValueError, match="operand mismatch: state"):
        sol.disturbance_track(d, state=_t(np.zeros((4, 39)), d["actual"].dtype))


def test_compensated_rollout_matches_its_host_twin():
    """piece = 1 for 12 ticks on the pushed fixture: the observer's last row is the table of the next tick, on one stream."""
    T = 12
    sol = _solver()
    st, step = _device_fixture(sol)
    try:
        out = disturbance.compensated_rollout(step, T, 1, lambda logs, state: sol.disturbance_track(logs, state=state), sol.set_disturbance)
        dev = _host({**out["logs"], "dist": out["dist"], "resid": out["resid"], "state": out["state"]})
    finally:
        sol.clear_disturbance()
    host = C.fixture_run("observer", T, 1)
    assert np.all(dev["solved"] == T) and np.all(host["solved"] == T) and dev["actual"].shape == (C.B_FIX, T, 12)
    _rollout_band(dev, host, "compensated_rollout, piece 1, vs its host twin")
    # The estimates, from that band: two states within 1e-5 each and four forces within 1e-4 sc each enter a residual, and d^ is a
    # convex combination of residuals.  Force part: m 2e-5 / delta + 4e-4 sc.  Torque part: L = I omega with I <= 1 kg m^2, lever arms
    # below 0.5 m that move by 2e-5 against forces up to sc: 2e-5 / delta + 4 (0.5 1e-4 sc + 2e-5 sc).
    ed = np.abs(dev["dist"] - host["dist"])
    sc = max(1.0, np.abs(host["forces"]).max())
    bf, bt = C.checker().cfg.m * 2e-5 / C.DELTA + 4e-4 * sc, 2e-5 / C.DELTA + 4.0 * (0.5e-4 * sc + 2e-5 * sc)
    print(f"compensated_rollout estimates: force part {ed[..., :3].max():.3e} N (band {bf:.3e}), torque part {ed[..., 3:].max():.3e} N m (band {bt:.3e})")
    assert ed[..., :3].max() <= bf and ed[..., 3:].max() <= bt
