"""Disturbance wrench rows and the wrench observer on the host (include/mpcqp_disturb.h; mpcqp.disturbance): the shift identity against
the literal disturbed QP, zero rows, the gravity identity, the observer's residuals on the pushed fixture, piece boundaries, poison and
argument checks, and the closed loop told and under the observer.  No GPU."""
import numpy as np
import pytest

import disturbance_cases as C
import mpcqp
import qp_spec as S
from conftest import rel_err
from mpcqp import disturbance

TOL_U, TOL_X = 1e-4, 1e-4          # tests/batch_checks.py: relative on the forces, absolute on the states
DISC = {"euler": mpcqp.DISC_EULER, "zoh": mpcqp.DISC_ZOH}
TIGHT = dict(eps_abs=1e-10, eps_rel=1e-10, max_iter=100000, polish_max=30)


def _literal_disturbed(x0, r, contact, xdes, mu, row, cfg):
    """The disturbed QP written out: X = Sx x0 + Su U + s with s from the affine recursion on qp_spec's own matrices, the cost on
    X - xdes, qp_spec's constraint rows; solved by qp_spec's ADMM and polish.  Returns (u [N,12], X [N+1,13])."""
    N, d = cfg.N, cfg.delta
    Sx, Su = S.condense(x0, r, contact, cfg)
    A, Rz = S.build_A(x0[2]), S.rot_z(x0[2])
    c = np.zeros(S.NX)
    c[6:9] = Rz @ np.diag(cfg.Ibody_inv) @ Rz.T @ row[3:6]
    c[9:12] = row[0:3] / cfg.m
    Ad, _ = S.discretise(A, np.zeros((S.NX, S.NU)), d, cfg.disc)
    Cd = d * c if cfg.disc == "euler" else (d * np.eye(S.NX) + 0.5 * d * d * A) @ c
    s = np.zeros((N + 1, S.NX))
    for k in range(N):
        s[k + 1] = Ad @ s[k] + Cd
    Wd = np.tile(np.asarray(cfg.w, float), N + 1)
    e0 = Sx @ x0 + s.reshape(-1) - xdes.reshape(-1)
    H = 2.0 * (Su.T @ (Wd[:, None] * Su)) + 2.0 * cfg.alpha * np.eye(N * S.NU)
    g = 2.0 * Su.T @ (Wd * e0)
    G, lo, hi = S.condensed_qp(x0, r, contact, xdes, mu, cfg)[3:6]
    u, _, y, *_ = S.admm_solve(H, g, G, lo, hi, eps=1e-10, max_iter=60000)
    u, y, ok = S.polish(H, g, G, lo, hi, u, y)
    assert ok
    return u.reshape(N, S.NU), (Sx @ x0 + Su @ u).reshape(N + 1, S.NX) + s


# ------------------------------------------------------------------------------------------ 1. the shift against the literal disturbed QP
@pytest.mark.parametrize("disc", ["euler", "zoh"])
def test_shifted_solve_is_the_literal_disturbed_qp(disc):
    B = 8
    b, rows, _ = C.shift_case(B)
    assert 0 < b["contact"].mean() < 1 and len({tuple(c.ravel()) for c in b["contact"]}) > 1       # mixed contacts
    eng = disturbance.DisturbedEngine(C.checker(disc=DISC[disc], **TIGHT), rows)
    out = eng.solve_batch_host(b["x0"], b["r"], b["contact"], b["xdes"], b["mu"])
    assert np.all(out["status"] == 1)
    cfg = S.QPConfig(N=10, delta=C.DELTA, alpha=1e-2, disc=disc)
    lit = [_literal_disturbed(b["x0"][i], b["r"][i], b["contact"][i], b["xdes"][i], b["mu"][i], rows[i], cfg) for i in range(B)]
    u, X = np.stack([l[0] for l in lit]), np.stack([l[1] for l in lit])
    plain = C.checker(disc=DISC[disc], **TIGHT).solve_batch_host(b["x0"], b["r"], b["contact"], b["xdes"], b["mu"])
    eu, eX = rel_err(out["u"], u).max(), np.abs(out["X"] - X).max()
    print(f"shift vs literal, {disc}: forces {eu:.3e} (band {TOL_U:g}), states {eX:.3e} (band {TOL_X:g}); "
          f"the wrench moves the forces by {rel_err(out['u'], plain['u']).max():.3e}")
    assert eu <= TOL_U and eX <= TOL_X
    assert rel_err(out["u"], plain["u"]).max() > 100 * TOL_U                                        # the rows are not a no-op


# ------------------------------------------------------------------------------------------------------------------- 2. zero rows
@pytest.mark.parametrize("disc", ["euler", "zoh"])
def test_zero_rows_leave_xdes_alone(disc):
    b, _, mod = C.shift_case(16, models=True)
    cfg = C.checker(disc=DISC[disc]).cfg
    for models in (None, mod):
        assert np.array_equal(disturbance.shift_host(b["x0"], b["xdes"], disturbance.wrench_rows(16), cfg, models), b["xdes"])


def test_shift_closed_form():
    """The recursion against the closed form the device writes (include/mpcqp_disturb.h), in both discretisations."""
    b, rows, mod = C.shift_case(5, models=True)
    for disc, th in (("euler", 0.0), ("zoh", 0.5)):
        cfg = C.checker(disc=DISC[disc]).cfg
        s, fin = disturbance.offsets_host(b["x0"], rows, cfg, mod)
        assert fin.all()
        k = np.arange(11)[None, :, None]
        cs, sn = np.cos(b["x0"][:, 2]), np.sin(b["x0"][:, 2])
        Rz = np.zeros((5, 3, 3)); Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = cs, -sn, sn, cs, 1.0
        al = np.einsum("bij,bj,bkj,bk->bi", Rz, 1.0 / mod[:, 1:4], Rz, rows[:, 3:6])
        a = rows[:, 0:3] / mod[:, 0:1]
        c2 = C.DELTA ** 2 * (0.5 * k * (k - 1) + th * k)
        want = np.concatenate([c2 * np.einsum("bij,bj->bi", Rz, al)[:, None], c2 * a[:, None], k * C.DELTA * al[:, None],
                               k * C.DELTA * a[:, None], np.zeros((5, 11, 1))], axis=2)
        assert np.abs(s - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


# ------------------------------------------------------------------------------------------------------------ 3. the gravity identity
@pytest.mark.parametrize("disc", ["euler", "zoh"])
def test_a_vertical_force_is_a_change_of_gravity(disc):
    B, a = 8, 0.5
    b, _, _ = C.shift_case(B, seed=3)
    eng = C.checker(disc=DISC[disc], **TIGHT)
    heavy = {k: v.copy() for k, v in b.items()}
    heavy["x0"][:, 12] += a
    heavy["xdes"][:, :, 12] += a
    one = eng.solve_batch_host(heavy["x0"], heavy["r"], heavy["contact"], heavy["xdes"], heavy["mu"])
    rows = disturbance.wrench_rows(B)
    rows[:, 2] = eng.cfg.m * a
    two = disturbance.DisturbedEngine(eng, rows).solve_batch_host(b["x0"], b["r"], b["contact"], b["xdes"], b["mu"])
    assert np.all(one["status"] == 1) and np.all(two["status"] == 1)
    eu, eX = rel_err(two["u"], one["u"]).max(), np.abs(two["X"][:, :, :12] - one["X"][:, :, :12]).max()
    print(f"gravity identity, {disc}: forces {eu:.3e}, states {eX:.3e}")
    assert eu <= TOL_U and eX <= TOL_X
    assert np.all(two["X"][:, :, 12] == b["x0"][:, None, 12])


# ----------------------------------------------------------------------------------------------------- 4. the observer on the fixture
def test_observer_residuals_on_the_fixture():
    run = C.fixture_run("untold")
    assert np.all(run["solved"] == C.T_FIX)
    out = disturbance.disturbance_track_host(C.truth_logs(), C.checker().cfg)
    assert np.all(out["resid"][:, 0] == 0) and np.all(out["dist"][:, 0] == 0)                   # no previous row yet
    ef = np.abs(out["resid"][:, 1:, 0:3] - C.PUSH[:, None, 0:3]).max()
    et = np.abs(out["resid"][:, 1:, 3:6] - C.PUSH[:, None, 3:6]).max()
    tau_err, _ = C.recorded()
    print(f"observer on the fixture: force residual error {ef:.3e} N (band 1e-9), torque residual error {et:.4f} N m (recorded {tau_err:.4f})")
    assert ef <= 1e-9
    assert et <= 2.0 * tau_err and tau_err < 0.1
    # the filter: d^ <- d^ + kappa (res - d^) from the second row on
    dh = np.zeros((C.B_FIX, 6))
    for t in range(1, C.T_FIX):
        dh = dh + 0.2 * (out["resid"][:, t] - dh)
        assert np.array_equal(dh, out["dist"][:, t])


def test_observer_clamps_and_reads_the_body_row():
    logs, cfg = C.truth_logs(), C.checker().cfg
    out = disturbance.disturbance_track_host(logs, cfg, observer={"kappa": 1.0, "f_lim": 7.0, "t_lim": 0.5})
    assert np.abs(out["dist"][..., 0:3]).max() == 7.0 and np.abs(out["dist"][..., 3:6]).max() == 0.5
    # a payload the observer is not told shows up as its weight: res_F_z = -m_payload g under the body the plant had
    body = mpcqp.plant.model_body(cfg.m, list(cfg.Ibody_inv), C.B_FIX)
    heavy = body.copy(); heavy[:, 0] += 2.0
    res = disturbance.disturbance_track_host(logs, cfg, body=heavy)["resid"]
    base = disturbance.disturbance_track_host(logs, cfg, body=body)["resid"]
    dv = (logs["actual"][:, 1:, 9:12] - logs["actual"][:, :-1, 9:12]) / C.DELTA
    want = 2.0 * dv; want[..., 2] += 2.0 * 9.81
    assert np.abs((res - base)[:, 1:, 0:3] - want).max() <= 1e-9


# -------------------------------------------------------------------------------------------------------------- 5. piece boundaries
def test_a_split_at_every_row_is_the_unsplit_call():
    logs, cfg = C.truth_logs(), C.checker().cfg
    whole = disturbance.disturbance_track_host(logs, cfg)
    state, dist, resid = None, [], []
    for t in range(C.T_FIX):
        o = disturbance.disturbance_track_host({k: v[:, t:t + 1] for k, v in logs.items()}, cfg, state=state)
        state = o["state"]; dist.append(o["dist"]); resid.append(o["resid"])
    assert np.array_equal(np.concatenate(dist, axis=1), whole["dist"]) and np.array_equal(np.concatenate(resid, axis=1), whole["resid"])
    assert np.array_equal(state, whole["state"]) and np.all(state[:, 39] == 1.0) and state.shape == (C.B_FIX, 40)


# ------------------------------------------------------------------------------------------------------- 6. poison and argument checks
def test_poison_rows():
    cfg = C.checker().cfg
    logs, body, first_bad = C.poison_case()
    clean = disturbance.disturbance_track_host(C.track_case(C.POISON_B, C.POISON_T), cfg)
    out = disturbance.disturbance_track_host(logs, cfg, body=body)
    for b, t0 in first_bad.items():
        for k in disturbance.OUT:
            bad = np.isnan(out[k][b]).all(axis=1)
            assert np.array_equal(bad, np.arange(12) >= (12 if t0 is None else t0)), (b, k)
            assert np.array_equal(out[k][b][~bad], clean[k][b][~bad])
        assert np.isnan(out["state"][b]).all() == (t0 is not None) and np.isnan(out["state"][b]).any() == (t0 is not None)
    # a state that is not finite poisons its robot from the first row on
    st = np.zeros((6, 40)); st[2, 3] = np.nan
    o = disturbance.disturbance_track_host(C.track_case(6, 3), cfg, state=st)
    assert np.isnan(o["dist"][2]).all() and np.isfinite(np.delete(o["dist"], 2, axis=0)).all()
    # a wrench row that is not finite poisons its own robot's xdes, and no other
    b, rows, _ = C.shift_case(4)
    rows[1, 4] = np.nan
    sh = disturbance.shift_host(b["x0"], b["xdes"], rows, cfg)
    assert np.isnan(sh[1]).all() and np.isfinite(np.delete(sh, 1, axis=0)).all()


def test_argument_checks():
    for kw in ({"gravity": 1.0}, {"gravity": float("nan")}, {"kappa": -0.1}, {"kappa": 1.5}, {"kappa": float("nan")}, {"f_lim": -1.0},
               {"t_lim": float("nan")}, {"gain": 0.2}):
        with pytest.raises(ValueError):
            disturbance.observer_row(**kw)
    assert disturbance.observer_row() == {"gravity": -9.81, "kappa": 0.2, "f_lim": float("inf"), "t_lim": float("inf")}
    par = disturbance.observer_struct({"kappa": 0.5})
    assert par.size == mpcqp._capi.ctypes.sizeof(mpcqp._capi.MpcQpWrenchObserver) and par.kappa == 0.5 and par.gravity == -9.81
    b, rows, _ = C.shift_case(4)
    with pytest.raises(ValueError):
        disturbance.shift_host(b["x0"], b["xdes"], rows[:3], C.checker().cfg)
    with pytest.raises(ValueError):
        disturbance.compensated_rollout(lambda n: {}, 4, 0, None, None)


# -------------------------------------------------------------------------------------------------------------------- 7. closed loop
def test_closed_loop_told_and_observed():
    untold, told, seen = C.fixture_run("untold"), C.fixture_run("told"), C.fixture_run("observer")
    for run in (untold, told, seen):
        assert np.all(run["solved"] == C.T_FIX)
    eu, et, es = C.final_xy_error(untold), C.final_xy_error(told), C.final_xy_error(seen)
    print("final CoM xy error [mm]: not told", np.round(1e3 * eu, 2), "told", np.round(1e3 * et, 2), "observer, piece 1", np.round(1e3 * es, 2))
    print("estimate after 36 ticks", np.round(seen["dist"][:, -1], 3))
    assert np.all(et[1:] < 0.5 * eu[1:]), (et, eu)
    assert np.all(es[1:] < 0.5 * eu[1:]), (es, eu)
    assert np.array_equal(told["actual"][0], untold["actual"][0])                                 # the unpushed robot's row is zero
    assert np.abs(seen["dist"][1:, -1, 0] - C.PUSH[1:, 0]).max() < 0.05                           # kappa = 0.2 over 35 live rows


# --------------------------------------------------------------------------------------------- the binding's table against the header
def test_abi_table_matches_the_header():
    import re
    import test_capi as tc
    capi = mpcqp._capi
    protos = tc._prototypes(capi.DISTURB_HEADER)
    table = {name: (restype, argtypes) for name, restype, argtypes in capi.DISTURB_ABI[capi.DISTURB_HEADER]}
    assert set(table) == set(protos) == set(capi.DISTURB_SYMBOLS) and len(protos) == 5
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is tc._C_RETURN[ret] and len(argtypes) == len(params), name
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            ctype = decl.rsplit(" ", 1)[0]
            if "*" in ctype or ctype == "mpcqp_handle":
                assert tc._is_pointer_type(t), (name, i, decl, t)
            else:
                assert t is tc._C_INTEGER[ctype], (name, i, decl, t)
    text = open(tc.os.path.join(tc.REPO, "include", capi.DISTURB_HEADER)).read()
    body = re.search(r"typedef struct MpcQpWrenchObserver \{(.*?)\} MpcQpWrenchObserver;", text, re.S).group(1)
    fields = [n for decl in re.findall(r"^\s*(?:uint32_t|double) ([^;]*);", body, re.M) for n in re.split(r",\s*", decl)]
    assert fields == [name for name, _ in capi.MpcQpWrenchObserver._fields_] and fields[1:] == list(disturbance.OBSERVER_DEFAULTS)
    assert int(re.search(r"#define MPCQP_DIST_STATE (\d+)", text).group(1)) == capi.DIST_STATE == disturbance.STATE
    plib = mpcqp.product_library()
    assert plib.has_disturb
    for name, restype, argtypes in capi.DISTURB_ABI[capi.DISTURB_HEADER]:
        fn = getattr(plib.lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    par = plib.default_wrench_observer()                                       # (no GPU call: the defaults are host code)
    assert {k: getattr(par, k) for k in disturbance.OBSERVER_DEFAULTS} == disturbance.OBSERVER_DEFAULTS


def test_checker_names_the_missing_header(oracle_lib):
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    with pytest.raises(mpcqp.MpcQpError, match=r"does not export include/mpcqp_disturb.h \(product library only\)"):
        eng.clear_disturbance()
