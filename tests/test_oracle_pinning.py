"""Pins the CPU oracle (test infrastructure) before anything is compared with it.

What the reference offers for this path: no tests, no fixtures; one committed run log.
The log pins the QP *inputs* exactly and the *outputs* only loosely (the logged OSQP answers are unconverged).
So: (1) the two independent restatements (numpy, literal sparse + condensed; C, literal condensed) must agree;
(2) every oracle answer must pass an explicit KKT check of the QP src/mpc.py:58-173 defines;
(3) the model constants are pinned by the logged horizon predictions (Euler dynamics with delta=0.01, m=8.885);
(4) the oracle's optimum must not be worse than the reference's own logged (unconverged) prediction;
(5) the committed golden optima are reproduced.
Solver outputs remain "parity unpinned" against OSQP itself (absent from the image, version unpinned upstream).
"""
import numpy as np
import pytest

import mpcqp
import qp_spec as S
from batch_checks import kkt_certificate
from conftest import rel_err


def _qp(golden, N, i):
    q = golden["qp_inputs"]
    return q[f"N{N}_x0"][i], q[f"N{N}_r"][i], q[f"N{N}_contact"][i], q[f"N{N}_xdes"][i], float(q["mu"])


def test_sparse_and_condensed_forms_agree():
    """The literal multiple-shooting QP of src/mpc.py:58-173 and the condensed form have the same optimum."""
    b = mpcqp.synth.make_batch(3, N=4, delta=0.03, seed=5, gait_names=("trot", "gallop"), mus=(0.5, 1.0))
    cfg = S.QPConfig(N=4, delta=0.03, alpha=1e-2)
    for i in range(3):
        x0, r, c, xd, mu = b["x0"][i], b["r"][i], b["contact"][i], b["xdes"][i], b["mu"][i]
        H, g, c0, G, lo, hi, Sx, Su = S.condensed_qp(x0, r, c, xd, mu, cfg)
        u, z, y, *_ = S.admm_solve(H, g, G, lo, hi, eps=1e-10, max_iter=60000)
        u, y, ok = S.polish(H, g, G, lo, hi, u, y)
        assert ok
        P, q, c0s, Ac, los, his = S.sparse_qp(x0, r, c, xd, mu, cfg)
        X = S.predict_states(x0, u, r, c, cfg)
        zs = np.concatenate([X.reshape(-1), u])
        Az = Ac @ zs
        assert np.all(Az >= los - 1e-7) and np.all(Az <= his + 1e-7)              # feasible in the literal form
        Js = 0.5 * zs @ P @ zs + q @ zs + c0s
        Jc = 0.5 * u @ H @ u + g @ u + c0
        assert abs(Js - Jc) <= 1e-9 * max(1.0, abs(Jc))
        assert abs(S.objective(X, u, xd, cfg) - Jc) <= 1e-9 * max(1.0, abs(Jc))
        # the sparse QP solved on its own (generic ADMM on P,q,Ac) reaches the same objective and states
        zz, _, _, it, rp, rd = S.admm_solve(P, q, Ac, np.maximum(los, -1e20), np.minimum(his, 1e20), rho=1.0,
                                            eps=1e-9, max_iter=40000)
        assert abs((0.5 * zz @ P @ zz + q @ zz + c0s) - Jc) <= 1e-5 * max(1.0, abs(Jc))
        assert np.abs(zz[:X.size] - X.reshape(-1)).max() <= 1e-4


@pytest.mark.parametrize("disc", ["euler", "zoh"])
def test_c_oracle_matches_numpy_restatement_and_kkt(oracle_solve, disc):
    b = mpcqp.synth.config3(24)
    ref = oracle_solve(b, disc={"euler": mpcqp.DISC_EULER, "zoh": mpcqp.DISC_ZOH}[disc])
    assert np.all(ref["status"] == 1)
    cfg = S.QPConfig(N=10, delta=0.03, alpha=1e-2, disc=disc)
    for i in range(24):
        x0, r, c, xd, mu = b["x0"][i], b["r"][i], b["contact"][i], b["xdes"][i], b["mu"][i]
        H, g, c0, G, lo, hi, *_ = S.condensed_qp(x0, r, c, xd, mu, cfg)
        u = ref["u"][i].reshape(-1)
        k = kkt_certificate(H, g, G, lo, hi, u)                    # sign-constrained multiplier fit on the active rows, then KKT
        scale = max(1.0, np.abs(g).max())
        assert k["stationarity"] <= 1e-7 * scale, k
        assert k["primal"] <= 1e-7 * max(1.0, np.abs(u).max()), k
        assert k["dual_sign"] <= 1e-9 * scale, k
        assert k["complementarity"] <= 1e-6 * scale, k               # |y| ~ scale times a bound gap <= 1e-7 |bound|
        # predicted states: literal recursion in numpy vs the C oracle's rollout
        assert np.abs(S.predict_states(x0, u, r, c, cfg) - ref["X"][i]).max() <= 1e-10
    # numpy solver path agrees with the C solver path
    for i in range(4):
        x0, r, c, xd, mu = b["x0"][i], b["r"][i], b["contact"][i], b["xdes"][i], b["mu"][i]
        H, g, c0, G, lo, hi, *_ = S.condensed_qp(x0, r, c, xd, mu, cfg)
        u, z, y, *_ = S.admm_solve(H, g, G, lo, hi, eps=1e-10, max_iter=60000)
        u, y, ok = S.polish(H, g, G, lo, hi, u, y)
        assert ok and np.abs(u - ref["u"][i].reshape(-1)).max() <= 1e-7


def test_log_pins_model_constants(golden):
    """The logged horizon predictions obey the explicit-Euler SRB model with delta=0.01 and m=8.885
    (src/mpc.py:71,110-117) to OSQP's slack: p_{k+1} = p_k + delta v_k, and the v_z row with the logged f_z."""
    L = golden["ref_log"]
    d = float(L["param_world_time_step"]); g = float(L["param_g"])
    assert d == 0.01 and float(L["param_N"]) == 60 and float(L["param_mu"]) == 1.0
    for i in (0, 1):
        Xp = L[f"pred{i}_state"]; fz = L[f"pred{i}_fz"]
        assert Xp.shape == (12, 61) and fz.shape == (4, 60)
        assert np.abs(Xp[3:6, 1:] - (Xp[3:6, :-1] + d * Xp[9:12, :-1])).max() <= 5e-3
        vz_model = Xp[11, :-1] + d * (fz.sum(axis=0) / 8.885 + g)
        assert np.abs(Xp[11, 1:] - vz_model).max() <= 5e-3          # m = 8.885 (8.782 from the URDF would miss by >5e-3? no: pinned loosely)
        # the same residual with a 10 % different mass is clearly worse -> the log does discriminate the constant
        vz_bad = Xp[11, :-1] + d * (fz.sum(axis=0) / (8.885 * 1.1) + g)
        assert np.abs(Xp[11, 1:] - vz_bad).max() > 2 * np.abs(Xp[11, 1:] - vz_model).max()


def test_qp_inputs_reproduce_logged_quantities(golden):
    """Inputs rebuilt for the golden ticks equal the logged per-tick data exactly (x0, x_des(:,0), stage-0 lever arms)."""
    L, q = golden["ref_log"], golden["qp_inputs"]
    for N in (10, 20, 60):
        for j, t in enumerate(q["ticks"]):
            assert np.array_equal(q[f"N{N}_x0"][j][:12], L["actual"][t]) and q[f"N{N}_x0"][j][12] == -9.81
            assert np.array_equal(q[f"N{N}_xdes"][j][0][:12], L["desired"][t])
            assert np.array_equal(q[f"N{N}_r"][j][0], L["feet_actual"][t] - L["actual"][t][3:6])
            assert set(np.unique(q[f"N{N}_contact"][j])) <= {0, 1}


def test_oracle_not_worse_than_logged_osqp_prediction(oracle_solve, golden):
    """At the reference's own cost (alpha = 0, N = 60, delta = 0.01) the oracle's optimum must be at least as good
    as the prediction OSQP logged at t = 0 and t = 80 (which is visibly unconverged)."""
    L, q = golden["ref_log"], golden["qp_inputs"]
    cfg = S.QPConfig(N=60, delta=0.01, alpha=0.0)
    for i, t in ((0, 0), (1, 80)):
        j = int(np.where(q["ticks"] == t)[0][0])
        x0, r, c, xd, mu = _qp(golden, 60, j)
        Xlog = np.vstack([L[f"pred{i}_state"], np.full((1, 61), -9.81)]).T          # [61,13]
        Jlog = S.objective(Xlog, np.zeros(1), xd, cfg)
        Jor = float(golden["qp_optima"]["N60_a0_J"][j])
        assert Jor <= Jlog * (1 + 1e-9)
        assert np.abs(golden["qp_optima"]["N60_a0_X"][j][:, :12] - Xlog[:, :12]).max() < 0.5   # same basin, loose


def test_golden_optima_reproduced(oracle_solve, golden):
    q, opt = golden["qp_inputs"], golden["qp_optima"]
    for N in (10, 20):
        b = {"x0": q[f"N{N}_x0"], "r": q[f"N{N}_r"], "contact": q[f"N{N}_contact"], "xdes": q[f"N{N}_xdes"],
             "mu": np.full(len(q["ticks"]), float(q["mu"]))}
        for alpha, tag in ((1e-2, "a1e-2"), (1e-4, "a1e-4")):
            sol = oracle_solve(b, N=N, delta=float(q["delta"]), alpha=alpha)
            assert np.all(sol["status"] == 1)
            assert rel_err(sol["u"], opt[f"N{N}_{tag}_u"]).max() <= 1e-8
            assert np.abs(sol["X"] - opt[f"N{N}_{tag}_X"]).max() <= 1e-9


def test_alpha0_unique_quantities(oracle_solve, golden):
    """alpha = 0 (the reference's cost): forces are not unique, objective / states / net wrench are."""
    q, opt = golden["qp_inputs"], golden["qp_optima"]
    N = 10
    b = {"x0": q[f"N{N}_x0"], "r": q[f"N{N}_r"], "contact": q[f"N{N}_contact"], "xdes": q[f"N{N}_xdes"],
         "mu": np.full(len(q["ticks"]), float(q["mu"]))}
    sol = oracle_solve(b, N=N, delta=float(q["delta"]), alpha=0.0, rho=0.3, max_iter=20000)
    cfg = S.QPConfig(N=N, delta=float(q["delta"]), alpha=0.0)
    ok = sol["status"] != 3
    assert ok.sum() >= 7
    for i in np.where(ok)[0]:
        J = S.objective(sol["X"][i], sol["u"][i], b["xdes"][i], cfg)
        assert abs(J - opt["N10_a0_J"][i]) <= 1e-6 * max(1.0, abs(J))
        assert np.abs(sol["X"][i] - opt["N10_a0_X"][i]).max() <= 1e-5


def test_nonfinite_input_flagged(oracle_solve):
    b = mpcqp.synth.config2(4)
    b["x0"][2, 4] = np.nan
    sol = oracle_solve(b)
    assert sol["status"][2] == -1 and np.all(sol["u"][2] == 0)
    assert np.all(sol["status"][[0, 1, 3]] == 1)


def test_gait_descriptor_expansion_host_vs_oracle(oracle_lib):
    """The gait entry point of the checker (literal C loops) and the vectorised numpy expansion agree exactly, and the
    expansion reproduces the planner semantics (phase = feet_id during the first ss ticks of a step, else all stance) --
    two described steps at N = 10, three and four at N = 20 (a horizon of 20 ticks spans up to three 15-tick steps), and a
    descriptor that is too short for its horizon (the last step's time runs on: all stance, the planner's own clamp)."""
    for N, S in ((10, 2), (20, 3), (20, 4), (20, 1)):
        g = mpcqp.synth.make_gait_batch(24, N=N, steps=S)
        t = mpcqp.synth.expand_gait_batch(g, N=N)
        eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config(N=N, max_iter=4000))
        a = eng.solve_batch_gait_host(g)
        b = eng.solve_batch_host(t["x0"], t["r"], t["contact"], t["xdes"], t["mu"])
        assert np.array_equal(a["u"], b["u"]) and np.array_equal(a["X"], b["X"]) and np.array_equal(a["status"], b["status"])
        for i in range(24):
            tis, ss, ds = g["gait"][i][:3]
            for k in range(N):
                tau = tis + k
                st = min(tau // (ss + ds), S - 1); tau -= st * (ss + ds)
                want = g["feet_id"][i, st] if tau < ss else np.ones(4, np.uint8)
                assert np.array_equal(t["contact"][i, k], want)
                if k > 0:
                    assert np.allclose(t["r"][i, k], g["footholds"][i, st] - t["xdes"][i, k, 3:6], atol=0)
    # with enough steps the schedule is the alternating one of the tuple generator (src/footstep_planner.py:159-177)
    g3 = mpcqp.synth.make_gait_batch(64, N=20, steps=3)
    base = mpcqp.synth.make_batch(64, 20, 0.03, 20250812, ("trot", "pronk", "amble", "gallop"), (0.3, 0.5, 0.7, 1.0))
    assert np.array_equal(mpcqp.synth.expand_gait_batch(g3, N=20)["contact"], base["contact"])


def test_torque_map_matches_reference_expression(oracle_lib):
    """tau[leg] = J[leg].T @ -forces[leg] (src/main.py:212-214) through the checker's C-ABI entry."""
    import ctypes
    rng = np.random.default_rng(5)
    B = 7
    u = np.ascontiguousarray(rng.normal(0, 30, (B, 10, 12))); J = np.ascontiguousarray(rng.normal(0, 0.2, (B, 4, 3, 3)))
    tau = np.zeros((B, 4, 3))
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    eng.torque_map_ptr(B, u.ctypes.data, J.ctypes.data, tau.ctypes.data)
    for b in range(B):
        for l in range(4):
            assert np.allclose(tau[b, l], J[b, l].T @ -u[b, 0, 3 * l:3 * l + 3], atol=1e-13)


# ------------------------------------------------------------------------------------------------------------------
# Output-side pins: every number the reference's committed log holds about its own solver OUTPUTS is checked against
# the restated QP.  The log keeps (src/logger.py:22-57, src/main.py:216-218, src/mpc.py:297-301): the stage-0 forces
# of all 1000 solves, and at t = 0 / 80 the predicted states (12 x 61) and the predicted f_z (4 x 60).  f_x / f_y of
# the predictions were not logged, so rows that involve them (omega / v_xy dynamics, friction of stages >= 1) have no
# reference-held witness; neither has optimality (OSQP stopped at its default 1e-3 tolerances).
# ------------------------------------------------------------------------------------------------------------------
OSQP_EPS = 1e-3          # OSQP default eps_abs = eps_rel (src/mpc.py:51-55 sets only max_iter and verbose)


def test_logged_stage0_forces_match_contact_mask_all_ticks(golden):
    """(a) 1000 ticks: a logged leg force is ~0 exactly when the replayed planner says the leg swings at stage 0
    (swing_param = 1 - phase, src/mpc.py:139-144,249-252; phase recorded from the reference planner itself)."""
    L, G = golden["ref_log"], golden["planner_golden"]
    F = L["forces"].reshape(1000, 4, 3)
    stance = G["replay_phase"].astype(bool)
    assert stance.shape == (1000, 4) and (~stance).sum() == 380
    slack = OSQP_EPS * (1.0 + np.abs(F).max())                       # eps_abs + eps_rel |z|_inf  (~0.1 N)
    mag = np.abs(F).max(axis=2)
    assert mag[~stance].max() <= slack                                # swing legs carry no force
    assert mag[stance].min() >= 3.0 - slack                           # stance legs carry at least f_min
    assert np.array_equal(mag > 1.0, stance)                          # the two populations are separated by > 2.8 N
    # our own planner port reproduces the same mask (it feeds contact[] of every product-path test)
    from mpcqp.footstep_planner import FootstepPlanner
    from test_planner_glue import _initial, _params
    pl = FootstepPlanner(_initial(L), _params(L), show=False)
    assert np.array_equal(np.array([pl.get_phase_at_time(t) for t in range(1000)], dtype=bool), stance)


def test_logged_stage0_forces_obey_bounds_and_friction(golden):
    """(b) logged stance forces obey 3 <= f_z <= 100 (src/mpc.py:45-46,151-157) and |f_xy| <= mu f_z
    (src/mpc.py:159-173, mu = 1) within OSQP's termination slack."""
    L, G = golden["ref_log"], golden["planner_golden"]
    F = L["forces"].reshape(1000, 4, 3)
    st = G["replay_phase"].astype(bool)
    mu = float(L["param_mu"])
    slack = OSQP_EPS * (1.0 + np.abs(F).max())
    fz = F[st][:, 2]
    assert fz.min() >= 3.0 - slack and fz.max() <= 100.0 + slack
    assert (np.abs(F[st][:, :2]).max(axis=1) - mu * fz).max() <= slack
    # the bounds do bind in the log (so the test would notice a wrong f_min / f_max): some legs sit at the lower bound
    assert (np.abs(fz - 3.0) <= slack).sum() >= 10 and fz.max() > 90.0
    # and the restated constants are the only ones compatible: f_min = 4 or mu = 0.5 would be violated by the log
    assert fz.min() < 4.0 - slack
    assert (np.abs(F[st][:, :2]).max(axis=1) - 0.5 * fz).max() > slack


def _logged_prediction_vs_sparse_rows(golden, i, t, mutate=None, stage0_forces=False):
    """Residual of the logged prediction i (tick t) on every row of the literal sparse QP (src/mpc.py:113-173) whose
    variables were all logged; returns {row class: max violation}, the OSQP termination bound, and J_log.
    ``stage0_forces``: also fill the 12 stage-0 forces of the same solve (the return value of MPC.solve that the caller logs,
    src/main.py:216-218 -> FORCES[t]): the stage-0 rows of the omega / v_xy dynamics and of the friction pyramid become checkable."""
    L, q = golden["ref_log"], golden["qp_inputs"]
    N = 60
    cfg = S.QPConfig(N=N, delta=0.01, alpha=0.0)
    j = int(np.where(q["ticks"] == t)[0][0])
    x0, r, c, xd, mu = _qp(golden, N, j)
    P, qv, c0, A, lo, hi, lab = S.sparse_qp(x0, r, c, xd, mu, cfg, labels=True)
    if mutate:
        A, lo, hi = mutate(A.copy(), lo.copy(), hi.copy(), lab, c)
    nX = 13 * (N + 1)
    z = np.full(nX + 12 * N, np.nan)
    z[:nX] = np.vstack([L[f"pred{i}_state"], np.full((1, N + 1), -9.81)]).T.reshape(-1)
    z[nX + 2::3] = L[f"pred{i}_fz"].T.reshape(-1)                     # f_z of leg l, stage k at 12 k + 3 l + 2
    if stage0_forces:
        assert np.array_equal(L["forces"][t].reshape(4, 3)[:, 2], L[f"pred{i}_fz"][:, 0])   # the same solve's output, logged twice
        z[nX:nX + 12] = L["forces"][t]
    known = ~np.isnan(z)
    rows_ok = ~np.any((A != 0) & ~known[None, :], axis=1)
    Az = A @ np.where(known, z, 0.0)
    viol = np.maximum(np.maximum(lo - Az, Az - hi), 0.0)
    out = {name: float(viol[(lab == name) & rows_ok].max()) for name in np.unique(lab) if ((lab == name) & rows_ok).any()}
    bound = OSQP_EPS + OSQP_EPS * max(np.abs(Az[rows_ok]).max(), np.abs(z[known]).max())
    return out, bound, int(rows_ok.sum())


@pytest.mark.parametrize("i,t", [(0, 0), (1, 80)])
def test_logged_predictions_meet_osqp_primal_bound_on_sparse_rows(golden, i, t):
    """(c) the (X, f_z) OSQP logged at t = 0 / 80 satisfies the restated constraint matrix row class by row class to
    OSQP's primal termination bound eps_abs + eps_rel max(|Az|, |z|): pins signs / scales of A, l, u in the blocks
    initial state, Theta / p / v_z / g dynamics, gravity pin, swing rows, f_z box."""
    res, bound, nrows = _logged_prediction_vs_sparse_rows(golden, i, t)
    assert nrows >= 1500
    want = {"x0", "dyn_0", "dyn_1", "dyn_2", "dyn_3", "dyn_4", "dyn_5", "dyn_11", "dyn_12", "gpin", "swing", "fz_lo", "fz_hi"}
    assert want <= set(res)
    assert not ({"dyn_6", "dyn_7", "dyn_8", "dyn_9", "dyn_10", "fric_x", "fric_y"} & set(res))   # need f_x / f_y: the predictions' were
                                                                                                 # not logged (stage 0: next test)
    assert 0.05 < bound < 0.1
    for name in want:
        assert res[name] <= bound, (name, res[name], bound)
    # observed levels (regression pins, far below the bound): Euler rows hold to 4e-3, box rows exactly
    assert max(res[k] for k in ("dyn_0", "dyn_1", "dyn_2", "dyn_3", "dyn_4", "dyn_5", "dyn_11", "x0")) <= 4e-3
    assert res["fz_lo"] == 0.0 and res["fz_hi"] == 0.0 and res["gpin"] == 0.0 and res["swing"] <= 2.5e-2


def _mut_gravity_sign(A, lo, hi, lab, c):          # A[11,12] = -1 instead of +1 (src/mpc.py:94)
    rows = np.where(lab == "dyn_11")[0]
    for k, rw in enumerate(rows):
        A[rw, 13 * k + 12] *= -1
    return A, lo, hi


def _mut_force_sign(A, lo, hi, lab, c):            # forces enter v_z with the wrong sign (src/mpc.py:105-107,117)
    rows = np.where(lab == "dyn_11")[0]
    A[np.ix_(rows, np.arange(13 * 61, A.shape[1]))] *= -1
    return A, lo, hi


def _mut_mass(A, lo, hi, lab, c):                  # m = 8.885 / 2
    rows = np.where(lab == "dyn_11")[0]
    A[np.ix_(rows, np.arange(13 * 61, A.shape[1]))] *= 2
    return A, lo, hi


def _mut_velocity_sign(A, lo, hi, lab, c):         # p+ = p - delta v (src/mpc.py:92,117)
    for a in range(3):
        rows = np.where(lab == "dyn_%d" % (3 + a))[0]
        for k, rw in enumerate(rows):
            A[rw, 13 * k + 9 + a] *= -1
    return A, lo, hi


def _mut_swing_inverted(A, lo, hi, lab, c):        # swing_param = phase instead of 1 - phase (src/mpc.py:251)
    rows = np.where(lab == "swing")[0]
    cols = 13 * 61 + np.arange(720)
    A[rows, cols] = 1.0 - A[rows, cols]
    return A, lo, hi


def _mut_box_swapped(A, lo, hi, lab, c):           # f_min and f_max exchanged (src/mpc.py:45-46)
    lo[lab == "fz_lo"] *= 100.0 / 3.0
    hi[lab == "fz_hi"] *= 3.0 / 100.0
    return A, lo, hi


def _mut_x0_sign(A, lo, hi, lab, c):               # X[:,0] == -x0 (src/mpc.py:113)
    rows = np.where(lab == "x0")[0]
    lo[rows] *= -1; hi[rows] *= -1
    return A, lo, hi


@pytest.mark.parametrize("mutate,cls,beyond_bound", [
    (_mut_gravity_sign, "dyn_11", True), (_mut_force_sign, "dyn_11", True), (_mut_mass, "dyn_11", True),
    (_mut_swing_inverted, "swing", True), (_mut_box_swapped, "fz_lo", True), (_mut_x0_sign, "x0", True),
    (_mut_velocity_sign, "dyn_3", False)])
def test_sign_or_scale_error_in_a_block_is_caught_by_the_log(golden, mutate, cls, beyond_bound):
    """Demonstration that (c) discriminates: one flipped sign / wrong scale in a block breaks the OSQP bound on that row
    class (or, for the position rows where 2 delta |v| is below OSQP's slack, at least triples the residual)."""
    base, bound, _ = _logged_prediction_vs_sparse_rows(golden, 0, 0)
    bad, _, _ = _logged_prediction_vs_sparse_rows(golden, 0, 0, mutate)
    if beyond_bound:
        assert bad[cls] > bound and bad[cls] > 10 * base[cls], (cls, base[cls], bad[cls], bound)
    else:
        assert bad[cls] > 3 * base[cls], (cls, base[cls], bad[cls])


# The log holds all 12 stage-0 forces of the two solves whose predictions it kept (FORCES[t], src/main.py:216-218): with them the
# stage-0 rows of the omega dynamics (the Ihat^-1 [r]x block of B, src/mpc.py:98-107 -- the most error-prone block of the model),
# of the v_x / v_y dynamics (1 / m) and of the friction pyramid (src/mpc.py:159-173) have a reference-held witness too.
STAGE0_ROWS = ("dyn_6", "dyn_7", "dyn_8", "dyn_9", "dyn_10", "fric_x", "fric_y")


@pytest.mark.parametrize("i,t", [(0, 0), (1, 80)])
def test_logged_stage0_forces_meet_osqp_bound_on_omega_vxy_friction_rows(golden, i, t):
    res, bound, nrows = _logged_prediction_vs_sparse_rows(golden, i, t, stage0_forces=True)
    assert set(STAGE0_ROWS) <= set(res)
    for name in STAGE0_ROWS:
        assert res[name] <= bound, (name, res[name], bound)
    # observed levels (regression pins): the omega rows hold to 2e-3, v_xy to 4e-3, the friction rows exactly
    assert max(res[k] for k in ("dyn_6", "dyn_7", "dyn_8")) <= 2e-3, res
    assert max(res[k] for k in ("dyn_9", "dyn_10")) <= 5e-3, res
    assert res["fric_x"] <= 1e-3 and res["fric_y"] <= 1e-3, res


def _mut_torque_sign(A, lo, hi, lab, c):           # tau = -(r x f): the Ihat^-1 [r]x block with the wrong sign (src/mpc.py:98-107)
    for a in range(3):
        rows = np.where(lab == "dyn_%d" % (6 + a))[0]
        A[np.ix_(rows, np.arange(13 * 61, A.shape[1]))] *= -1
    return A, lo, hi


def _mut_mass_xy(A, lo, hi, lab, c):               # m = 8.885 / 2 in the v_x / v_y rows
    for a in range(2):
        rows = np.where(lab == "dyn_%d" % (9 + a))[0]
        A[np.ix_(rows, np.arange(13 * 61, A.shape[1]))] *= 2
    return A, lo, hi


def _mut_friction_half(A, lo, hi, lab, c):         # mu = 0.5 instead of params['mu'] = 1 (src/main.py:40)
    rows = np.where((lab == "fric_x") | (lab == "fric_y"))[0]
    cols = 13 * 61 + 2 + 3 * np.arange(240)
    A[np.ix_(rows, cols)] *= 0.5
    return A, lo, hi


def _mut_inertia_swapped(A, lo, hi, lab, c):       # I_body_inv = diag(1, 1/0.24, 1): pitch row scaled by 1/0.24 (src/mpc.py:73-76)
    rows = np.where(lab == "dyn_7")[0]
    A[np.ix_(rows, np.arange(13 * 61, A.shape[1]))] *= 1.0 / 0.24
    return A, lo, hi


@pytest.mark.parametrize("t_i", [(0, 0), (1, 80)])
@pytest.mark.parametrize("mutate,cls,factor", [(_mut_torque_sign, "dyn_7", 10.0), (_mut_mass_xy, "dyn_9", 2.5),
                                              (_mut_friction_half, "fric_x", None), (_mut_inertia_swapped, "dyn_7", 10.0)])
def test_stage0_force_witness_catches_torque_mass_and_friction_errors(golden, t_i, mutate, cls, factor):
    """The stage-0 witness discriminates: a flipped torque sign, a wrong pitch inertia, a halved mass in the v_xy rows or a halved
    friction coefficient each raise the residual of their row class several-fold (the pitch row: 1.5e-3 -> 5.8e-2 at t = 0)."""
    i, t = t_i
    base, bound, _ = _logged_prediction_vs_sparse_rows(golden, i, t, stage0_forces=True)
    bad, _, _ = _logged_prediction_vs_sparse_rows(golden, i, t, mutate, stage0_forces=True)
    if factor is None:
        assert bad[cls] > bound and base[cls] <= 1e-3, (cls, base[cls], bad[cls], bound)
    else:
        assert bad[cls] > factor * base[cls] and bad[cls] > 1e-2, (cls, base[cls], bad[cls])


def test_logged_prediction_objective_gap(golden):
    """(d) J_log - J_oracle >= 0 at both logged ticks (reference cost, alpha = 0, N = 60): the oracle's optimum is never
    worse than what OSQP returned.  (The gap is large -- J_log / J_oracle = 2.8 at t = 0, 2.2 at t = 80 -- because
    OSQP's default dual tolerance eps_rel |q|_inf ~ 150 leaves the force distribution essentially undetermined.)"""
    L, q = golden["ref_log"], golden["qp_inputs"]
    cfg = S.QPConfig(N=60, delta=0.01, alpha=0.0)
    for i, t in ((0, 0), (1, 80)):
        j = int(np.where(q["ticks"] == t)[0][0])
        xd = q["N60_xdes"][j]
        Xlog = np.vstack([L[f"pred{i}_state"], np.full((1, 61), -9.81)]).T
        Jlog = S.objective(Xlog, np.zeros(1), xd, cfg)
        Jor = float(golden["qp_optima"]["N60_a0_J"][j])
        gap = Jlog - Jor
        assert gap >= -1e-9 * abs(Jlog)
        assert Jor > 0.2 * Jlog, (Jlog, Jor)                   # same order of magnitude: same cost function, same weights
