"""Per-robot model rows (include/mpcqp_model.h) through every entry point behind the table's gate that tests/test_gpu_models.py does
not reach: mpcqp_solve_batch_phase, mpcqp_rollout, mpcqp_rollout_phase, mpcqp_rollout_legs and mpcqp_rollout_drive, on the case of
tests/models_rollout_cases.py (four classes of rows cycling through the robots, every plant the body of its own row).

A roll-out's logs hold every operand of every solve a COLD engine made, so each logged (robot, tick) is replayed as an independent QP
(mpcqp.models.replay_rows) with the table tiled, row b repeated T times:

  * device against device: solve_batch_phase on the B T rows returns, bit for bit, the commanded forces the roll-out logged and the
    same solved counts -- a roll-out that read another row on some tick, or let the row reach anything but the solve, differs;
  * device against the checker: the same rows on one tight checker handle per distinct row (eps 1e-10, max_iter 100000, polish_max
    30), held with check_batch(allowed=0) at the bands of tests/batch_checks.py.  On this case a neighbour's row moves every
    replayed QP by at least 0.18 relative and the configuration's row by more than 1e-2 (tests/test_models_rollouts_host.py), so a
    wrong row on any tick misses the 1e-4 band by two to three orders of magnitude.

Conventions of tests/test_gpu_models.py: fp64 I/O, MIXED, N = 10, the engine's max_iter at ten times the host layer's default.  The
end-to-end bands are those of test_rollout_phase_matches_host_checker (tests/test_gpu_gaits.py) and
test_device_rollout_matches_oracle (tests/test_rollout.py)."""
import functools

import numpy as np
import pytest

import drive_cases as dc
import models_rollout_cases as C
import mpcqp
from batch_checks import check_batch
from conftest import rel_err
from mpcqp import models as M

pytestmark = pytest.mark.gpu

LEG_LOGS = ("swing", "q", "qd", "tau", "foot", "err", "flag", "miss")
KEYS = {"phase": C.PHASE_STATE + C.PHASE_LOGS, "legs": C.PHASE_STATE + ("legs",) + C.PHASE_LOGS + LEG_LOGS,
        "drive": C.PHASE_STATE + ("legs",) + C.PHASE_LOGS + LEG_LOGS + ("cmd",), "plan": ("x", "ref", "tick", "actual", "desired", "forces", "solved")}
PLAN_ARGS = ("x", "ref", "plan_pos", "plan_feet_id", "plan_meta", "tick", "mu")
FLOATS = ("x", "ref", "feet", "stand", "gain", "mu", "step_height", "plan_pos")
INTS = {"gait": "int32", "tick": "int32", "plan_meta": "int32", "plan_feet_id": "uint8"}


@functools.lru_cache(maxsize=None)
def _cap():
    return 10 * mpcqp.product_library().default_config(N=10, flags=mpcqp.FLAG_POLISH).max_iter


def _engine(io="f64", warm=False, **kw):
    return mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed", warm_start=warm, warm_shift=warm, max_iter=_cap(), **kw)


def _t(a, dt):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _dev(sol, d):
    """Host operands -> device tensors: floats in the engine's dtype, the leg state in fp64, integers in their own."""
    import torch
    out = {}
    for k, v in d.items():
        if k in FLOATS:
            out[k] = _t(v, sol.tdtype)
        elif k in INTS:
            out[k] = _t(v, getattr(torch, INTS[k]))
        elif k == "legs":
            out[k] = _t(v, torch.float64)
    return out


def _plant(sol, pr, body="given"):
    """The plant arguments; body "given" = the rows' own, None = NULL, or an array."""
    import torch
    b = pr["body"] if isinstance(body, str) else body
    return {"body": _t(b, sol.tdtype), "push": _t(pr["push"], sol.tdtype), "push_ticks": _t(pr["push_ticks"], torch.int32)}


def _run(sol, kind, pb, pr, T, body="given", **kw):
    """One roll-out of `kind` on the device from host operands; returns the logs and the advanced state as numpy arrays."""
    import torch
    d = _dev(sol, pb)
    if kind == "plan":
        out = sol.rollout(*[d[k] for k in PLAN_ARGS], T)
    elif kind == "phase":
        out = sol.rollout_phase(*[d[k] for k in C.PHASE_ARGS], T, **_plant(sol, pr, body))
    elif kind == "legs":
        out = sol.rollout_legs(*[d[k] for k in C.LEGS_ARGS], T, d["step_height"], kw.pop("land", "rule"), **_plant(sol, pr, body), **kw)
    else:
        ground = kw.pop("ground", None)
        out = sol.rollout_drive(*[d[k] for k in C.LEGS_ARGS], T, d["step_height"], kw.pop("land", "rule"), kw.pop("drive", "limited"),
                                _t(ground, sol.tdtype), **_plant(sol, pr, body), **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update({k: d[k].cpu().numpy() for k in ("x", "ref", "feet", "legs", "tick") if k in d})
    return res


def _same(a, b, keys, what, idx=slice(None), idx_b=slice(None)):
    for k in keys:
        assert np.array_equal(a[k][idx], b[k][idx_b], equal_nan=True), (what, k)


def _with_table(kind, rows, pb, pr, T, **kw):
    sol = _engine()
    sol.set_models(rows)
    return _run(sol, kind, pb, pr, T, **kw)


LIMITED = dict(drive="limited", inertia=dc.weak_row(0.5))


@functools.lru_cache(maxsize=None)
def _dev_phase():
    """rollout_phase on the phase case with the table (cold engine); shared, not to be altered."""
    pb, pr, rows, T = C.phase_case()
    return _with_table("phase", rows, pb, pr, T)


@functools.lru_cache(maxsize=None)
def _dev_legs_actual():
    pb, pr, rows, T = C.legs_case()
    return _with_table("legs", rows, pb, pr, T, land="actual")


@functools.lru_cache(maxsize=None)
def _dev_drive_limited():
    pb, pr, rows, T = C.drive_case()
    return _with_table("drive", rows, pb, pr, T, ground=C.drive_ground(), **LIMITED)


def _replay(what, logs, pb, rows, T, cmd="forces"):
    """Both replays of a roll-out's solves (module docstring).  Returns the worst force error against the checker."""
    import torch
    B = len(rows)
    ops = M.replay_rows(logs, pb, pb["tick"], pb["x"][:, 12])
    tiled = np.repeat(rows, T, axis=0)
    sol = _engine()
    sol.set_models(tiled)
    d = _dev(sol, ops)
    o = sol.solve_batch_phase(d["x"], d["ref"], d["feet"], d["gait"], d["tick"], d["stand"], d.get("gain"), d["mu"])
    torch.cuda.synchronize()
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}
    ok = np.isin(out["status"], (1, 2))
    # device against device, bit for bit
    assert np.array_equal(out["u"][:, 0].reshape(B, T, 12), logs[cmd]), f"{what}: the replayed QPs are not the ones the roll-out solved"
    assert np.array_equal(ok.reshape(B, T).sum(axis=1), logs["solved"]), what
    # device against the checker
    batch, ref = C.replay_reference(ops, tiled)
    assert np.all(ref["status"] == 1), what
    solved = check_batch(out, batch, ref, max_iter=_cap(), allowed=0, what=what)
    worst = float(rel_err(out["u"], ref["u"])[solved].max())
    print(f"{what}: {B * T} replayed QPs, worst force error against the checker {worst:.3e} (band 1e-4)")
    return worst


def _fz_box(forces, contact_log, rows):
    """fz <= f_max[b] + 1e-6 everywhere, and the bound is reached in every class."""
    B, T = forces.shape[:2]
    fz = forces.reshape(B, T, 4, 3)[..., 2]
    assert np.all(fz <= rows[:, 5][:, None, None] + 1e-6)
    assert C.reaches_upper_bound(forces, contact_log, rows, 1e-6).all()


# ------------------------------------------------------------------------------------------------------ 1. solve_batch_phase
def _phase_solve(sol, ops, want_X=True):
    import torch
    d = _dev(sol, ops)
    o = sol.solve_batch_phase(d["x"], d["ref"], d["feet"], d["gait"], d["tick"], d["stand"], d["gain"], d["mu"], want_X=want_X)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy().copy()) for k, v in o.items()}


def test_solve_batch_phase_with_the_table_against_the_checker():
    pb, _, rows, _ = C.phase_case()
    B = C.PHASE_B
    batch, ref = C.replay_reference(pb, rows)
    assert np.all(ref["status"] == 1)
    sol = _engine()
    sol.set_models(rows)
    out = _phase_solve(sol, pb)
    ok = check_batch(out, batch, ref, max_iter=_cap(), allowed=0, what="solve_batch_phase with a table")
    print(f"solve_batch_phase with a table: worst force error {rel_err(out['u'], ref['u'])[ok].max():.3e}")
    fz = out["u"].reshape(B, 10, 4, 3)[..., 2]
    assert np.all(fz <= rows[:, 5][:, None, None] + 1e-6)
    plain = _phase_solve(_engine(), pb)
    assert rel_err(plain["u"], ref["u"]).min() > 1e-2          # the configuration's answer is another one, for every robot


def test_solve_batch_phase_rereads_the_row_for_every_qp_of_a_resident_workgroup():
    """B = 2560 on the queued form (listed_max = -1: resident workgroups take several QPs each), four classes cycling through the
    slots: bitwise the results of one workgroup per QP (FLAG_NATURAL_ORDER), and the first 64 against the checker."""
    B = 2560
    pb = mpcqp.gaits.make_phase_batch(B, C.NAMES, 10, seed=C.PHASE_SEED)
    pb["tick"] = (np.arange(B) // 8 % 10).astype(np.int32)          # every phase of the clock under every gait
    rows = C.model_rows(B)
    res = {}
    for name, kw in (("queued", {"listed_max": -1}), ("natural", {"flags": mpcqp.FLAG_POLISH | mpcqp.FLAG_NATURAL_ORDER})):
        sol = _engine(**kw)
        sol.set_models(rows)
        res[name] = _phase_solve(sol, pb)
    _same(res["queued"], res["natural"], ("u", "X", "status", "iters", "res"), "resident workgroups")
    assert np.isin(res["queued"]["status"], (1, 2)).all()
    head = {k: v[:64] for k, v in pb.items()}
    batch, ref = C.replay_reference(head, rows[:64])
    assert np.all(ref["status"] == 1)
    check_batch({k: v[:64] for k, v in res["queued"].items()}, batch, ref, max_iter=_cap(), allowed=0, what="queued solve_batch_phase, first 64")


# ---------------------------------------------------------------------------------------------------------- 2. rollout_phase
def test_rollout_phase_with_the_table():
    pb, pr, rows, T = C.phase_case()
    B = C.PHASE_B
    out = _dev_phase()
    assert np.all(out["solved"] == T) and np.all(out["tick"] == T)
    _replay("rollout_phase", out, pb, rows, T)
    _fz_box(out["forces"], out["contact_log"], rows)
    plain = _run(_engine(), "phase", pb, pr, T)
    assert np.all(np.abs(plain["forces"] - out["forces"]).reshape(B, -1).max(axis=1) > 1e-2)      # every robot's forces: the rows matter
    # end to end against the grouped checker loop, at the bands of test_rollout_phase_matches_host_checker
    ref = C.host_phase()
    assert np.all(ref["solved"] == T) and np.array_equal(out["contact_log"], ref["contact_log"])
    sc = max(1.0, np.abs(ref["forces"]).max())
    fb = 1e-5 * (1.0 + np.abs(pb["stand"][:, :, :2]).max() + pb["gain"].max())
    figures = {"forces": (np.abs(out["forces"] - ref["forces"]).max(), 1e-4 * sc), "actual": (np.abs(out["actual"] - ref["actual"]).max(), 1e-5),
               "desired": (np.abs(out["desired"] - ref["desired"]).max(), 1e-12), "ref": (np.abs(out["ref"] - ref["ref"]).max(), 1e-12),
               "x": (np.abs(out["x"] - ref["x"]).max(), 1e-5), "feet": (np.abs(out["feet"] - ref["feet"]).max(), fb),
               "feet_log": (np.abs(out["feet_log"] - ref["feet_log"]).max(), fb)}
    for k, (err, band) in figures.items():
        print(f"rollout_phase with a table, end to end: {k} err {err:.3e} band {band:.3e}")
    for k, (err, band) in figures.items():
        assert err <= band, (k, err, band)


def test_body_null_with_a_table_is_the_configurations_body():
    """The row is the MPC's model only: with body = NULL the plant steps with the configuration's model whatever the table says."""
    pb, pr, rows, T = C.phase_case()
    cfg_body = mpcqp.plant.model_body(_engine().cfg.m, list(_engine().cfg.Ibody_inv), C.PHASE_B)
    null = _with_table("phase", rows, pb, pr, T, body=None)
    explicit = _with_table("phase", rows, pb, pr, T, body=cfg_body)
    _same(null, explicit, KEYS["phase"], "body = NULL against the configuration's body")
    assert not np.array_equal(null["actual"], _dev_phase()["actual"]) and np.isfinite(null["actual"]).all()
    # ... and the legs step (its torso acceleration is the plant's right-hand side) and the drive
    lb, lr, lrows, LT = C.legs_case()
    cfg_body = cfg_body[:C.LEGS_B]
    for kind, kw in (("legs", {"land": "actual"}), ("drive", dict(LIMITED, ground=np.where(np.arange(C.LEGS_B) % 2 == 0, dc.GROUND_MU, 1e3)))):
        null = _with_table(kind, lrows, lb, lr, LT, body=None, **kw)
        explicit = _with_table(kind, lrows, lb, lr, LT, body=cfg_body, **kw)
        _same(null, explicit, KEYS[kind], f"{kind}: body = NULL against the configuration's body")
        matched = _with_table(kind, lrows, lb, lr, LT, **kw)
        assert not np.array_equal(null["actual"], matched["actual"]) and not np.array_equal(null["q"], matched["q"], equal_nan=True)


# ----------------------------------------------------------------------------------------------------------------- 3. rollout
def test_rollout_on_a_plan_table_with_the_table():
    rb, rows, T = C.plan_case()
    ref = M.rollout_models_host(C.oracle_lib(), C.LOOP_KW, rows, *[rb[k] for k in PLAN_ARGS], T)
    out = _with_table("plan", rows, rb, None, T)
    plain = _run(_engine(), "plan", rb, None, T)
    assert np.all(out["solved"] == T) and np.all(ref["solved"] == T) and np.all(out["tick"] == T)
    sc = max(1.0, np.abs(ref["forces"]).max())
    figures = {"forces": (np.abs(out["forces"] - ref["forces"]).max(), 1e-4 * sc), "actual": (np.abs(out["actual"] - ref["actual"]).max(), 1e-5),
               "desired": (np.abs(out["desired"] - ref["desired"]).max(), 1e-12), "x": (np.abs(out["x"] - ref["x"]).max(), 1e-5),
               "ref": (np.abs(out["ref"] - ref["ref"]).max(), 1e-12)}
    for k, (err, band) in figures.items():
        print(f"rollout with a table, end to end: {k} err {err:.3e} band {band:.3e}")
    for k, (err, band) in figures.items():
        assert err <= band, (k, err, band)
    # the prediction that becomes the next state is the one under the robot's own row
    assert np.array_equal(out["actual"][:, 0], plain["actual"][:, 0])
    moved = np.abs(out["actual"][:, 1] - plain["actual"][:, 1]).max(axis=1)
    print(f"rollout with a table: actual[:,1] against no table, min over robots {moved.min():.3e}")
    assert np.all(moved > 1e-5)


# ------------------------------------------------------------------------------------------------------------ 4. rollout_legs
def test_rollout_legs_with_the_table():
    pb, pr, rows, T = C.legs_case()
    sol = _engine()
    sol.set_models(rows)
    rule = _run(sol, "legs", pb, pr, T, land="rule")
    phase = _run(sol, "phase", pb, pr, T)
    _same(rule, phase, KEYS["phase"], "rollout_legs(rule) against rollout_phase, both with the table")
    assert np.all(rule["solved"] == T)
    act = _dev_legs_actual()
    assert np.all(act["solved"] == T) and not np.array_equal(act["feet_log"], rule["feet_log"])
    _replay("rollout_legs(actual)", act, pb, rows, T)
    _fz_box(act["forces"], act["contact_log"], rows)


# ----------------------------------------------------------------------------------------------------------- 5. rollout_drive
def test_rollout_drive_with_the_table():
    import torch
    pb, pr, rows, T = C.drive_case()
    B = C.DRIVE_B
    sol = _engine()
    sol.set_models(rows)
    legs = _run(sol, "legs", pb, pr, T, land="actual")
    ideal = _run(sol, "drive", pb, pr, T, land="actual", drive="ideal", ground=None)
    _same(ideal, legs, KEYS["legs"], "ideal drive without a ground against rollout_legs, both with the table")
    assert np.array_equal(ideal["cmd"], ideal["forces"]) and np.all(ideal["solved"] == T)
    lim = _dev_drive_limited()
    assert np.all(lim["solved"] == T)
    _replay("rollout_drive(limited), commanded forces", lim, pb, rows, T, cmd="cmd")
    _fz_box(lim["cmd"], lim["contact_log"], rows)
    # the applied forces: the rule on the logged rows, as test_limited_drive_in_the_loop replays it
    n = B * T
    ground = _t(np.repeat(C.drive_ground(), T), sol.tdtype)
    rep = sol.stance_drive(_t(lim["actual"].reshape(n, 12), sol.tdtype), _t(lim["cmd"].reshape(n, 12), sol.tdtype),
                           _t(lim["feet_log"].reshape(n, 4, 3), sol.tdtype), _t(lim["contact_log"].reshape(n, 4), torch.uint8), ground,
                           inertia=LIMITED["inertia"])
    torch.cuda.synchronize()
    stance = lim["contact_log"].reshape(n, 4) != 0
    assert np.array_equal(rep["f"].cpu().numpy(), lim["forces"].reshape(n, 12))
    assert np.array_equal(rep["tau"].cpu().numpy()[stance], lim["tau"].reshape(n, 4, 3)[stance])
    assert np.array_equal(rep["flag"].cpu().numpy()[stance] & dc.BITS, lim["flag"].reshape(n, 4)[stance] & dc.BITS)
    changed = (lim["cmd"] != lim["forces"]).reshape(B, T, 4, 3).any(axis=-1)
    flag = lim["flag"]
    assert changed.sum() > 0 and ((flag & 2) != 0)[stance.reshape(B, T, 4)].any() and ((flag & 32) != 0)[stance.reshape(B, T, 4)].any()
    assert not np.array_equal(lim["forces"], ideal["forces"])
    # ideal drive on slippery ground under every robot: no torque limit, the cone alone changes the forces; the solves replay the same way
    slip = _run(sol, "drive", pb, pr, T, drive="ideal", ground=C.drive_ground(even_only=False), inertia=LIMITED["inertia"])
    assert np.all(slip["solved"] == T) and (slip["cmd"] != slip["forces"]).any() and not ((slip["flag"] & 2) != 0)[slip["contact_log"] != 0].any()
    _replay("rollout_drive(ideal, ground 0.3), commanded forces", slip, pb, rows, T, cmd="cmd")


# ------------------------------------------------------------------------------------------------- 6. the configuration's own row
def _three(sol, cases):
    """rollout_phase, rollout_legs(actual) and rollout_drive(limited) of one engine, in its current table state."""
    (pb, pr, _, T), (lb, lr, _, LT), (db, dr, _, DT) = cases
    return {"phase": _run(sol, "phase", pb, pr, T), "legs": _run(sol, "legs", lb, lr, LT, land="actual"),
            "drive": _run(sol, "drive", db, dr, DT, ground=C.drive_ground(), **LIMITED)}


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_the_configurations_own_row_changes_nothing(io):
    """m = 8 and Ibody_inv = (4, 1, 0.5) invert exactly: a table of that row gives bit for bit what no table gives, and so does the
    engine after clear_models; another table does not."""
    cases = (C.phase_case(), C.legs_case(), C.drive_case())
    sol = _engine(io, m=8.0, Ibody_inv=(4.0, 1.0, 0.5))
    base = _three(sol, cases)
    sizes = {"phase": C.PHASE_B, "legs": C.LEGS_B, "drive": C.DRIVE_B}
    for kind, case in zip(("phase", "legs", "drive"), cases):
        pb, pr, rows, T = case
        kw = {"phase": {}, "legs": {"land": "actual"}, "drive": dict(LIMITED, ground=C.drive_ground())}[kind]
        own = M.model_rows(sol.cfg, sizes[kind])
        assert np.array_equal(own[0], [8.0, 0.25, 1.0, 2.0, sol.cfg.f_min, sol.cfg.f_max])
        sol.set_models(own)
        _same(_run(sol, kind, pb, pr, T, **kw), base[kind], KEYS[kind], f"{kind} {io}: the configuration's own row")
        sol.set_models(rows)
        other = _run(sol, kind, pb, pr, T, **kw)
        assert not np.array_equal(other["forces"], base[kind]["forces"]), kind
        sol.clear_models()
        _same(_run(sol, kind, pb, pr, T, **kw), base[kind], KEYS[kind], f"{kind} {io}: after clear_models")
        assert base[kind]["solved"].min() > 0 and np.isfinite(base[kind]["actual"]).all()


# ------------------------------------------------------------------------------------------------------------ 7. an invalid row
def test_an_invalid_row_fails_alone_in_every_rollout():
    """A NaN mass on one robot: that robot solves nothing and is commanded zero force on every tick; every other robot's state and
    logs are bit for bit those of the valid table."""
    rb, prows, PT = C.plan_case()
    runs = (("phase", C.phase_case(), {}, _dev_phase, "forces"), ("legs", C.legs_case(), {"land": "actual"}, _dev_legs_actual, "forces"),
            ("drive", C.drive_case(), dict(LIMITED, ground=C.drive_ground()), _dev_drive_limited, "cmd"),
            ("plan", (rb, None, prows, PT), {}, None, "forces"))
    for kind, (pb, pr, rows, T), kw, good, cmd in runs:
        B = len(rows)
        victim = 5
        good = good() if good else _with_table(kind, rows, pb, pr, T, **kw)
        bad_rows = rows.copy()
        bad_rows[victim, 0] = np.nan
        bad = _with_table(kind, bad_rows, pb, pr, T, **kw)
        assert bad["solved"][victim] == 0 and not np.any(bad[cmd][victim]), kind
        keep = np.arange(B) != victim
        _same(bad, good, KEYS[kind], f"{kind}: robots next to an invalid row", keep, keep)
        assert np.all(bad["solved"][keep] == T), kind


# ------------------------------------------------------------------------------------------------------ 8. batch independence
def test_a_slice_of_robots_with_its_slice_of_the_table():
    sub = slice(4, 12)                                                              # 8 robots, both classes' order kept (4 % 4 == 0)
    cut = lambda d: {k: (v[sub] if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    pb, pr, rows, T = C.phase_case()
    _same(_with_table("phase", rows[sub], cut(pb), cut(pr), T), _dev_phase(), KEYS["phase"], "phase slice", slice(None), sub)
    odd = slice(5, 13)                                                              # ... and a slice that starts at another class
    _same(_with_table("phase", rows[odd], {k: v[odd] for k, v in pb.items()}, {k: v[odd] for k, v in pr.items()}, T), _dev_phase(),
          KEYS["phase"], "phase slice from class 1", slice(None), odd)
    lb, lr, lrows, LT = C.legs_case()
    _same(_with_table("legs", lrows[sub], cut(lb), cut(lr), LT, land="actual"), _dev_legs_actual(), KEYS["legs"], "legs slice", slice(None), sub)
    ground = np.where(np.arange(C.LEGS_B) % 2 == 0, dc.GROUND_MU, 1e3)
    whole = _with_table("drive", lrows, lb, lr, LT, ground=ground, **LIMITED)
    part = _with_table("drive", lrows[sub], cut(lb), cut(lr), LT, ground=ground[sub], **LIMITED)
    _same(part, whole, KEYS["drive"], "drive slice", slice(None), sub)
    assert np.all(whole["solved"] > 0) and (whole["cmd"] != whole["forces"]).any()


# ------------------------------------------------------------------------------------------------------------ 9. a warm engine
def test_a_warm_started_engine_with_the_table():
    """warm_start and warm_shift change the path to each optimum, not the optimum: every tick is solved and the forces stay within
    the end-to-end band of the cold run's checker reference.  (A warm engine's rows are not replayable: each solve also read the last.)"""
    pb, pr, rows, T = C.phase_case()
    sol = _engine(warm=True)
    sol.set_models(rows)
    out = _run(sol, "phase", pb, pr, T)
    ref = C.host_phase()
    assert np.all(out["solved"] == T)
    sc = max(1.0, np.abs(ref["forces"]).max())
    err = np.abs(out["forces"] - ref["forces"]).max()
    print(f"warm rollout_phase with a table: forces err {err:.3e} band {1e-4 * sc:.3e}, actual err {np.abs(out['actual'] - ref['actual']).max():.3e}")
    assert err <= 1e-4 * sc
    _fz_box(out["forces"], out["contact_log"], rows)
    assert not np.array_equal(out["forces"], _dev_phase()["forces"])               # (it is another path)
