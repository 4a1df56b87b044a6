"""The host side of the disturbance table on every path (mpcqp.disturbance.DisturbedEngine, mpcqp.plant.plan_expand_host /
rollout_loop_host), and the conditions that tests/test_gpu_disturbance_paths.py relies on, measured on the CPU checker alone; the cases
are in tests/disturbance_path_cases.py.

  1. Without a table the Python tick loop of mpcqp_rollout is the checker's C loop (same solver, same inputs: 1e-12, in fact bit for bit).
  2. With rows, rollout_host and plant.rollout_plant_host under a DisturbedEngine run WITH the table: they differ from the table-less
     run by far more than the band.  (The handle's rollout_host is the C loop, which cannot see the rows.)
  3. The conditions of every closed loop: every tick solved, nobody below z = 0.2 m, told against untold at least 100 bands apart, and
     a neighbour's row moves robot 1 outside the band.
  4. The single QPs: the tight checker solves every QP with a finite row, and the table moves the forces by more than 100 bands.
  5. The ordered launch's distribution at B = 64: the checker solves every plain row."""
import numpy as np
import pytest

import disturbance_path_cases as P
import mpcqp
from conftest import rel_err
from mpcqp import disturbance, plant, synth

LOGS = ("forces", "actual", "desired", "x", "ref", "tick", "solved")


# ---------------------------------------------------------------------------------------------------------- 1. the Python loop, no table
@pytest.mark.parametrize("case", ["seed5", "five-steps"])
def test_python_loop_is_the_checkers_loop_without_a_table(oracle_lib, case):
    rb, T = (synth.make_rollout_batch(6, seed=5), 24) if case == "seed5" else (synth.make_rollout_batch(3, total_steps=5, seed=11), 40)
    eng = P.loop_checker()
    a = [rb[k] for k in P.PLAN_ARGS]
    c, p = eng.rollout_host(*a, T), plant.rollout_loop_host(eng, *a, T)
    w = disturbance.DisturbedEngine(eng, None).rollout_host(*a, T)                    # no rows: the handle's own loop
    for k in LOGS:
        err = float(np.abs(np.asarray(c[k], np.float64) - p[k]).max())
        print(f"{case} {k}: |python loop - C loop| {err:.3e} (bit for bit: {np.array_equal(c[k], p[k])})")
        assert err <= 1e-12, k
        assert np.array_equal(c[k], w[k]), k
    assert np.all(c["solved"] == T)


def test_plan_expand_agrees_with_the_stage_zero_rule(oracle_lib):
    """Stage 0 of the expansion is plant.stance_feet's row, on plan rows no planner would write too (tests/test_rollout.py's)."""
    rb = synth.make_rollout_batch(6, total_steps=5, seed=3)
    meta, tick = rb["plan_meta"].copy(), rb["tick"].copy()
    meta[0] = (0, 4, 2, 0); meta[1] = (5, 0, 0, 0); meta[2] = (99, 4, 2, 0); meta[3] = (5, -3, -1, 0)
    tick[4] = -7; tick[5] = 3
    e = plant.plan_expand_host(rb["x"], rb["ref"], rb["plan_pos"], rb["plan_feet_id"], meta, tick, 10, 0.03)
    feet, contact = plant.stance_feet(rb["plan_pos"], rb["plan_feet_id"], meta, tick)
    assert np.array_equal(e["contact"][:, 0], contact) and np.array_equal(e["r"][:, 0], feet - rb["x"][:, None, 3:6])
    eng = P.loop_checker()
    a = (rb["x"], rb["ref"], rb["plan_pos"], rb["plan_feet_id"], meta, tick, rb["mu"])
    c, p = eng.rollout_host(*a, 8), plant.rollout_loop_host(eng, *a, 8)
    for k in LOGS:
        assert np.array_equal(c[k], p[k]), k


# ------------------------------------------------------------------------------------------------ 2. the table reaches rollout_host
@pytest.mark.parametrize("kind", ["plan", "plant"])
def test_rollout_host_and_rollout_plant_host_run_with_the_table(oracle_lib, kind):
    told, untold = P.host_loop(kind, True), P.host_loop(kind, False)
    fb, sb = P.loop_band(told)
    df = np.abs(told["forces"] - untold["forces"]).reshape(P.PLAN_B, -1).max(axis=1)
    dx = float(np.abs(told["x"] - untold["x"]).max())
    print(f"{kind}: told against untold, forces {df.max():.3e} (band {fb:.3e}), final x {dx:.3e} (band {sb:.1e})")
    assert df.max() >= 100.0 * fb and dx >= 100.0 * sb
    assert df[0] == 0.0 and np.all(df[1:] > fb)                                       # row 0 is zero; every other robot is moved
    if kind == "plan":   # the next state is the prediction under the wrench: X[:,1] = X~[:,1] + s[1], and s[1] = delta c is not zero
        rb, rows, _ = P.plan_case()
        s, _ = disturbance.offsets_host(rb["x"], rows, P.loop_checker().cfg)
        assert np.abs(s[1:, 1]).max(axis=1).min() > 1e-4
        moved = np.abs(told["actual"][:, 1] - untold["actual"][:, 1]).max(axis=1)
        assert np.array_equal(told["actual"][:, 0], untold["actual"][:, 0]) and np.all(moved[1:] > 100.0 * sb)


# --------------------------------------------------------------------------------------------------- 3. the conditions of the closed loops
@pytest.mark.parametrize("kind", P.LOOPS)
def test_closed_loop_conditions(oracle_lib, kind):
    told, untold = P.host_loop(kind, True), P.host_loop(kind, False)
    T = told["forces"].shape[1]
    rows = {"plan": lambda: P.plan_case()[1], "plant": lambda: P.plan_case()[1], "phase": lambda: P.phase_case()[1]}.get(kind, lambda: P.legs_case()[2])()
    fb, _ = P.loop_band(told)
    assert np.all(told["solved"] == T) and np.all(untold["solved"] == T)             # condition 1
    zmin = float(told["actual"][:, :, 5].min())
    assert zmin >= 0.2                                                                # condition 2
    d = float(np.abs(P.commanded(told) - P.commanded(untold)).max())
    assert d >= 100.0 * fb                                                            # condition 4
    sw = P.run_host_loop(kind, P.swapped(rows))
    d1 = float(np.abs(P.commanded(sw)[1] - P.commanded(told)[1]).max())
    assert d1 > fb                                                                    # condition 5
    print(f"{kind}: z >= {zmin:.3f} m, told against untold {d:.3e}, a neighbour's row on robot 1 {d1:.3e}, band {fb:.3e}")
    own = rows[:P.D.B_FIX] if kind == "phase" else rows                               # (the fixture's four robots are tiled)
    assert not np.any(rows[0]) and len({tuple(r) for r in own}) == len(own)
    if kind not in ("plan", "plant", "phase"):                                        # the torque's x and y are there, so Rz matters
        assert np.all(np.any(rows[1:, 3:5] != 0.0, axis=1) | np.any(rows[1:, 0:3] != 0.0, axis=1))


@pytest.mark.parametrize("kind", ["phase", "legs"])
def test_closed_loop_conditions_with_a_model_table(oracle_lib, kind):
    ref, mod, _ = P.host_loop_models(kind)
    plain = P.host_loop(kind, True)
    T = ref["forces"].shape[1]
    fb, _ = P.loop_band(ref)
    zmin = float(ref["actual"][:, :, 5].min())
    d = np.abs(ref["forces"] - plain["forces"]).reshape(len(mod), -1).max(axis=1)
    print(f"{kind} with model rows: z >= {zmin:.3f} m, against the configuration's model per robot >= {d.min():.3e}, band {fb:.3e}")
    assert np.all(ref["solved"] == T) and zmin >= 0.2 and len({tuple(r) for r in mod}) == P.MR.CLASSES
    assert np.all(d > fb)                                                             # every robot's forces: the model rows matter


def test_the_offset_yaw_moves_the_odd_robots(oracle_lib):
    """est_init's yaw + 0.3 rad on the odd robots: their told QPs differ from the plain estimate feed's from the first tick, far outside the
    band; the even robots' first tick does not change."""
    a, b = P.host_loop("observe_yaw"), P.host_loop("observe_estimate")
    fb, _ = P.loop_band(a)
    d = np.abs(a["cmd"][:, 0] - b["cmd"][:, 0]).max(axis=1)
    print(f"offset yaw, first tick: per robot {d.round(3).tolist()}, band {fb:.3e}")
    assert np.all(d[1::2] > 10.0 * fb) and np.all(d[0::2] == 0.0)
    # what a shift from the plant's yaw would plan for, on the host: the rows turned back by the offset about z
    pb, _, rows, _ = P.legs_case(yaw=True)
    s_est, _ = disturbance.offsets_host(np.concatenate([pb["est_init"], pb["x"][:, 12:]], axis=1), rows, P.loop_checker().cfg)
    s_x, _ = disturbance.offsets_host(pb["x"], rows, P.loop_checker().cfg)
    odd = np.arange(P.LEGS_B) % 2 == 1
    gap = np.abs(s_est - s_x).reshape(P.LEGS_B, -1).max(axis=1)
    print(f"offset yaw: |s(estimate's yaw) - s(plant's yaw)| per robot {gap.round(5).tolist()}")
    assert np.all(gap[odd] > 1e-3) and np.all(gap[~odd] == 0.0)


# ------------------------------------------------------------------------------------------------------------------ 4. the single QPs
@pytest.mark.parametrize("point", P.GRID, ids=[g[0] for g in P.GRID])
def test_single_qp_conditions(oracle_lib, point):
    _, N, B, io, _, engine, disc = point
    kw = P.engine_overrides(engine, disc)
    b, rows, mod, nan_row = P.solve_case(N, B, io=io)
    fin = np.arange(B) != nan_row
    assert not np.any(rows[0]) and len({tuple(r) for r in rows[fin]}) == B - 1 and len({tuple(r) for r in mod}) == min(B, P.MR.CLASSES)
    head = np.arange(3)                                            # robots 0 (zero row), 1 and 2: enough for conditions 4 and 5
    cut = {k: v[head] for k, v in b.items()}
    for models in (None, mod):
        sub = None if models is None else models[head]
        ref = P.solve_reference(b, rows, models, N, kw)
        assert np.all(ref["status"][fin] == 1) and ref["status"][nan_row] == -1, ref["status"]          # condition 3
        plain = P.solve_reference(cut, np.zeros((3, 6)), sub, N, kw)
        e = rel_err(ref["u"][head], plain["u"])
        print(f"{point[0]} models={'yes' if models is not None else 'no'}: told against untold, relative, robots 1 and 2: {e[1]:.3e} {e[2]:.3e}")
        assert e[0] == 0.0 and e[1:].max() >= 100.0 * P.FORCE_BAND and nan_row not in head               # condition 4
        sw = P.solve_reference(cut, P.swapped(rows)[head], sub, N, kw)
        assert rel_err(sw["u"], ref["u"][head])[1] > P.FORCE_BAND                                        # condition 5
        s, _ = disturbance.offsets_host(b["x0"], np.where(fin[:, None], rows, 0.0), mpcqp.Library(P.D.ORACLE_SO).default_config(N=N, delta=P.DELTA, **kw),
                                        models)
        assert np.abs(s).max() > 1e-2


# --------------------------------------------------------------------------------------------------- 5. the ordered launch's distribution
@pytest.mark.parametrize("N,seed", [(10, 20261030), (20, 20261031)])
def test_the_checker_solves_every_plain_row_of_the_order_case(oracle_lib, N, seed):
    b, rows, mod, bad, huge = P.order_case(64, N, seed)
    ref = P.solve_reference(b, rows, mod, N, want_X=False)
    plain = np.setdiff1d(np.arange(64), np.concatenate([bad, huge]))
    assert len(bad) == 12 and len(huge) == 6 and not np.isfinite(rows[bad]).all(axis=1).any() and np.isfinite(rows[huge]).all()
    assert np.all(ref["status"][bad] == -1) and np.all(ref["status"][plain] == 1), ref["status"]
