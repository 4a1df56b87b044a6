"""The conditions of tests/test_gpu_actuator_rows.py on the CPU checker, no GPU (include/mpcqp_actuators.h; the cases are in
tests/actuator_cases.py): what makes each device comparison discriminating -- counts, margins to the deciding thresholds, NaN / 0xff
patterns -- is asserted here from the host counterparts alone.

  1. leg_effort_host with one row per robot at T = 4: the margins, the legs beyond their envelope, what a neighbour's row changes.
  2. The stance draw over 627 rows with every invalid kind and the valid edge rows planted.
  3. rollout_legs_host with the four classes cycling through the robots, row by row; the ideal drive on slippery ground.
  4. Model rows, actuator rows and ground rows in one call of models.rollout_drive_models_host.
  5. An invalid row inside a roll-out, clause by clause, in the four modes of actuator_cases.LOOP_MODES.

The figures printed here are quoted by the documents; the tests assert floors and directions, not those values."""
import numpy as np
import pytest

import actuator_cases as ac
import drive_cases as dc
import legsim_cases
import models_rollout_cases as C
from legsim_cases import ROLL_B, ROLL_T
from mpcqp import actuators, gaits, lite3_model
from mpcqp import models as M
from test_models_rollouts_host import _replayed_u0

KNOWN_LOGS = ("q", "qd", "tau", "foot", "err")


def _same(a, b):
    return np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind == "f")


# --------------------------------------------------------------------------------------------------- 1. leg_effort, one row per robot
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_leg_effort_rows_differ_per_robot_and_decide_the_limit(io):
    s, rows = ac.effort_case(io)
    B, T = s["actual"].shape[:2]
    b = ac.INVALID_ROBOT
    ok = actuators.valid_rows(rows)
    assert (B, T) == (32, 4) and not ok[b] and ok.sum() == B - 1 and len(np.unique(rows[ok], axis=0)) == B - 1
    assert np.array_equal(np.isinf(rows[:, 3]), np.arange(B) % 5 == 4)
    for what, drop in ac.EFFORT_VARIANTS:
        h = ac.effort_host(s, rows, drop)
        h0 = lite3_model.leg_effort_host(*[None if k in drop else s[k] for k in ac.EFFORT_IN])
        live = h["limit"] != 0xff
        margin = ac.effort_margin(h, rows)
        # the table changes the limit byte only, and on robot b every byte
        for k in ("qdd", "tau_dyn", "tau", "power"):
            assert _same(h[k], h0[k]), (what, k)
        assert np.all(h["limit"][b] == 0xff) and live[np.arange(B) != b].all() and not np.any(h0["limit"] == 0xff)
        assert np.array_equal(h["limit"][live] & ~np.uint8(4), h0["limit"][live] & ~np.uint8(4))
        lo, hi = actuators.limits_host(rows, h["qd"])
        tm = rows[:, None, None, 0:3]
        with np.errstate(invalid="ignore"):
            falling = (((h["tau"] > hi) & (hi < tm)) | ((h["tau"] < lo) & (-lo < tm))).any(axis=-1) & live
        bit4, bit4_none = ((h["limit"] & 4) != 0) & live, (h0["limit"] & 4) != 0
        near = int((margin <= legsim_cases.FLAG_MARGIN).sum())
        moved = [int(((ac.effort_host(s, np.roll(rows, sh, axis=0), drop)["limit"] != h["limit"]).any(axis=(1, 2))).sum()) for sh in (1, -1)]
        print(f"leg_effort {io} {what}: smallest margin {margin.min():.2e}, bit 4 on {int(bit4.sum())} legs ({int(falling.sum())} on the falling part "
              f"of a curve), {int(bit4_none.sum())} without a table; a neighbour's row changes {moved} of {B} robots")
        assert near == 0                                                        # no leg is left out of the device comparison
        assert falling.sum() >= 20 and bit4.sum() >= 2 * bit4_none.sum() and bit4_none.sum() > 0
        assert min(moved) >= ac.EFFORT_ROBOTS_MOVED
        # a table indexed by row, not by robot, or read at slot 0 gives other bytes
        by_row = np.stack([ac.effort_host(s, rows[(np.arange(B) * T + t) % B], drop)["limit"][:, t] for t in range(T)], axis=1)
        slot0 = ac.effort_host(s, np.tile(rows[:1], (B, 1)), drop)["limit"]
        assert (by_row != h["limit"]).sum() >= 20 and (slot0 != h["limit"]).sum() >= 20


# ------------------------------------------------------------------------------------------------------- 2. the conversion, 627 rows
def test_invalid_kinds_are_those_of_the_envelope_test():
    good = actuators.actuator_rows(1, None, 1.0, 0.05, 0.25)[0]
    kinds = ac.invalid_kinds(good)
    assert len(kinds) == len(ac.CONV_INVALID) == 10 and len({k[0] for k in kinds}) == 10
    for name, col, val in kinds:
        r = good.copy()
        r[col] = val
        assert not actuators.valid_rows(r[None])[0], name


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_conversion_case_plants_every_kind_and_stays_off_the_thresholds(dtype):
    case, mended, bad = ac.conversion_case()
    c = ac.as_io(case, dtype)
    n = c["x"].shape[0]
    assert n == 627 == 2 * 256 + 115 and bad.sum() == 10
    assert np.array_equal(actuators.valid_rows(c["rows"]), ~bad) and actuators.valid_rows(mended).all()
    e = list(ac.CONV_EDGES)
    rows = c["rows"]
    assert rows[e[0], 0] == 0.0 and rows[e[1], 3] == 0.0 and rows[e[2], 1] == 0.0 and np.signbit(rows[e[2], 1])
    assert np.array_equal(rows[e[3], 6:9], rows[e[3], 3:6] + np.spacing(rows[e[3], 3:6])) and np.isnan(rows[e[4], 6:9]).all()
    h = ac.drive(c)
    st = c["contact"] != 0
    near = dc.near_threshold(h)
    print(f"conversion case {np.dtype(dtype).name}: {int(near.sum())} of {near.size} legs within FLAG_MARGIN, smallest margin {h['margin'].min():.2e}")
    assert near.mean() <= dc.MARGIN_SHARE
    # every invalid row: NaN / 0xff on its stance legs, its swing legs keep their forces; no valid row shows 0xff
    f_in, f_out = c["f"].reshape(n, 4, 3), h["f"].reshape(n, 4, 3)
    assert st[bad].any(axis=1).all() and (~st[bad]).any()
    assert np.all(h["flag"][bad][st[bad]] == 0xff) and np.isnan(f_out[bad][st[bad]]).all() and np.isnan(h["tau"][bad][st[bad]]).all()
    assert np.array_equal(f_out[bad][~st[bad]], f_in[bad][~st[bad]]) and not np.any(h["flag"][~bad] == 0xff)
    hm = ac.drive(dict(c, rows=mended))
    for k in ("f", "tau", "flag", "margin"):
        assert _same(h[k][~bad], hm[k][~bad]), k
    assert not np.any(hm["flag"] == 0xff)
    # the edge rows act: a joint without torque and a curve that falls from standstill clamp their legs
    assert np.all((h["flag"][e[0]] & 2) != 0) and np.all((h["flag"][e[2]] & 2) != 0) and np.isfinite(h["tau"][e]).all()
    # the draw repeats: the same robot under 19 different rows, so a row read at another slot shows
    first = {k: h[k][:33] for k in ("f", "tau")}
    assert sum(not _same(h[k][33 * i:33 * (i + 1)], first[k]) for i in range(1, ac.CONV_TILES) for k in first) == 2 * (ac.CONV_TILES - 1)


# ------------------------------------------------------------------------------------------------- 3. rollout_legs, row by row
def _roll(idx, table, land="rule", drive=None, ground=None, inertia=None):
    pb, rows = legsim_cases.rollout_batch()
    pb = dict(pb, legs=np.zeros((ROLL_B, 4, 7)))
    a = [pb[k][idx] for k in ("x", "ref", "feet", "legs", "gait", "stand", "gain", "tick", "mu")]
    kw = {k: rows[k][idx] for k in ("body", "push", "push_ticks")}
    if table is not None:
        kw["actuators"] = table[idx]
    height = np.full(len(a[0]), legsim_cases.STEP_HEIGHT)
    if drive is None:
        return gaits.rollout_legs_host(ac.checker_engine(), *a, ROLL_T, height, land=land, inertia=inertia, **kw)
    return gaits.rollout_drive_host(ac.checker_engine(), *a, ROLL_T, height, land=land, drive=drive, ground=None if ground is None else ground[idx],
                                    inertia=inertia, **kw)


def test_rollout_legs_with_mixed_rows_is_the_uniform_runs(oracle_lib):
    table = ac.rollout_rows()
    mixed = _roll(np.arange(ROLL_B), table, land="actual")
    for c, (scale, knee, free) in enumerate(ac.CLASSES):
        idx = np.arange(c, ROLL_B, 4)
        if np.isinf(knee):
            ref = _roll(idx, None, land="actual", inertia=dc.weak_row(scale))
        else:
            ref = _roll(idx, ac.rows_of((ac.CLASSES[c],), ROLL_B), land="actual")
        for k in ref:
            assert _same(mixed[k][idx], ref[k]), (c, k)
    up = mixed["contact_log"] == 0
    cl = ((mixed["flag"] & 2) != 0) & (mixed["flag"] != 0xff)
    cls = np.arange(ROLL_B) % 4
    per = [int((cl & up)[cls == c].sum()) for c in range(4)]
    print(f"rollout_legs(actual) with mixed rows: clamped swing rows per class {per}; solved {mixed['solved'].tolist()}")
    assert per[2] > 0 and per[3] > 0 and per[0] == 0 and not (cl & ~up).any() and np.all(mixed["solved"] == ROLL_T)


def test_the_ideal_drive_clamps_swing_rows_only(oracle_lib):
    idx = np.arange(8)
    ground = np.where(np.arange(ROLL_B) % 2 == 0, dc.GROUND_MU, 1e3)
    with_table = _roll(idx, ac.rollout_rows(), drive="ideal", ground=ground)
    without = _roll(idx, None, drive="ideal", ground=ground)
    up = with_table["contact_log"] == 0
    cl = ((with_table["flag"] & 2) != 0) & (with_table["flag"] != 0xff)
    cls = idx % 4
    print(f"ideal drive on slippery ground: clamped swing rows per class {[int((cl & up)[cls == c].sum()) for c in range(4)]}, "
          f"ground-limited stance rows {int((((with_table['flag'] & 32) != 0) & ~up).sum())}")
    assert not (cl & ~up).any() and (cl & up)[cls == 2].sum() > 0 and (((with_table["flag"] & 32) != 0) & ~up).sum() > 0
    for k in with_table:
        assert _same(with_table[k][cls == 0], without[k][cls == 0]), k          # the flat Lite3 row is no row
    assert not _same(with_table["q"][cls == 2][up[cls == 2]], without["q"][cls == 2][up[cls == 2]])


# ------------------------------------------------------------------------------------- 4. models, actuators and ground in one call
def test_three_tables_in_one_call_are_sixteen_live_combinations(oracle_lib):
    pb, pr, rows, T = C.legs_case()
    act, ground, acls = ac.combined_tables()
    B = C.LEGS_B
    combos = {(tuple(rows[b]), tuple(act[b]), float(ground[b])) for b in range(B)}
    assert len(combos) == B == 16 and len(np.unique(rows, axis=0)) == 4 and np.array_equal(rows[:4], rows[4:8])
    assert len(np.unique(act, axis=0)) == 4 and np.array_equal(act[0], act[3]) and not np.array_equal(act[3], act[4])
    h = ac.combined_host()
    fl, st = h["flag"], h["contact_log"] != 0
    live = fl != 0xff
    cl = ((fl & 2) != 0) & live
    gl = ((fl & 32) != 0) & live & st
    near = ((h["margin"] <= legsim_cases.FLAG_MARGIN) | (h["drive_margin"] <= legsim_cases.FLAG_MARGIN)) & live
    swing_robots, stance_robots = (cl & ~st).any(axis=(1, 2)), (cl & st).any(axis=(1, 2))
    print(f"three tables: solved {h['solved'].tolist()}, lowest CoM {h['actual'][:, :, 5].min():.3f} m, ground-limited robots "
          f"{np.nonzero(gl.any(axis=(1, 2)))[0].tolist()}, swing rows clamped on {int(swing_robots.sum())} robots, stance rows on "
          f"{int(stance_robots.sum())}; {int(near.sum())} of {near.size} entries within FLAG_MARGIN")
    assert np.all(h["solved"] == T) and live.all() and h["actual"][:, :, 5].min() > 0.2
    assert np.array_equal(gl.any(axis=(1, 2)), np.arange(B) % 2 == 0)
    curved = np.isfinite(act[:, 3])
    assert swing_robots[curved].sum() >= 4 and not swing_robots[acls == 0].any() and stance_robots.sum() >= 2
    assert near.mean() <= dc.MARGIN_SHARE
    assert (h["cmd"] != h["forces"]).any()
    # the commanded forces replay as independent QPs under the model table tiled, and the tight checker solves every one of them
    u0, solved = _replayed_u0(h, pb, rows, T)
    assert np.array_equal(u0, h["cmd"]) and np.array_equal(solved, h["solved"])
    ops = M.replay_rows(h, pb, pb["tick"], pb["x"][:, 12])
    assert np.all(C.replay_reference(ops, np.repeat(rows, T, axis=0))[1]["status"] == 1)


# ------------------------------------------------------------------------------------ 5. an invalid row inside a roll-out
@pytest.mark.parametrize("mode", range(len(ac.LOOP_MODES)), ids=[m[0] for m in ac.LOOP_MODES])
def test_an_invalid_row_inside_a_rollout(oracle_lib, mode):
    name, drive, land = ac.LOOP_MODES[mode]
    assert dc.loop_batch()["names"][ac.INVALID_IN_LOOP] == "walk" and not actuators.valid_rows(ac.loop_rows())[ac.INVALID_IN_LOOP]
    assert actuators.valid_rows(ac.loop_rows(False)).all() and actuators.valid_rows(ac.loop_rows()).sum() == dc.LOOP_B - 1
    bad, good = ({k: v[0] for k, v in ac.loop_host(mode, inv).items()} for inv in (True, False))
    T = dc.LOOP_T
    assert good["solved"] == T and np.isfinite(good["actual"]).all() and not np.any(good["flag"] == 0xff)
    up, landing = ac.swing_and_landing_rows(good["contact_log"])
    ff = bad["flag"] == 0xff
    nan = {k: np.isnan(bad[k]).reshape(T, 4, -1) for k in KNOWN_LOGS}
    for k in KNOWN_LOGS:                                                        # a row is NaN in every entry of every leg log, or in none
        assert np.array_equal(nan[k].all(axis=-1), ff) and np.array_equal(nan[k].any(axis=-1), ff), k
    first = ac.first_nonfinite_tick(bad["actual"])
    print(f"invalid row, {name}: {int(up.sum())} swing rows, {int(landing.sum())} landing rows, {int(ff.sum())} rows 0xff, actual non-finite from tick "
          f"{first}, solved {int(bad['solved'])}, miss NaN on {int(np.isnan(bad['miss']).sum())} rows")
    assert up.sum() >= 20 and landing.sum() >= 5 and (~up & ~landing).sum() >= 20
    if land == "rule":
        for k in ("x", "ref", "feet", "tick", "actual", "desired", "forces", "feet_log", "contact_log", "swing", "solved"):
            assert _same(bad[k], good[k]), k
        assert np.array_equal(ff, up | landing)
        assert np.array_equal(np.isnan(bad["miss"]), good["miss"] != 0.0) and np.isnan(bad["miss"]).sum() >= 5
        keep = ~ff
        for k in KNOWN_LOGS + ("flag",):
            assert _same(bad[k][keep], good[k][keep]), k
    elif drive == "limited":
        assert ff.all() and first == 1 and bad["solved"] == 1 and np.isfinite(bad["cmd"][0]).all()
    else:
        # land = actual without a drive: the first landing puts the NaN into feet, the solve of the landing tick reports NONFINITE, its
        # row is 0xff on every leg and the plant carries the NaN into x: swing rows only before that tick, everything from it on
        t_land = int(np.nonzero(landing.any(axis=1))[0][0])
        assert np.array_equal(ff[:t_land], up[:t_land]) and ff[t_land:].all() and 1 <= t_land and first == t_land + 1 < ac.LOOP_HOST_T - 1
        assert not np.isfinite(bad["actual"][first:]).all(axis=-1).any() and bad["solved"] == t_land
        assert np.array_equal(bad["contact_log"], good["contact_log"])
        short = {k: v[0] for k, v in ac.loop_host(mode, True, ac.LOOP_HOST_T).items()}
        for k in KNOWN_LOGS + ("flag", "actual", "miss", "forces", "feet_log"):   # the short loop a device test runs is this one's head
            assert _same(short[k], bad[k][:ac.LOOP_HOST_T]), k
        assert short["solved"] == bad["solved"]
