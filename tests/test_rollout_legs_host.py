"""The host counterpart of mpcqp_rollout_legs (gaits.rollout_legs_host; include/mpcqp_sim.h) on the CPU checker, no GPU: land = rule is
rollout_phase_host + phase_swing_host + swing_track_host exactly; land = actual lands every foot where its leg put it; the one-row
growth the device test's replay band is multiplied by; and the 60-tick report of what landing on the delivered foot does to each
named gait, which DESIGN.md quotes."""
import numpy as np
import pytest

import mpcqp
from legroll_cases import (LEG_LOGS, PHASE_LOGS, REPORT_T, ROW_GROWTH_NPZ, gait_report, host_loop, landings, measure_row_growth, replay_rows,
                           report_lines)
from legsim_cases import DELTA, ROLL_B, ROLL_T, STEP_HEIGHT, flag_margins
from mpcqp import gaits, lite3_model


def _same(a, b):
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# --------------------------------------------------------------------------------------------------- 1. land = rule is the three calls
def test_land_rule_is_the_three_host_calls(oracle_lib):
    pb, rows, o = host_loop("rule")
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config(N=10, delta=DELTA, max_iter=4000))
    ref = gaits.rollout_phase_host(eng, pb["x"], pb["ref"], pb["feet"], pb["gait"], pb["stand"], pb["gain"], pb["tick"], pb["mu"], ROLL_T,
                                   rows["body"], rows["push"], rows["push_ticks"])
    for k in ("x", "ref", "tick", "feet") + PHASE_LOGS:
        assert _same(o[k], ref[k]), k
    sw = gaits.phase_swing_host(ref["actual"], ref["desired"], ref["feet_log"], pb["gait"], pb["tick"], pb["stand"], pb["gain"],
                                np.full(ROLL_B, STEP_HEIGHT), DELTA)["swing"]
    assert _same(o["swing"], sw)
    wr = gaits.log_wrench(rows["push"], rows["push_ticks"], pb["tick"], ROLL_T)
    assert (np.abs(wr).max(axis=(1, 2)) > 0).sum() == 2                         # the two pushed robots
    acc = lite3_model.plant_base_acc_host(ref["actual"], ref["forces"], ref["feet_log"], rows["body"], wrench=wr)
    trk = lite3_model.swing_track_host(ref["actual"], ref["forces"], ref["feet_log"], ref["contact_log"], sw, acc, delta=DELTA)
    for k in ("q", "qd", "tau", "foot", "err", "flag"):
        assert _same(o[k], trk[k]), k
    assert _same(o["legs"], trk["state"])
    # the miss of a landing is the err of the landing row one tick on, and nothing else is a miss
    td = landings(o["contact_log"])
    assert td.sum() >= 2 * 14 and np.all(o["miss"][:, :-1][~td[:, :-1]] == 0.0)
    assert np.abs(o["miss"][:, :-1][td[:, :-1]] - o["err"][:, 1:][td[:, :-1]]).max() <= 1e-12
    print(f"landing misses of the land = rule loop: {np.round(o['miss'][td].min() * 1e3, 2)} to {np.round(o['miss'][td].max() * 1e3, 2)} mm")
    # the flag cap of the device test holds on this case with room to spare, for both landings
    for land in ("rule", "actual"):
        r = host_loop(land)[2]
        near = flag_margins(r)
        print(f"land = {land}: {int(near.sum())} of {near.size} (robot, tick, leg) within 1e-9 of a flag threshold; smallest margin {r['margin'].min():.3e}")
        assert near.sum() == 0 and not np.any(r["flag"] == 0xff)


def test_wrench_argument_of_the_base_acceleration():
    pb, rows, o = host_loop("rule")
    a = (o["actual"], o["forces"], o["feet_log"], rows["body"])
    plain = lite3_model.plant_base_acc_host(*a)
    assert _same(plain, lite3_model.plant_base_acc_host(*a, wrench=None))
    assert np.abs(plain - lite3_model.plant_base_acc_host(*a, wrench=np.zeros((ROLL_B, ROLL_T, 6)))).max() == 0.0
    wr = gaits.log_wrench(rows["push"], rows["push_ticks"], pb["tick"], ROLL_T)
    pushed = lite3_model.plant_base_acc_host(*a, wrench=wr)
    on = np.abs(wr).max(axis=2) > 0
    assert on.sum() >= 2 and _same(pushed[~on], plain[~on])
    m = rows["body"][:, 0][:, None, None]
    assert np.abs((pushed - plain)[..., 3:6] - wr[..., 0:3] / m).max() <= 1e-12  # a force at the CoM: F / m, whatever the rest


# --------------------------------------------------------------------------------------------------------- 2. land = actual identities
def test_land_actual_lands_where_the_leg_put_the_foot():
    pb, rows, o = host_loop("actual")
    rule = host_loop("rule")[2]
    B, T = ROLL_B, ROLL_T
    after, _ = replay_rows(o, pb, rows, pb["tick"])
    up = o["contact_log"] == 0
    both = up[:, :-1] & up[:, 1:]
    assert both.sum() > 100
    assert np.abs(after[:, :-1, :, 0:3][both] - o["q"][:, 1:][both]).max() == 0.0 and np.abs(after[:, :-1, :, 3:6][both] - o["qd"][:, 1:][both]).max() == 0.0
    assert _same(after[:, -1], o["legs"])
    nxt = np.concatenate([o["actual"][:, 1:], o["x"][:, None, :12]], axis=1)
    feet_nxt = np.concatenate([o["feet_log"][:, 1:], o["feet"][:, None]], axis=1)
    td = np.stack([gaits.touchdown_mask(pb["gait"], pb["tick"].astype(np.int64) + t + 1) for t in range(T)], axis=1)
    assert np.array_equal(td[:, :-1], landings(o["contact_log"])[:, :-1]) and td.sum() >= 2 * 14
    flat = lambda a: a.reshape((B * T,) + a.shape[2:])
    rep = lambda a: np.repeat(np.asarray(a), T, axis=0)
    p_act = gaits.leg_feet_host(flat(nxt), flat(after)).reshape(B, T, 4, 3)
    foothold = gaits.touchdown_foothold(flat(nxt)[:, 3:6], gaits.measured_yaw(flat(nxt)[:, 0:3]), flat(nxt)[:, 9:12], flat(o["desired"])[:, 9:12],
                                        rep(pb["stand"]), rep(pb["gain"]), rep(pb["gait"]), DELTA).reshape(B, T, 4, 3)
    assert np.array_equal(feet_nxt[td][:, :2], p_act[td][:, :2])
    assert np.array_equal(feet_nxt[td][:, 2], np.broadcast_to(pb["stand"][:, None, :, 2], (B, T, 4))[td])
    assert np.abs(o["miss"][td] - np.linalg.norm(p_act - foothold, axis=-1)[td]).max() <= 1e-12 and np.all(o["miss"][~td] == 0.0)
    assert np.array_equal(feet_nxt[~td], o["feet_log"][~td])
    rfeet = np.concatenate([rule["feet_log"][:, 1:], rule["feet"][:, None]], axis=1)
    moved = np.linalg.norm((feet_nxt - rfeet)[..., :2], axis=-1)
    steps = td.any(axis=(1, 2))
    worst = np.array([moved[b][td[b]].max() if steps[b] else 0.0 for b in range(B)])
    print(f"landed feet against the land = rule loop: largest xy difference per robot {np.round(worst * 1e3, 2)} mm")
    assert steps.sum() == 14 and np.all(worst[steps] > 1e-3) and np.all(worst[~steps] == 0.0)     # millimetres; the two standing robots: none
    first = np.array([np.nonzero(td[b].any(axis=1))[0][0] if steps[b] else T for b in range(B)])
    for b in range(B):                                                          # up to and including the row of the first landing the loops are one
        assert _same(o["actual"][b, :first[b] + 1], rule["actual"][b, :first[b] + 1]), b
    assert not _same(o["actual"][steps], rule["actual"][steps])
    with pytest.raises(ValueError, match="land"):
        gaits.rollout_legs_host(None, *([None] * 9), 1, None, land="where")


def test_row_growth_is_the_recorded_one():
    g = measure_row_growth()
    rec = float(np.load(ROW_GROWTH_NPZ)["growth"])
    print(f"growth of a 1e-10 perturbation of a row's start state over the row: {g:.3f} (recorded {rec:.3f})")
    assert g < 1e3 and abs(g - rec) <= 1e-3 * rec


# ------------------------------------------------------------------------------------------------------------------------- 3. the report
def test_report_of_actual_landings_per_gait():
    """What landing on the delivered foot does to the closed loop, per named gait over 60 ticks on the CPU checker (one robot per gait,
    period 12, unpushed), at the Lite3's torque limits and at half of them.  Only what the loop shows is asserted:
      - every solve of every gait is solved, with either landing and either limit: no gait stops solving on its delivered feet;
      - at the default limits no swing row clamps a torque, so halving the limits changes nothing for a gait that stays below half
        of them -- all but the walk, whose 3-tick swings do not: its legs saturate, and with actual landings the worst landing
        miss grows from 61 mm to more than 200 mm while the MPC still solves every tick;
      - a land = rule loop does not see the legs at all: its solved counts and heights are the same at both limits."""
    full, half = gait_report(1.0), gait_report(0.5)
    for scale, rep in ((1.0, full), (0.5, half)):
        print("\n".join(report_lines(rep, scale)))
    names = list(full["rule"])
    for rep in (full, half):
        for land in ("rule", "actual"):
            assert all(rep[land][n][0] == REPORT_T for n in names), land
            assert all(np.isfinite(rep[land][n][1:4]).all() for n in names)
        assert rep["rule"]["stand"][3] == 0.0 and rep["actual"]["stand"] == rep["rule"]["stand"]     # never lifts: nothing to land
    assert all(full["rule"][n][:3] == half["rule"][n][:3] for n in names)
    assert all(full[land][n][4] == 0 for land in ("rule", "actual") for n in names)
    quiet = [n for n in names if half["actual"][n][4] == 0 and half["rule"][n][4] == 0]
    assert set(names) - set(quiet) == {"walk"} and all(half[land][n] == full[land][n] for land in ("rule", "actual") for n in quiet)
    assert half["actual"]["walk"][3] > 0.2 > 0.1 > full["actual"]["walk"][3]
    moved = [n for n in names if full["actual"][n][2] != full["rule"][n][2]]
    print(f"gaits whose RMS height error changes with actual landings: {moved}")
    assert set(moved) == set(names) - {"stand"}
