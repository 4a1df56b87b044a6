"""The conditions of tests/test_gpu_slip_rows.py on the CPU checker, no GPU (include/mpcqp_slip.h; the cases are in
tests/slip_rows_cases.py): what makes each device comparison discriminating is asserted here from the host counterparts alone.

  1. models.rollout_slip_models_host is gaits.rollout_slip_host per robot, with ground, foot mass, slip state and actuator rows
     sub-indexed.
  2. The combined case: every tick solves, nobody falls, feet slide on the low-friction robots, stance and swing rows clamp, the feet
     follow the displacements, and the host replay through stance_slip_host with all four tables tiled is exact.
  3. The envelope's rate depends on s0: the moving stance legs whose applied torque moves by more than 1e-3 N m when the envelope is
     read at the foot-at-rest rate, on the combined case and on the draw; and the rule with s0 left out of the rate, applied through the
     host function's own arguments, fails the device comparison, host against host.
  4. The margin share of the draw in both I/O roundings and of the combined case's replayed rows.
  5. The growth factor of the draw, measured here and stored in tests/golden/slip_rows_growth.npz.
  6. The combined case at a second substep count: it solves, replays exactly at that count and not at the default.

The figures printed here are quoted by the documents; the tests assert floors and directions, not those values."""
import numpy as np
import pytest

import actuator_cases as ac
import drive_cases as dc
import legsim_cases
import models_rollout_cases as C
import mpcqp
import slip_cases as sc
import slip_rows_cases as rc
from legsim_cases import DELTA
from mpcqp import gaits, lite3_model
from mpcqp import models as M
from test_gpu_stance_drive import _error
from test_models_rollouts_host import _replayed_u0


def _same(a, b):
    return np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind == "f")


def _rows(a):
    return a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])


# ------------------------------------------------------------------------------------------------------------- 1. the host variant
def test_the_grouped_loop_is_rollout_slip_host_per_robot(oracle_lib):
    K = rc.combined_case()
    pb, pr, T = K["pb"], K["pr"], 5
    whole = rc.combined_host()
    for b in (3, 6, 12):                                                        # an odd and two even robots of three model classes
        idx = np.array([b])
        eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config(**C.LOOP_KW, **M.row_overrides(K["rows"][b])))
        one = gaits.rollout_slip_host(eng, *[pb[k][idx] for k in C.LEGS_ARGS], T, pb["step_height"][idx], K["ground"][idx], K["foot_mass"][idx],
                                      K["slip"][idx], land="actual", drive="limited", actuators=K["act"][idx], **{k: v[idx] for k, v in pr.items()})
        for k in ("actual", "desired", "forces", "cmd", "feet_log", "contact_log", "q", "qd", "tau", "flag", "miss", "slip_log", "disp"):
            assert _same(one[k][0], whole[k][b, :T]), (b, k)
    # a number for the foot mass and no start state are the loop's own defaults; ground and foot_mass are required
    sub = np.arange(4)
    a = [pb[k][sub] for k in C.LEGS_ARGS]
    cut = {k: v[sub] for k, v in pr.items()}
    uniform = np.tile(K["rows"][1], (4, 1))
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config(**C.LOOP_KW, **M.row_overrides(K["rows"][1])))
    got = M.rollout_slip_models_host(oracle_lib, C.LOOP_KW, uniform, *a, 3, pb["step_height"][sub], K["ground"][sub], 0.3, **cut)
    ref = gaits.rollout_slip_host(eng, *a, 3, pb["step_height"][sub], K["ground"][sub], 0.3, **cut)
    assert set(got) == set(ref)
    for k in ref:
        assert _same(got[k], ref[k]), k
    with pytest.raises(ValueError, match="needs ground and foot_mass"):
        M.rollout_slip_models_host(oracle_lib, C.LOOP_KW, uniform, *a, 1, pb["step_height"][sub], None, 0.3)


# ------------------------------------------------------------------------------------------------------------ 2. the combined case
def test_the_combined_case_is_sixteen_live_sliding_combinations(oracle_lib):
    K = rc.combined_case()
    pb, rows, T, B = K["pb"], K["rows"], K["T"], C.LEGS_B
    me, s0 = K["foot_mass"], K["slip"]
    assert len(set(me.tolist())) == B and me.min() >= sc.MASS_LO and me.max() <= sc.MASS_HI and not np.all(np.diff(me) > 0)
    assert len({(tuple(rows[b]), tuple(K["act"][b]), float(K["ground"][b])) for b in range(B)}) == B
    assert rc.LOW_MU != sc.ICE and np.array_equal(K["ground"] < 1.0, np.arange(B) % 2 == 0)
    speed = np.linalg.norm(s0, axis=-1)
    assert 0 < speed.max() < 0.9 and rc.START_SPEED < 0.3 and (speed > 0).sum() >= B
    h = rc.combined_host()
    n = rc.counts(h, K)
    st = h["contact_log"] != 0
    on_swing, on_stance = rc.start_on_swing(K, h["contact_log"]), s0.any(axis=-1) & st[:, 0]
    print(f"combined slip case: solved {h['solved'].tolist()}, lowest CoM {h['actual'][:, :, 5].min():.3f} m, {n}; start entries on "
          f"{int(on_stance.sum())} stance and {int(on_swing.sum())} swing legs; largest |slip_log| {np.abs(h['slip_log']).max():.2f} m/s, "
          f"largest |disp| {np.abs(h['disp']).max():.4f} m")
    assert np.all(h["solved"] == T) and n["dead"] == 0
    assert h["actual"][:, :, 5].min() > 0.2
    assert n["low-friction robots"] == 8 and n["sliding low-friction robots"] >= 6
    assert n["clamped stance"] > 0 and n["clamped swing"] > 0
    curved = np.isfinite(K["act"][:, 3])                                        # swing rows clamped under a falling curve, not a flat box
    assert (((h["flag"] & 2) != 0) & (h["flag"] != 0xff) & ~st)[curved].sum() > 0 and curved.sum() == 8
    assert on_swing.sum() >= 3 and on_stance.sum() >= 3
    assert sc.foot_move_holds(h["feet_log"], h["contact_log"], h["disp"], pb["gait"], pb["tick"])
    # the replay through the rule alone, the four tables tiled
    o = rc.replay_host(h, K)
    assert np.array_equal(o["f"], _rows(h["forces"])) and np.array_equal(o["disp"], _rows(h["disp"]))
    assert np.array_equal(o["tau"][_rows(st)], _rows(h["tau"])[_rows(st)])
    # a start entry on a swing leg is logged as given and is gone on the next row; the state chain is the rule's
    assert np.array_equal(h["slip_log"][:, 0], s0) and not h["slip_log"][:, 1][on_swing].any()
    end = o["slip"].reshape(B, T, 4, 2)
    for t in range(1, T + 1):
        td = gaits.touchdown_mask(pb["gait"], pb["tick"] + t)
        nxt = h["slip_log"][:, t] if t < T else h["slip"]
        assert np.array_equal(nxt[~td], end[:, t - 1][~td]) and not nxt[td].any(), t
    # each table matters: another robot's value changes the rows of the rule
    for name, pos in (("ground", 4), ("foot_mass", 5), ("actuators", 7)):
        ops = list(rc.replay_operands(h, K))
        ops[pos] = np.roll(ops[pos], T, axis=0)
        x, f, feet, contact, ground, fm, s_in, act = ops
        w = lite3_model.stance_slip_host(x, f, feet, contact, ground, fm, s_in, actuators=act, delta=DELTA)
        moved = int((np.abs(w["f"] - o["f"]).reshape(B, T, -1).max(axis=(1, 2)) > 1e-6).sum())
        print(f"combined slip case: the next robot's {name} moves the applied forces of {moved} robots")
        assert moved >= 2, name
    # the commanded forces replay as independent QPs under the model table tiled
    u0, solved = _replayed_u0(h, pb, rows, T)
    assert np.array_equal(u0, h["cmd"]) and np.array_equal(solved, h["solved"])


# ------------------------------------------------------------------------------------------------------- 3. s0 in the envelope's rate
def test_the_combined_case_reads_the_envelope_at_the_moving_foots_rate(oracle_lib):
    K = rc.combined_case()
    h = rc.combined_host()
    o = rc.replay_host(h, K)
    x, f, feet, contact, ground, me, s0, act = rc.replay_operands(h, K)
    moving = s0.any(axis=-1) & (contact != 0)
    sens = rc.s0_sensitive(o["tau_cmd"], o["rate"], rc.rest_rate(x, f, feet, contact, ground, act), act, moving)
    print(f"combined slip case: {int(moving.sum())} moving stance leg-rows, {int(sens.sum())} of them s0-sensitive "
          f"(robots {sorted(set((np.nonzero(sens)[0] // K['T']).tolist()))})")
    assert sens.sum() >= rc.S0_LEGS


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_draw_reads_the_envelope_at_the_moving_foots_rate(dtype):
    c = rc.as_io(rc.rows_draw(), dtype)
    o = rc.slip(c)
    st = c["contact"] != 0
    moving = c["slip"].any(axis=-1) & st
    rest = rc.rest_rate(c["x"], c["f"], c["feet"], c["contact"], c["ground"], c["rows"])
    sens = rc.s0_sensitive(o["tau_cmd"], o["rate"], rest, c["rows"], moving)
    near = dc.near_threshold(o)
    b = ac.INVALID_ROBOT
    print(f"slip draw with a table, {np.dtype(dtype).name}: {int(moving.sum())} moving stance legs of {int(st.sum())}, {int(sens.sum())} "
          f"s0-sensitive, {int(near.sum())} within FLAG_MARGIN, smallest margin {o['margin'][st & (o['flag'] != 0xff)].min():.2e}")
    assert sens.sum() >= rc.S0_LEGS and moving.sum() >= 30
    assert near.sum() <= dc.MARGIN_SHARE * st.sum()
    # at rest the rule reads the drive's rate; a moving foot's rate is another one
    o0 = rc.slip(dict(c, slip=np.zeros_like(c["slip"])))
    assert np.array_equal(o0["rate"], rest) and np.all((o["rate"] != rest).any(axis=-1)[moving & (o["reach"] != 0)])
    assert np.array_equal(o["rate"][~moving], rest[~moving])
    # robot 13's row is invalid: its stance legs are poisoned, its swing legs and everybody else are not
    assert st[b].any() and np.all(o["flag"][b][st[b]] == 0xff) and not np.any(np.delete(o["flag"], b, axis=0) == 0xff)
    assert np.isnan(o["slip"][b][st[b]]).all() and np.isnan(o["disp"][b][st[b]]).all() and not o["flag"][b][~st[b]].any()
    # the same call without s0: other torques on the moving legs (a pull delivers 0 either way), the same bits on the legs at rest
    other = rc.tau_moves_without_s0(o, o0, moving)
    print(f"slip draw with a table, {np.dtype(dtype).name}: slip = 0 changes the torque of {int(other.sum())} moving legs, {int((other & sens).sum())} "
          f"of them s0-sensitive")
    assert (other & sens).sum() >= rc.S0_LEGS
    at_rest = ~c["slip"].any(axis=-1)
    for k in ("tau", "flag", "slip", "disp"):
        assert _same(o[k][at_rest], o0[k][at_rest]), k


def test_the_rule_without_s0_in_the_rate_fails_the_device_comparison():
    """The mutation: the envelope read at the foot-at-rest rate, everything else the rule's.  slip_rows_cases.rule_with_rate builds it
    from stance_slip_host's own arguments; with the moving foot's rate the construction is stance_slip_host bit for bit."""
    c = rc.rows_draw()
    host = rc.slip(c)
    st = c["contact"] != 0
    a = [c[k] for k in ("x", "f", "feet", "contact", "ground", "foot_mass", "slip", "rows")]
    f_in = c["f"].reshape(-1, 4, 3)
    scale = rc.band_scale()
    own = rc.rule_with_rate(*a, host["rate"], delta=DELTA)
    live = st & (host["flag"] != 0xff)
    assert np.array_equal(own["f"][live], host["f"].reshape(-1, 4, 3)[live])
    for k in ("tau", "flag", "slip", "disp"):
        assert np.array_equal(own[k][live], host[k][live]), k
    assert np.all(own["flag"][st & ~live] == 0xff)
    full = lambda r: {"f": np.where(st[..., None], r["f"], f_in), "tau": r["tau"], "flag": np.where(st, r["flag"], 0).astype(np.uint8),
                      "slip": r["slip"], "disp": r["disp"]}
    rc.compare_with_host("the construction itself", "f64", full(own), host, f_in, c["foot_mass"], st, scale, _error)
    mutant = full(rc.rule_with_rate(*a, rc.rest_rate(*a[:5], c["rows"]), delta=DELTA))
    with np.errstate(invalid="ignore"):
        differ = live & ((np.abs(mutant["tau"] - host["tau"]).max(axis=-1) > dc.F64_BAND * scale) | (mutant["flag"] != host["flag"]))
    print(f"the rule without s0 in the rate: {int(differ.sum())} of {int(live.sum())} live stance legs differ from the host by more than the band "
          f"({dc.F64_BAND:.0e} x {scale:.2f}); largest torque difference {np.nanmax(np.abs(mutant['tau'] - host['tau'])[live]):.3f} N m")
    assert differ.sum() >= rc.S0_LEGS
    with pytest.raises(AssertionError):
        rc.compare_with_host("the rule without s0 in the rate", "f64", mutant, host, f_in, c["foot_mass"], st, scale, _error)


# ------------------------------------------------------------------------------------------------------------- 4. the margin share
def test_the_replayed_rows_keep_clear_of_the_thresholds(oracle_lib):
    K = rc.combined_case()
    h = rc.combined_host()
    o = rc.replay_host(h, K)
    st = _rows(h["contact_log"]) != 0
    near = dc.near_threshold(o)
    print(f"combined slip case: {int(near.sum())} of {int(st.sum())} replayed stance leg-rows within {legsim_cases.FLAG_MARGIN:g} of a threshold")
    assert near.sum() <= dc.MARGIN_SHARE * st.sum()


# ------------------------------------------------------------------------------------------------------------ 5. the growth factor
def test_the_recorded_growth_factor_is_the_hosts_own():
    got, rec = rc.draw_growth(), rc.recorded_growth()
    print(f"growth factor of the slip draw with a table: {got:.2f} (recorded {rec['draw']:.2f}; the drive's draw {ac.recorded_growth()['draw']:.2f})")
    assert set(rec) == {"draw"}
    assert 1.0 <= rec["draw"] < 1e3 and abs(got - rec["draw"]) <= 0.02 * rec["draw"]


# ------------------------------------------------------------------------------------------------------ 6. another substep count
def test_the_combined_case_at_another_substep_count(oracle_lib):
    K = rc.combined_case()
    n = rc.SECOND_SUBSTEPS
    h = rc.combined_host(n)
    print(f"combined slip case, substeps {n}: solved {h['solved'].tolist()}, lowest CoM {h['actual'][:, :, 5].min():.3f} m, {rc.counts(h, K)}")
    assert n not in (0, 10) and np.all(h["solved"] == K["T"]) and not np.any(h["flag"] == 0xff)
    own, other = rc.replay_host(h, K, substeps=n), rc.replay_host(h, K, substeps=10)
    assert np.array_equal(own["f"], _rows(h["forces"])) and np.array_equal(own["disp"], _rows(h["disp"]))
    assert not np.array_equal(other["f"], _rows(h["forces"])) and not np.array_equal(other["disp"], _rows(h["disp"]))
    assert not np.array_equal(h["forces"], rc.combined_host()["forces"])
