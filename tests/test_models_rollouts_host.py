"""The host side of per-robot model rows through the roll-outs (mpcqp.models, tests/models_rollout_cases.py), without a GPU: the
grouped checker against a single handle, the replay of a roll-out's logs as independent QPs against the loop that wrote them, and
the figures that make the GPU comparison of tests/test_gpu_models_rollouts.py discriminating."""
import numpy as np
import pytest

import drive_cases
import models_rollout_cases as C
import mpcqp
from conftest import rel_err
from mpcqp import gaits
from mpcqp import models as M

PLAN_ARGS = ("x", "ref", "plan_pos", "plan_feet_id", "plan_meta", "tick", "mu")


def _same(a, b, keys=None):
    for k in keys or a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _replayed_u0(logs, pb, rows, T):
    """Stage-0 forces of the replayed rows on checker handles of the loop's own configuration, as [B,T,12], and the solved count."""
    ops = M.replay_rows(logs, pb, pb["tick"], pb["x"][:, 12])
    e = gaits.phase_expand_host(ops["x"], ops["ref"], ops["feet"], ops["gait"], ops["tick"], ops["stand"], ops["gain"], 10, 0.03)
    o = M.solve_batch_models_host(C.oracle_lib(), C.LOOP_KW, np.repeat(rows, T, axis=0),
                                  {"x0": ops["x"], "r": e["r"], "contact": e["contact"], "xdes": e["xdes"], "mu": ops["mu"]}, want_X=False)
    B = len(rows)
    return o["u"][:, 0].reshape(B, T, 12), np.isin(o["status"], (1, 2)).reshape(B, T).sum(axis=1)


def test_rows_of_the_case():
    rows = C.model_rows(24)
    assert rows.shape == (24, 6) and len(np.unique(rows, axis=0)) == C.CLASSES and np.array_equal(rows[:4], rows[4:8])
    assert np.all(rows[:, 0] >= 0.8 * 8.885) and np.all(rows[:, 0] <= 1.4 * 8.885)
    last = np.arange(24) % 4 == 3
    assert np.all(rows[~last, 5] == 100.0) and np.array_equal(rows[last, 5], 0.6 * rows[last, 0] * C.G)
    assert np.all(2.0 * rows[last, 5] > rows[last, 0] * C.G)        # two legs carry the robot, at 5/6 of their bound
    body = C.matched_bodies(rows)
    assert np.array_equal(M.models_from_bodies(body, rows[:, 4], rows[:, 5]), rows)


def test_replay_reproduces_the_phase_loop_exactly():
    pb, pr, rows, T = C.phase_case()
    h = C.host_phase()
    u0, solved = _replayed_u0(h, pb, rows, T)
    assert np.array_equal(u0, h["forces"]) and np.array_equal(solved, h["solved"])
    ops = M.replay_rows(h, pb, pb["tick"], pb["x"][:, 12])
    assert ops["x"].shape == (24 * T, 13) and ops["tick"].dtype == np.int32 and np.array_equal(ops["tick"][:T], np.arange(T))
    assert np.array_equal(ops["x"][:T, :12], h["actual"][0]) and np.array_equal(ops["feet"][T:2 * T], h["feet_log"][1])
    assert np.array_equal(ops["gait"][T], pb["gait"][1]) and ops["gain"].shape == (24 * T,)
    assert M.replay_rows(h, dict(pb, gain=None), pb["tick"], -9.81)["gain"] is None


def test_phase_case_is_not_vacuous_and_a_wrong_row_is_far_outside_the_band():
    pb, pr, rows, T = C.phase_case()
    h = C.host_phase()
    assert np.all(h["solved"] == T) and h["actual"][:, :, 5].min() > 0.25
    assert C.reaches_upper_bound(h["forces"], h["contact_log"], rows, 1e-9).all()
    assert np.all(h["forces"].reshape(24, T, 4, 3)[..., 2] <= rows[:, 5][:, None, None] + 1e-9)
    assert (h["contact_log"].sum(axis=2) == 0).any() and np.any(pr["push"] != 0)
    ops = M.replay_rows(h, pb, pb["tick"], pb["x"][:, 12])
    tiled = np.repeat(rows, T, axis=0)
    batch, ref = C.replay_reference(ops, tiled)
    assert np.all(ref["status"] == 1)
    stance = batch["contact"].reshape(24 * T, -1).any(axis=1)
    nb = M.solve_batch_models_host(C.oracle_lib(), C.TIGHT_KW, np.repeat(np.roll(rows, 1, axis=0), T, axis=0), batch, want_X=False)
    cf = M.solve_batch_models_host(C.oracle_lib(), C.TIGHT_KW, M.model_rows(C.oracle_lib().default_config(**C.TIGHT_KW), 24 * T), batch,
                                   want_X=False)
    e_nb, e_cf = rel_err(nb["u"], ref["u"]), rel_err(cf["u"], ref["u"])
    print(f"wrong rows on the replayed QPs: neighbour's row min {e_nb[stance].min():.3e}, configuration's row min {e_cf.min():.3e}")
    assert stance.all() and e_nb[stance].min() >= 0.18 and e_cf.min() > 1e-2


def test_phase_case_grows_a_perturbation_no_more_than_twice_the_existing_case():
    """The end-to-end bands of test_rollout_phase_matches_host_checker (tests/test_gpu_gaits.py) are carried over to this case: its
    closed loop must not amplify a 1e-9 move of the state by more than twice what that test's case does (24 robots, 30 ticks, the
    configuration's model, synth.make_plant_rows bodies)."""
    lib = C.oracle_lib()
    pb, pr, rows, T = C.phase_case()
    rest = [pb[k] for k in C.PHASE_ARGS[1:]]
    new = C.perturbed_growth(lambda x: M.rollout_phase_models_host(lib, C.LOOP_KW, rows, x, *rest, T, **pr), pb["x"])
    old_rows = mpcqp.synth.make_plant_rows(C.PHASE_B, seed=C.PHASE_SEED, push_start=(3, 15))
    eng = mpcqp.Engine(lib, lib.default_config(**C.LOOP_KW))
    old = C.perturbed_growth(lambda x: gaits.rollout_phase_host(eng, x, *rest, 30, old_rows["body"], old_rows["push"], old_rows["push_ticks"]),
                             pb["x"])
    print(f"growth of a 1e-9 perturbation of x over the roll-out: this case {new:.2f}, the existing case {old:.2f}")
    assert new <= 2.0 * old


def test_grouped_loop_is_a_single_handle_when_all_rows_are_equal():
    lib = C.oracle_lib()
    cfg = lib.default_config(**C.LOOP_KW)
    pb, pr, _, _ = C.phase_case()
    B, T = 8, 6
    cut = lambda d: {k: (None if v is None else v[:B]) for k, v in d.items()}
    pb, pr = cut(pb), cut(pr)
    rows = M.model_rows(cfg, B)
    eng = mpcqp.Engine(lib, cfg)
    one = gaits.rollout_phase_host(eng, *[pb[k] for k in C.PHASE_ARGS], T, pr["body"], pr["push"], pr["push_ticks"])
    _same(M.rollout_phase_models_host(lib, C.LOOP_KW, rows, *[pb[k] for k in C.PHASE_ARGS], T, **pr), one)
    # body = None is the configuration's body, whatever the rows say
    heavy = rows.copy(); heavy[:, 0] *= 1.3
    explicit = M.rollout_phase_models_host(lib, C.LOOP_KW, heavy, *[pb[k] for k in C.PHASE_ARGS], T,
                                           body=mpcqp.plant.model_body(cfg.m, list(cfg.Ibody_inv), B))
    _same(M.rollout_phase_models_host(lib, C.LOOP_KW, heavy, *[pb[k] for k in C.PHASE_ARGS], T), explicit)
    assert not np.array_equal(explicit["forces"], one["forces"])
    # the plan-table roll-out and rollout_plant
    rb = mpcqp.synth.make_rollout_batch(B, seed=C.PLAN_SEED)
    a = [rb[k] for k in PLAN_ARGS]
    _same(M.rollout_models_host(lib, C.LOOP_KW, rows, *a, T), eng.rollout_host(*a, T))
    _same(M.rollout_plant_models_host(lib, C.LOOP_KW, rows, *a, T), mpcqp.plant.rollout_plant_host(eng, *a, T))
    # legs and drive, on 4 robots
    lb, lr, _, _ = C.legs_case()
    lb, lr = ({k: (None if v is None else v[:4]) for k, v in d.items()} for d in (lb, lr))
    la = [lb[k] for k in C.LEGS_ARGS]
    _same(M.rollout_legs_models_host(lib, C.LOOP_KW, rows[:4], *la, T, lb["step_height"], land="actual", **lr),
          gaits.rollout_legs_host(eng, *la, T, lb["step_height"], land="actual", **lr))
    weak, ground = drive_cases.weak_row(0.5), np.array([0.3, 1e3, 0.3, 1e3])
    _same(M.rollout_drive_models_host(lib, C.LOOP_KW, rows[:4], *la, T, lb["step_height"], ground=ground, inertia=weak, **lr),
          gaits.rollout_drive_host(eng, *la, T, lb["step_height"], ground=ground, inertia=weak, **lr))


def test_two_classes_are_two_handles_on_the_halves():
    lib = C.oracle_lib()
    pb, pr, rows, _ = C.phase_case()
    B, T = 8, 6
    pb, pr = ({k: (None if v is None else v[:B]) for k, v in d.items()} for d in (pb, pr))
    two = rows[:B].copy(); two[2:] = two[np.arange(2, B) % 2]
    got = M.rollout_phase_models_host(lib, C.LOOP_KW, two, *[pb[k] for k in C.PHASE_ARGS], T, **pr)
    for c in range(2):
        idx = np.arange(c, B, 2)
        eng = mpcqp.Engine(lib, lib.default_config(**C.LOOP_KW, **M.row_overrides(two[c])))
        one = gaits.rollout_phase_host(eng, *[pb[k][idx] for k in C.PHASE_ARGS], T, pr["body"][idx], pr["push"][idx], pr["push_ticks"][idx])
        for k in one:
            assert np.array_equal(got[k][idx], one[k]), (c, k)


@pytest.mark.parametrize("which", ["legs", "drive_limited", "drive_ideal"])
def test_legs_and_drive_cases_replay_exactly_and_are_not_vacuous(which):
    if which == "legs":
        (pb, pr, rows, T), h, cmd = C.legs_case(), C.host_legs("actual"), "forces"
    else:
        (pb, pr, rows, T), h, cmd = C.drive_case(), C.host_drive(which[6:]), "cmd"
    u0, solved = _replayed_u0(h, pb, rows, T)
    assert np.array_equal(u0, h[cmd]) and np.array_equal(solved, h["solved"])
    zmin = h["actual"][:, :, 5].min()
    print(f"{which}: min z {zmin:.4f}, rows where the drive changed the force {int((h[cmd] != h['forces']).any(axis=2).sum())}")
    assert np.all(h["solved"] == T) and zmin > 0.2 and C.reaches_upper_bound(h[cmd], h["contact_log"], rows, 1e-9).all()
    if which != "legs":
        assert (h["cmd"] != h["forces"]).any()
