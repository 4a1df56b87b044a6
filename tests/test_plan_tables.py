"""Footstep plans and swing trajectories in table form (include/mpcqp_plan.h): the C interface and its host checkers.  No GPU:
the header and export checks read the built product library, the table helpers are held to the reference's own goldens."""
import os
import re

import numpy as np
import pytest

import mpcqp
from conftest import REPO
from mpcqp.foot_trajectory_generator import swing_tables
from mpcqp.footstep_planner import FootstepPlanner, plan_tables
from plan_cases import CASES, case_inputs, inputs


def _declared(name):
    hdr = open(os.path.join(REPO, "include", name)).read()
    return sorted(set(re.findall(r"^\s*(?:int|uint32_t|const char\s*\*)\s*(mpcqp_[a-z_]+)\s*\(", hdr, re.M))), hdr


def test_plan_header_declares_plan_symbols_and_product_exports_them():
    syms, hdr = _declared("mpcqp_plan.h")
    assert set(syms) == set(mpcqp._capi.PLAN_SYMBOLS)
    assert '#include "mpcqp.h"' in hdr
    lib = mpcqp.product_library()
    assert lib.has_plan
    for sym in syms:
        assert hasattr(lib.lib, sym), sym


def test_plan_symbols_stay_out_of_the_shared_header(oracle_lib):
    syms, hdr = _declared("mpcqp.h")
    assert set(syms) == set(mpcqp._capi.EXPORTED_SYMBOLS)
    assert not set(syms) & set(mpcqp._capi.PLAN_SYMBOLS)
    assert int(re.search(r"#define MPCQP_VERSION (0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x00010301 == mpcqp.product_library().version()
    # product-only: the CPU checker does not export them and its binding refuses the calls
    assert not oracle_lib.has_plan
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    with pytest.raises(mpcqp.MpcQpError, match="product library only"):
        eng.plan_footsteps_ptr(1, 1, 1, 1, 1, 1, 1, 1)


@pytest.mark.parametrize("gait,tag", CASES)
def test_plan_tables_reproduce_golden_plans_and_swing(golden, gait, tag):
    L, G = golden["ref_log"], golden["planner_golden"]
    key = gait + tag
    feet0, cmd, g, dt, h = case_inputs(L, gait, tag)
    S = len(G[key + "_plan_pos"])
    t = plan_tables(feet0, cmd, g, S, dt)
    assert np.abs(t["plan_pos"][0] - G[key + "_plan_pos"]).max() <= 1e-12
    assert np.abs(t["plan_ang"][0] - G[key + "_plan_ang"]).max() <= 1e-12
    assert np.array_equal(t["plan_feet_id"][0], G[key + "_plan_feet_id"])
    assert t["plan_meta"][0].tolist() == [S, int(g[0, 1]), int(g[0, 2]), 0]
    T = len(G[key + "_swing_traj"])
    traj, des = swing_tables(t, np.zeros(1, np.int32), T, h, dt)
    assert np.abs(traj[0] - G[key + "_swing_traj"]).max() <= 1e-9
    # started later, the same rows (the side effect of the skipped ticks is replayed from tick 0)
    traj2, des2 = swing_tables(t, np.array([37], np.int32), T - 37, h, dt)
    assert np.array_equal(traj2[0], traj[0, 37:]) and np.array_equal(des2[0], des[0, 37:])


def test_swing_tables_reproduce_closed_loop_desired_feet(golden):
    L, G = golden["ref_log"], golden["planner_golden"]
    feet0, cmd, g, dt, h = inputs(L)
    t = plan_tables(feet0, cmd, g, int(g[0, 0]), dt)
    _, des = swing_tables(t, np.zeros(1, np.int32), 1000, h, dt)
    assert np.abs(des[0] - G["replay_feet_des"]).max() <= 1e-12


def test_plan_tables_pad_truncate_and_stand():
    p = mpcqp.synth.make_plan_inputs(64, seed=5)
    full = plan_tables(p["feet0"], p["cmd"], p["gait"], 120, 0.03)
    short = plan_tables(p["feet0"], p["cmd"], p["gait"], 9, 0.03)
    for k in ("plan_pos", "plan_ang", "plan_hip", "plan_feet_id"):
        assert np.array_equal(short[k], full[k][:, :9], equal_nan=True), k        # a shorter table is a prefix
    total = p["gait"][:, 0]
    steps = np.where(total > 0, total, 100)
    assert np.array_equal(full["plan_meta"][:, 0], np.minimum(steps, 120)) and np.array_equal(short["plan_meta"][:, 0], np.minimum(steps, 9))
    for b in range(64):
        n = full["plan_meta"][b, 0]
        assert np.array_equal(full["plan_pos"][b, n:], np.broadcast_to(full["plan_pos"][b, n - 1], (120 - n, 4, 3)))   # last row repeated
        if total[b] == 0:
            assert np.array_equal(full["plan_pos"][b], np.broadcast_to(p["feet0"][b], (120, 4, 3)))
            assert np.isnan(full["plan_hip"][b, :, :2]).all() and (full["plan_feet_id"][b] == 1).all()
        else:
            assert (full["plan_feet_id"][b, 0] == 1).all()
            m = [(int(p["gait"][b, 3]) >> k) & 1 for k in range(4)]
            if n > 2:
                assert full["plan_feet_id"][b, 1].tolist() == m and full["plan_feet_id"][b, 2].tolist() == [1 - v for v in m]
    neg = p["gait"].copy(); neg[:, 0] = -3                                        # negative total_steps: the standing plan
    s = plan_tables(p["feet0"], p["cmd"], neg, 5, 0.03)
    assert (s["plan_meta"][:, 0] == 5).all() and np.array_equal(s["plan_pos"], np.broadcast_to(p["feet0"][:, None], (64, 5, 4, 3)))


def test_make_plan_inputs_covers_the_gait_space():
    p = mpcqp.synth.make_plan_inputs(4096, seed=11)
    g, c = p["gait"], p["cmd"]
    assert set(g[:, 3]) == set(range(16))
    assert {0, 1, 2, 3, 20, 50} <= set(g[:, 0]) and any(v % 2 == 1 and v > 3 for v in g[:, 0])
    assert 0 in set(g[:, 2]) and len(set(g[:, 1])) >= 2 and len(set(g[:, 2])) >= 2
    assert {0.0, 0.3, -0.3, 1.0} <= set(np.round(c[:, 3], 6)) and np.abs(c[:, 2]).max() > 0.05 and np.ptp(c[:, 0]) > 5.0


def test_from_tables_answers_planner_queries():
    p = mpcqp.synth.make_plan_inputs(4, seed=2)
    p["gait"][:, :3] = (12, 4, 2)
    t = plan_tables(p["feet0"], p["cmd"], p["gait"], 12, 0.03)
    for b in range(4):
        ini = {l: p["feet0"][b, k] for k, l in enumerate(mpcqp.footstep_planner.LEGS)}
        ini["yaw"] = p["cmd"][b, 0]
        host = FootstepPlanner(ini, {"ss_duration": 4, "ds_duration": 2, "world_time_step": 0.03, "h": p["cmd"][b, 4], "total_steps": 12,
                                     "v_com_ref": np.array([p["cmd"][b, 1], p["cmd"][b, 2], 0]), "theta_dot": p["cmd"][b, 3],
                                     "first_swing": np.array([(int(p["gait"][b, 3]) >> k) & 1 for k in range(4)])})
        pl = FootstepPlanner.from_tables(t["plan_pos"][b], t["plan_feet_id"][b], t["plan_ang"][b], 4, 2, t["plan_hip"][b])
        assert np.array_equal(pl.contact_mask(3, 40), host.contact_mask(3, 40))
        assert pl.plan[5]["pos"] == host.plan[5]["pos"] and pl.get_phase_at_time(17) == host.get_phase_at_time(17)
