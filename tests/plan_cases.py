"""Planner inputs of the golden cases (tests/golden/planner_golden.npz, ref_log.npz) in the table form of include/mpcqp_plan.h:
the same parameters test_planner_glue.py hands the host FootstepPlanner, as feet0 / cmd / gait rows."""
import numpy as np

GAITS = {"gallop": [0, 0, 1, 1], "trot": [1, 0, 0, 1], "amble": [1, 0, 1, 0], "pronk": [0, 0, 0, 0]}
TURN = {"theta_dot": 0.3, "v_com_ref": (0.1, 0.02)}
CASES = [(g, tag) for g in GAITS for tag in ("", "_turn")]      # 8 golden plans: key = gait + tag


def mask(first_swing):
    return int(sum(int(v) << k for k, v in enumerate(first_swing)))


def inputs(L, first_swing=None, turn=False):
    """(feet0 [1,4,3], cmd [1,5], gait [1,4], dt, step_height) of one golden case."""
    v = TURN["v_com_ref"] if turn else (float(L["param_v_com_ref"][0]), float(L["param_v_com_ref"][1]))
    w = TURN["theta_dot"] if turn else float(L["param_theta_dot"])
    fs = L["param_first_swing"].astype(int) if first_swing is None else first_swing
    feet0 = L["feet_actual"][0][None].astype(float)
    cmd = np.array([[float(L["actual"][0, 2]), v[0], v[1], w, float(L["param_h"])]])
    gait = np.array([[int(L["param_total_steps"]), int(L["param_ss_duration"]), int(L["param_ds_duration"]), mask(fs)]], np.int32)
    return feet0, cmd, gait, float(L["param_world_time_step"]), np.array([float(L["param_step_height"])])


def case_inputs(L, gait, tag):
    return inputs(L, np.array(GAITS[gait]), turn=tag == "_turn")
