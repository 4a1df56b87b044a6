"""Cases shared by tests/test_disturbance_paths_host.py and tests/test_gpu_disturbance_paths.py: the disturbance table
(include/mpcqp_disturb.h) through every solving path and every roll-out, with wrench rows that differ per robot.

Single QPs.  `solve_case(N, B, seed)`: the batch and the wrench distribution of disturbance_cases.shift_case (up to 20 N and 3 N m)
with row 0 zero, every other row distinct and one row NaN, next to models_rollout_cases.model_rows(B) (four classes).  GRID has the
engines, horizons, I/O types and discretisations; its batch sizes are the smallest whose B (N + 1) rows cross one 256-lane block of the
shift kernel and leave the last block partly empty.  `solve_reference` is the checker's answer through models.grouped_host with each
group's handle wrapped as DisturbedEngine(handle, rows[idx]).

Roll-outs.  Nothing is invented: the plan table is synth.make_rollout_batch(8, seed=7) over 6 ticks, the phase loop the pushed fixture of
disturbance_cases, and the legs, drive, slip and observe loops the first 8 robots of legsim_cases.rollout_batch() over 8 ticks with the
operands of drive_cases and observe_cases (ground 0.3 under the even robots, tau_max x 0.5, the sensor draw).  `loop_rows` tells every
robot its own push where it has one, otherwise a draw of at most 8 N and 1 N m whose torque has x and y components, so that Rz matters;
row 0 is zero.  `host_loop(kind)` is the host twin of each device roll-out through DisturbedEngine on the closed loops' checker, once per
process; the results are shared and must not be altered.

The conditions these cases meet on the CPU are asserted in tests/test_disturbance_paths_host.py."""
import functools

import numpy as np

import disturbance_cases as D
import drive_cases as dc
import legsim_cases
import models_rollout_cases as MR
import mpcqp
import observe_cases as oc
from mpcqp import disturbance, gaits, lite3_model, plant, synth
from mpcqp import models as M

DELTA = D.DELTA
TIGHT = dict(eps_abs=1e-10, eps_rel=1e-10, max_iter=100000, polish_max=30)           # test_gpu_disturbance.py's tight checker
FORCE_BAND, STATE_BAND = 1e-4, 1e-5                                                  # closed loops: forces 1e-4 of their scale, states 1e-5
# (tests/test_rollout.py, test_gpu_plant.py, test_gpu_gaits.py and test_gpu_disturbance.py's _rollout_band hold these same two figures)
GRID = (   # id, N, B, io, precision, engine, disc
    ("dense-n10-f32", 10, 24, "f32", "mixed", "dense", "euler"),
    ("dense-n10-f64-f64", 10, 24, "f64", "f64", "dense", "euler"),
    ("dense-n20-f64", 20, 13, "f64", "mixed", "dense", "euler"),
    ("dense-n20-f32-zoh", 20, 13, "f32", "mixed", "dense", "zoh"),
    ("stage-flag-n10-zoh", 10, 24, "f64", "mixed", "stage_flag", "zoh"),
    ("stage-n60-f32", 60, 5, "f32", "mixed", "stage", "euler"),
    ("stage-omega-n10", 10, 24, "f64", "mixed", "stage_omega", "euler"),
)
DISC = {"euler": mpcqp.DISC_EULER, "zoh": mpcqp.DISC_ZOH}
PLAN_B, PLAN_T, PLAN_SEED = 8, 6, 7
LEGS_B, LEGS_T = 8, 8
PHASE_B, PHASE_T = 16, 6                                                             # the fixture's four robots, tiled
YAW_OFFSET = 0.3
LOOP_FORCE, LOOP_TORQUE = 8.0, 1.0
LOOPS = ("plan", "plant", "phase", "legs", "drive", "slip", "observe_truth", "observe_estimate", "observe_gated", "observe_aided",
         "observe_yaw")


def engine_overrides(engine, disc):
    """The MpcQpConfig overrides (of the device handle and of the checker alike) that select a grid point's engine and discretisation."""
    kw = {"disc": DISC[disc]}
    if engine == "stage_omega":                                                      # an anisotropic omega weight: the stage-wise engine
        w = list(mpcqp.Library(D.ORACLE_SO).default_config(N=10).w)
        w[7] = 2.0 * w[6]
        kw["w"] = w
    return kw


def wrench_rows(B, N=10, seed=0, nan_row=None):
    """shift_case's rows with row 0 zero and (nan_row) one row whose torque is NaN; the others are distinct."""
    _, rows, _ = D.shift_case(B, N, seed)
    rows = rows.copy()
    rows[0] = 0.0
    assert len({tuple(r) for r in rows}) == B
    if nan_row is not None:
        rows[nan_row, 4] = np.nan
    return rows


def solve_case(N, B, seed=0, io="f64", nan=True):
    """(batch, wrench rows, model rows, the NaN row or None).  With io = "f32" every float operand is rounded once, so that the host sees
    what the device reads."""
    b, _, _ = D.shift_case(B, N, seed)
    b = {k: v for k, v in b.items() if k in ("x0", "r", "contact", "xdes", "mu")}
    if io == "f32":
        b = {k: (v if k == "contact" else D.r32(v)) for k, v in b.items()}
    nan_row = B - 2 if nan and B >= 5 else None                                          # (never one of robots 0, 1, 2: `swapped`)
    return b, wrench_rows(B, N, seed, nan_row), MR.model_rows(B), nan_row


def shifted_tuple(b, rows, cfg, models=None):
    """The tuple the table makes of `b`: xdes - s from the host (NaN on a robot with a non-finite row)."""
    return dict(b, xdes=disturbance.shift_host(b["x0"], b["xdes"], rows, cfg, models))


def solve_reference(b, rows, models, N, overrides=None, want_X=True):
    """The checker's answer with both tables: one tight handle per distinct model row (models.grouped_host), each wrapped with its
    robots' wrench rows.  models = None: the configuration's model on one handle."""
    kw = dict(N=N, delta=DELTA, **TIGHT, **(overrides or {}))
    lib = mpcqp.Library(D.ORACLE_SO)
    solve = lambda eng, idx: disturbance.DisturbedEngine(eng, rows[idx]).solve_batch_host(
        b["x0"][idx], b["r"][idx], b["contact"][idx], b["xdes"][idx], b["mu"][idx], want_X=want_X)
    if models is None:
        eng = mpcqp.Engine(lib, lib.default_config(**kw))
        try:
            return solve(eng, np.arange(len(rows)))
        finally:
            eng.close()
    return M.grouped_host(lib, kw, models, len(rows), solve)


# ------------------------------------------------------------------------------------------------------------------- the ordered launch
ORDER_SIZES = ((2304, 10, "f32", 20261030), (2304, 10, "f64", 20261030), (600, 20, "f32", 20261031))   # test_gpu_order_identity.py's


def order_case(B, N, seed):
    """The bench distribution of tests/test_gpu_order_identity.py, clean, with a wrench table of 12 non-finite rows (NaN, +inf, -inf) and
    6 rows at 1e30, and model rows of four classes.  Returns (batch, wrench rows, model rows, the non-finite rows, the huge rows)."""
    b = synth.make_batch(B, N, 0.03, seed, ("trot", "pronk", "amble", "gallop"), (0.3, 0.5, 0.7, 1.0))
    b = {k: v for k, v in b.items() if k in ("x0", "r", "contact", "xdes", "mu")}
    rng = np.random.default_rng(seed + 1)
    rows = np.concatenate([rng.uniform(-20.0, 20.0, (B, 3)), rng.uniform(-3.0, 3.0, (B, 3))], axis=1)
    rows[0] = 0.0
    pick = rng.permutation(np.arange(1, B))[:18]
    bad, huge = pick[:12], pick[12:]
    for i, r in enumerate(bad):
        rows[r, i % 6] = (np.nan, np.inf, -np.inf)[i % 3]
    for i, r in enumerate(huge):
        rows[r, i % 6] = 1e30 if i % 2 == 0 else -1e30
    return b, rows, MR.model_rows(B), bad, huge


# ----------------------------------------------------------------------------------------------------------------------- the roll-outs
def loop_checker(**kw):
    lib = mpcqp.Library(D.ORACLE_SO)
    return mpcqp.Engine(lib, lib.default_config(**{**MR.LOOP_KW, **kw}))


def loop_rows(B, push=None, seed=41):
    """Rows for the closed loops: robot b's own push where it has one, else a draw of at most LOOP_FORCE and LOOP_TORQUE whose torque has
    x and y components; row 0 zero."""
    rng = np.random.default_rng(seed + B)
    rows = np.concatenate([rng.uniform(-LOOP_FORCE, LOOP_FORCE, (B, 3)), rng.uniform(-LOOP_TORQUE, LOOP_TORQUE, (B, 3))], axis=1)
    rows[:, 3:5] = np.where(np.abs(rows[:, 3:5]) < 0.2, np.copysign(0.2, rows[:, 3:5]), rows[:, 3:5])
    if push is not None:
        has = np.any(np.asarray(push) != 0.0, axis=1)
        rows[has] = np.asarray(push, np.float64)[has]
    rows[0] = 0.0
    assert len({tuple(r) for r in rows}) == B
    return rows


def plan_case():
    """(rb, rows, T): the plan-table batch of mpcqp_rollout and mpcqp_rollout_plant.  The plant of rollout_plant is pushed by the rows
    themselves: the MPC is told the truth, as in the fixture's "told" run."""
    rb = synth.make_rollout_batch(PLAN_B, seed=PLAN_SEED)
    return rb, loop_rows(PLAN_B), PLAN_T


def plan_ticks():
    return np.tile(np.array([[0, 1 << 20]], np.int32), (PLAN_B, 1))


def phase_case():
    """(pb, rows, idx, T): the pushed fixture of disturbance_cases tiled to 16 robots, told its pushes."""
    idx = np.arange(PHASE_B) % D.B_FIX
    return D.fixture_batch(), D.PUSH[idx], idx, PHASE_T


def legs_case(yaw=False):
    """(pb, plant rows, wrench rows, T): the first 8 robots of legsim_cases.rollout_batch().  pb carries the operands of every loop of
    the family: "legs", "step_height", "ground", "foot_mass", "height", the sensor draw, and "est_init" -- x[:, :12], with `yaw` the
    yaw entry moved by YAW_OFFSET on the odd robots."""
    pb, pr = legsim_cases.rollout_batch()
    B = LEGS_B
    pb = {k: v[:B] for k, v in pb.items()}
    pr = {k: v[:B] for k, v in pr.items()}
    s = oc.sensor_draw(B, LEGS_T)
    pb.update(legs=np.zeros((B, 4, 7)), step_height=np.full(B, legsim_cases.STEP_HEIGHT), ground=oc.ground_rows(B),
              foot_mass=np.full(B, lite3_model.foot_mass()), height=pb["stand"][:, :, 2].copy(), bias=s["bias"], noise=s["noise"],
              enc_noise=s["enc_noise"], est_init=pb["x"][:, :12].copy())
    if yaw:
        pb["est_init"][1::2, 2] += YAW_OFFSET
    return pb, pr, loop_rows(B, pr["push"]), LEGS_T


LEGS_ARGS = ("x", "ref", "feet", "legs", "gait", "stand", "gain", "tick", "mu")
PLAN_ARGS = ("x", "ref", "plan_pos", "plan_feet_id", "plan_meta", "tick", "mu")
OBSERVE = {"observe_truth": dict(feed="truth"), "observe_estimate": dict(feed="estimate"), "observe_gated": dict(feed="estimate", gate={}),
           "observe_aided": dict(feed="estimate", attitude={}), "observe_yaw": dict(feed="estimate")}


def run_host_loop(kind, rows="own", eng=None, x=None):
    """The host twin of the device roll-out `kind` (one of LOOPS) under the wrench rows `rows` ("own": the case's, None: no table, or an
    array), on `eng` (the closed loops' checker) and, for the growth measurement, from another start state x."""
    eng = eng or loop_checker()
    pick = lambda own: own if isinstance(rows, str) else rows
    if kind in ("plan", "plant"):
        rb, own, T = plan_case()
        de = disturbance.DisturbedEngine(eng, pick(own))
        a = [rb[k] if k != "x" or x is None else x for k in PLAN_ARGS]
        if kind == "plan":
            return de.rollout_host(*a, T)
        return plant.rollout_plant_host(de, *a, T, None, own, plan_ticks())
    if kind == "phase":
        pb, own, idx, T = phase_case()
        de = disturbance.DisturbedEngine(eng, pick(own))
        return gaits.rollout_phase_host(de, (pb["x"] if x is None else x)[idx], pb["ref"][idx], pb["feet"][idx], pb["gait"][idx], pb["stand"][idx],
                                        pb["gain"][idx], pb["tick"][idx], pb["mu"][idx], T, push=D.PUSH[idx], push_ticks=D.PUSH_TICKS[idx])
    pb, pr, own, T = legs_case(yaw=kind == "observe_yaw")
    de = disturbance.DisturbedEngine(eng, pick(own))
    a = [pb[k] if k != "x" or x is None else x for k in LEGS_ARGS]
    if kind == "legs":
        return gaits.rollout_legs_host(de, *a, T, pb["step_height"], land="rule", **pr_kw(pr))
    weak = dict(inertia=dc.weak_row(0.5), **pr_kw(pr))
    if kind == "drive":
        return gaits.rollout_drive_host(de, *a, T, pb["step_height"], land="rule", drive="limited", ground=pb["ground"], **weak)
    if kind == "slip":
        return gaits.rollout_slip_host(de, *a, T, pb["step_height"], pb["ground"], pb["foot_mass"], **weak)
    return gaits.rollout_observe_host(de, *a, T, pb["step_height"], pb["ground"], pb["foot_mass"], est_init=pb["est_init"], height=pb["height"],
                                      bias=pb["bias"], noise=pb["noise"], enc_noise=pb["enc_noise"], **OBSERVE[kind], **weak)


def pr_kw(pr):
    return {"body": pr["body"], "push": pr["push"], "push_ticks": pr["push_ticks"]}


@functools.lru_cache(maxsize=None)
def host_loop(kind, told=True):
    """run_host_loop under the case's rows (told) or without a table, once per process; shared: do not alter."""
    return run_host_loop(kind, "own" if told else None)


@functools.lru_cache(maxsize=None)
def host_loop_models(kind):
    """The "phase" or the "legs" loop with a model table of four classes as well, every plant the body of its own row: per class one
    checker handle of that row's model (models.grouped_host), wrapped with its robots' wrench rows.  Returns (logs, model rows, bodies);
    shared: do not alter."""
    lib = mpcqp.Library(D.ORACLE_SO)
    if kind == "phase":
        pb, rows, idx, T = phase_case()
        mod = MR.model_rows(PHASE_B)
        body, per = MR.matched_bodies(mod), [pb[k][idx] for k in MR.PHASE_ARGS]
        loop = lambda eng, i: gaits.rollout_phase_host(disturbance.DisturbedEngine(eng, rows[i]), *[a[i] for a in per], T, body[i],
                                                       D.PUSH[idx][i], D.PUSH_TICKS[idx][i])
    else:
        pb, pr, rows, T = legs_case()
        mod = MR.model_rows(LEGS_B)
        body, per = MR.matched_bodies(mod), [pb[k] for k in LEGS_ARGS]
        loop = lambda eng, i: gaits.rollout_legs_host(disturbance.DisturbedEngine(eng, rows[i]), *[a[i] for a in per], T, pb["step_height"][i],
                                                      land="rule", body=body[i], push=pr["push"][i], push_ticks=pr["push_ticks"][i])
    return M.grouped_host(lib, MR.LOOP_KW, mod, len(mod), loop), mod, body


def swapped(rows):
    """Rows 1 and 2 exchanged: what an off-by-one row index would read for robot 1."""
    out = np.array(rows, dtype=np.float64)
    out[[1, 2]] = out[[2, 1]]
    return out


def commanded(logs):
    """The forces the MPC commanded: "cmd" where the loop has a drive rule, else "forces"."""
    return logs["cmd"] if "cmd" in logs and logs["cmd"] is not None else logs["forces"]


def loop_band(ref):
    """(force band, state band) of a closed loop against its host twin `ref`: 1e-4 of the forces' scale, 1e-5 on the states."""
    return FORCE_BAND * max(1.0, float(np.abs(commanded(ref)).max())), STATE_BAND
