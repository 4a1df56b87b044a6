"""The case shared by tests/test_models_rollouts_host.py and tests/test_gpu_models_rollouts.py: per-robot model rows
(include/mpcqp_model.h) through every roll-out that reads them.

Rows.  Four classes cycling through the slots, mass 0.8 .. 1.4 of the nominal one, f_max = 100 N for the first three and 0.6 m |g|
for the last: on two legs that class sits at its upper bound, and it still carries a trot (the 0.45 m |g| class of the default
synth.make_model_rows cannot: those robots fall, and a fallen robot's QPs say little about the row).  Every robot's plant is the body
of its own row ("matched"): (m, Ixx, Iyy, Izz, 0, 0, 0).

Batches.  The phase batch is the one of tests/test_gpu_gaits.py's host comparison (24 robots on the eight named gaits at period 10,
seed 7, its pushes) over 24 ticks; the legs batch is legsim_cases.rollout_batch() (16 robots, 25 ticks); the drive batch is
drive_cases.loop_batch() (8 robots, 36 ticks) with tau_max x 0.5 and, for the limited drive, ground 0.3 under the even robots; the
plan-table batch is synth.make_rollout_batch(24, seed=7) over 20 ticks.

On the CPU checker (tests/test_models_rollouts_host.py holds these): every tick of every robot solves, no robot drops below
z = 0.25 m (0.2 m under the limited and the slipping drive), the upper f_z bound is active somewhere in every class, and a wrong row
moves the replayed QPs far outside the 1e-4 band:
a neighbour's row by at least 0.18 relative on every row with a stance leg, the configuration's row by more than 1e-2 on every row."""
import functools

import numpy as np

import drive_cases
import legsim_cases
import mpcqp
from conftest import ORACLE_SO
from mpcqp import gaits, synth
from mpcqp import models as M

G = 9.81
CLASSES = 4
NAMES = tuple(gaits.GAITS)
PHASE_B, PHASE_T, PHASE_SEED = 24, 24, 7
LEGS_B, LEGS_T = legsim_cases.ROLL_B, legsim_cases.ROLL_T
DRIVE_B, DRIVE_T = drive_cases.LOOP_B, drive_cases.LOOP_T
PLAN_B, PLAN_T, PLAN_SEED = 24, 20, 7
LOOP_KW = dict(N=10, delta=0.03, max_iter=4000)                                       # the checker of the closed loops (test_gpu_gaits.py's)
TIGHT_KW = dict(N=10, delta=0.03, max_iter=100000, eps_abs=1e-10, eps_rel=1e-10, polish_max=30)   # the checker of single QPs (test_gpu_models.py's)
PHASE_LOGS = ("actual", "desired", "forces", "feet_log", "contact_log", "solved")
PHASE_STATE = ("x", "ref", "feet", "tick")


def oracle_lib():
    return mpcqp.Library(ORACLE_SO)


def model_rows(B):
    rows = synth.make_model_rows(B, classes=CLASSES, mass_scale=(0.8, 1.4), f_max=(100.0, 100.0))
    last = np.arange(B) % CLASSES == CLASSES - 1
    rows[last, 5] = 0.6 * rows[last, 0] * G
    return rows


def matched_bodies(rows):
    """The plant of a robot whose controller knows it: body = (m, Ixx, Iyy, Izz, 0, 0, 0) of the robot's row."""
    return np.ascontiguousarray(np.concatenate([rows[:, :4], np.zeros((len(rows), 3))], axis=1))


def phase_case():
    """(pb, plant rows, model rows, T) of the phase batch."""
    pb = gaits.make_phase_batch(PHASE_B, NAMES, 10, seed=PHASE_SEED)
    pr = synth.make_plant_rows(PHASE_B, seed=PHASE_SEED, push_start=(3, 15))
    rows = model_rows(PHASE_B)
    return pb, {"body": matched_bodies(rows), "push": pr["push"], "push_ticks": pr["push_ticks"]}, rows, PHASE_T


def legs_case():
    """(pb, plant rows, model rows, T) of the legs batch; pb carries "legs" and "step_height"."""
    pb, pr = legsim_cases.rollout_batch()
    pb = dict(pb, legs=np.zeros((LEGS_B, 4, 7)), step_height=np.full(LEGS_B, legsim_cases.STEP_HEIGHT))
    rows = model_rows(LEGS_B)
    return pb, {"body": matched_bodies(rows), "push": pr["push"], "push_ticks": pr["push_ticks"]}, rows, LEGS_T


def drive_case():
    """(pb, plant rows, model rows, T) of the drive batch, nobody pushed; `drive_ground()` and `drive_cases.weak_row(0.5)` go with it."""
    pb = drive_cases.loop_batch()
    rows = model_rows(DRIVE_B)
    return pb, {"body": matched_bodies(rows), "push": None, "push_ticks": None}, rows, DRIVE_T


def drive_ground(even_only=True):
    """The slippery ground: drive_cases.GROUND_MU under the even robots (a ground that never limits under the odd ones), or under all."""
    return np.where(np.arange(DRIVE_B) % 2 == 0, drive_cases.GROUND_MU, 1e3) if even_only else np.full(DRIVE_B, drive_cases.GROUND_MU)


def plan_case():
    """(rb, model rows, T) of the plan-table batch (mpcqp_rollout: no plant, x <- X[:,1])."""
    return synth.make_rollout_batch(PLAN_B, seed=PLAN_SEED), model_rows(PLAN_B), PLAN_T


PHASE_ARGS = ("x", "ref", "feet", "gait", "stand", "gain", "tick", "mu")
LEGS_ARGS = ("x", "ref", "feet", "legs", "gait", "stand", "gain", "tick", "mu")


@functools.lru_cache(maxsize=None)
def host_phase():
    """rollout_phase_models_host on the phase case (LOOP_KW), once per process; the result is shared: do not alter it."""
    pb, pr, rows, T = phase_case()
    return M.rollout_phase_models_host(oracle_lib(), LOOP_KW, rows, *[pb[k] for k in PHASE_ARGS], T, pr["body"], pr["push"], pr["push_ticks"])


@functools.lru_cache(maxsize=None)
def host_legs(land):
    pb, pr, rows, T = legs_case()
    return M.rollout_legs_models_host(oracle_lib(), LOOP_KW, rows, *[pb[k] for k in LEGS_ARGS], T, pb["step_height"], land=land, **pr)


@functools.lru_cache(maxsize=None)
def host_drive(drive):
    """drive = "limited": tau_max x 0.5, ground 0.3 under the even robots; "ideal": ground 0.3 under every robot."""
    pb, pr, rows, T = drive_case()
    return M.rollout_drive_models_host(oracle_lib(), LOOP_KW, rows, *[pb[k] for k in LEGS_ARGS], T, pb["step_height"], drive=drive,
                                       ground=drive_ground(drive == "limited"), inertia=drive_cases.weak_row(0.5), **pr)


def replay_reference(ops, rows_tiled):
    """The checker's answer of replayed rows (`M.replay_rows`): phase_expand_host, then one tight checker handle per distinct row.
    Returns (tuple batch in the mpcqp.synth layout, checker result)."""
    e = gaits.phase_expand_host(ops["x"], ops["ref"], ops["feet"], ops["gait"], ops["tick"], ops["stand"], ops["gain"], 10, 0.03)
    batch = {"x0": ops["x"], "r": e["r"], "contact": e["contact"], "xdes": e["xdes"], "mu": ops["mu"]}
    return batch, M.solve_batch_models_host(oracle_lib(), TIGHT_KW, rows_tiled, batch, want_X=False)


def reaches_upper_bound(forces, contact_log, rows, tol=1e-6):
    """Per class: some stance leg of some tick has f_z within `tol` of the class's f_max.  forces [B,T,12], contact_log [B,T,4]."""
    fz = np.asarray(forces, np.float64).reshape(forces.shape[0], forces.shape[1], 4, 3)[..., 2]
    at = (np.abs(fz - rows[:, 5][:, None, None]) <= tol) & (np.asarray(contact_log) != 0)
    return np.array([bool(at[c::CLASSES].any()) for c in range(CLASSES)])


def perturbed_growth(loop, x, eps=1e-9, seed=3):
    """Host-measured growth of a closed loop `loop(x) -> logs`: the largest change of "actual" over the roll-out when x is moved by
    `eps` (random signs on the twelve state entries), divided by eps."""
    x2 = np.array(x, dtype=np.float64)
    x2[:, :12] += eps * np.random.default_rng(seed).choice([-1.0, 1.0], (len(x2), 12))
    return float(np.abs(loop(x2)["actual"] - loop(x)["actual"]).max() / eps)
