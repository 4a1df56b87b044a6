"""Per-robot model rows (include/mpcqp_model.h): row helpers and the host checkers.

A model row is ``(m, Ixx, Iyy, Izz, f_min, f_max)`` -- the mass, the principal inertias in the torso frame and the f_z box of ONE
robot's MPC, fp64.  ``MPCBatch.set_models`` hands a table of them to the device engine.  The CPU checker under ``oracle/`` has one
model per handle, so the checkers here group the batch by identical row and solve each group with a handle of its own, created
with that row's ``m``, ``Ibody_inv = 1 / I``, ``f_min`` and ``f_max`` (``grouped_host``): one checker per entry point that reads
the table -- the solves, ``rollout``, ``rollout_plant``, ``rollout_phase``, ``rollout_legs``, ``rollout_drive`` and ``rollout_slip``.  The row is the
MPC's model only: the plant and the legs step of a roll-out use `body`, and with ``body=None`` the CONFIGURATION's model, whatever
the table says.  ``replay_rows`` turns a roll-out's logs back into the QPs it solved, one per (robot, tick).
"""
from __future__ import annotations

import numpy as np

from . import _capi
from .plant import DEFAULT_SUBSTEPS, rollout_plant_host

ROW = 6


def model_rows(cfg, B):
    """The configuration's own row, B times: [B,6] fp64.  Setting it changes nothing when 1 / m and 1 / Ibody_inv are exact."""
    Ii = [float(v) for v in cfg.Ibody_inv]
    row = np.array([float(cfg.m), 1.0 / Ii[0], 1.0 / Ii[1], 1.0 / Ii[2], float(cfg.f_min), float(cfg.f_max)])
    return np.tile(row, (int(B), 1))


def models_from_bodies(body, f_min, f_max):
    """Plant `body` rows [B,7] = (m, Ixx, Iyy, Izz, Ixy, Ixz, Iyz) (include/mpcqp_sim.h) -> model rows [B,6] with the given f_z box
    (scalars or [B]).  The MPC's model is diagonal: a non-zero product of inertia raises ValueError."""
    body = np.asarray(body, dtype=np.float64).reshape(-1, 7)
    if np.any(body[:, 4:7] != 0.0):
        bad = np.nonzero(np.any(body[:, 4:7] != 0.0, axis=1))[0]
        raise ValueError(f"models_from_bodies: rows {bad.tolist()[:8]} have products of inertia; the MPC's model is diag(Ixx, Iyy, Izz)")
    B = body.shape[0]
    box = np.stack([np.broadcast_to(np.asarray(f_min, np.float64), (B,)), np.broadcast_to(np.asarray(f_max, np.float64), (B,))], axis=1)
    return np.ascontiguousarray(np.concatenate([body[:, :4], box], axis=1))


def row_overrides(row):
    """The MpcQpConfig overrides that give a handle the model of `row`."""
    m, ixx, iyy, izz, lo, hi = (float(v) for v in row)
    return {"m": m, "Ibody_inv": (1.0 / ixx, 1.0 / iyy, 1.0 / izz), "f_min": lo, "f_max": hi}


def _groups(models, B):
    models = np.ascontiguousarray(models, dtype=np.float64)
    if models.shape != (B, ROW):
        raise ValueError(f"models must be [{B},{ROW}], got {models.shape}")
    rows, inv = np.unique(models, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    return [(rows[g], np.nonzero(inv == g)[0]) for g in range(len(rows))]


def solve_batch_models_host(oracle_lib, cfg_overrides, models, batch, want_X=True):
    """Host checker of a solve with a model table: QPs are grouped by identical row, each group is solved by one checker handle
    created from `cfg_overrides` plus that row's m, Ibody_inv, f_min, f_max.  `batch` is the mpcqp.synth tuple layout.  Returns
    u, X, status, iters, res as ``Engine.solve_batch_host``."""
    B = len(batch["x0"])
    return grouped_host(oracle_lib, cfg_overrides, models, B, lambda eng, idx: eng.solve_batch_host(
        batch["x0"][idx], batch["r"][idx], batch["contact"][idx], batch["xdes"][idx], batch["mu"][idx], want_X=want_X))


def grouped_host(oracle_lib, cfg_overrides, models, B, loop):
    """The grouped checker: `loop(engine, idx)` -- any per-robot host loop, run on the robots `idx` with the checker handle `engine`
    and returning a dict of arrays with one leading row per robot of `idx` (None values pass through) -- is called once per
    distinct row of `models` [B,6], on a handle created from `cfg_overrides` plus that row's m, Ibody_inv, f_min, f_max, and the
    results are scattered back into [B,...] arrays.  The handle is closed after its call."""
    out = None
    for row, idx in _groups(models, B):
        kw = dict(cfg_overrides); kw.update(row_overrides(row))
        eng = _capi.Engine(oracle_lib, oracle_lib.default_config(**kw))
        try:
            o = loop(eng, idx)
        finally:
            eng.close()
        if out is None:
            out = {k: (None if v is None else np.zeros((B,) + np.shape(v)[1:], np.asarray(v).dtype)) for k, v in o.items()}
        for k, v in o.items():
            if v is not None:
                out[k][idx] = v
    return out


def _sub(a, idx):
    """Rows `idx` of a per-robot operand; None stays None."""
    return None if a is None else np.asarray(a)[idx]


def _config_body(oracle_lib, cfg_overrides, body, B):
    """body = None is the CONFIGURATION's body (`cfg_overrides`), as on the device: never the row's."""
    if body is None:
        from .plant import model_body
        base = oracle_lib.default_config(**cfg_overrides)
        body = model_body(base.m, list(base.Ibody_inv), B)
    return np.asarray(body, np.float64)


def rollout_plant_models_host(oracle_lib, cfg_overrides, models, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T, body=None, push=None,
                              push_ticks=None, substeps=DEFAULT_SUBSTEPS):
    """Host checker of mpcqp_rollout_plant with a model table: ``plant.rollout_plant_host`` per group of robots with an identical
    row, each with a checker handle of that row's model.  body = None steps the plant with the CONFIGURATION's model
    (`cfg_overrides`), as the device does.  Returns the advanced (x, ref, tick) and the logs, as ``plant.rollout_plant_host``."""
    B = np.asarray(x).shape[0]
    body = _config_body(oracle_lib, cfg_overrides, body, B)
    per = (x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu)
    return grouped_host(oracle_lib, cfg_overrides, models, B, lambda eng, idx: rollout_plant_host(
        eng, *[np.asarray(a)[idx] for a in per], T, body=body[idx], push=_sub(push, idx), push_ticks=_sub(push_ticks, idx), substeps=substeps))


def rollout_models_host(oracle_lib, cfg_overrides, models, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T):
    """Host checker of mpcqp_rollout (plan table, world step x <- X[:,1]) with a model table: ``Engine.rollout_host`` per group, so
    the prediction that becomes the next state is the one under the robot's own row.  Returns what ``Engine.rollout_host`` returns."""
    B = np.asarray(x).shape[0]
    per = (x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu)
    return grouped_host(oracle_lib, cfg_overrides, models, B, lambda eng, idx: eng.rollout_host(*[np.asarray(a)[idx] for a in per], T))


def rollout_phase_models_host(oracle_lib, cfg_overrides, models, x, ref, feet, gait, stand, gain, tick, mu, T, body=None, push=None,
                              push_ticks=None, substeps=DEFAULT_SUBSTEPS):
    """Host checker of mpcqp_rollout_phase with a model table: ``gaits.rollout_phase_host`` per group.  body = None is the
    configuration's body.  Returns what ``gaits.rollout_phase_host`` returns."""
    from .gaits import rollout_phase_host
    B = np.asarray(x).shape[0]
    body = _config_body(oracle_lib, cfg_overrides, body, B)
    per = (x, ref, feet, gait, stand, gain, tick, mu)
    return grouped_host(oracle_lib, cfg_overrides, models, B, lambda eng, idx: rollout_phase_host(
        eng, *[_sub(a, idx) for a in per], T, body[idx], _sub(push, idx), _sub(push_ticks, idx), substeps))


def _legs_models_host(loop, oracle_lib, cfg_overrides, models, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, body, per_kw, kw):
    B = np.asarray(x).shape[0]
    body = _config_body(oracle_lib, cfg_overrides, body, B)
    step_height = np.broadcast_to(np.asarray(step_height, np.float64), (B,))
    per = (x, ref, feet, legs, gait, stand, gain, tick, mu)
    return grouped_host(oracle_lib, cfg_overrides, models, B, lambda eng, idx: loop(
        eng, *[_sub(a, idx) for a in per], T, step_height[idx], body=body[idx], **{k: _sub(v, idx) for k, v in per_kw.items()}, **kw))


def rollout_legs_models_host(oracle_lib, cfg_overrides, models, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land="rule",
                             body=None, push=None, push_ticks=None, substeps=DEFAULT_SUBSTEPS, gains=None, leg_substeps=0, inertia=None,
                             actuators=None):
    """Host checker of mpcqp_rollout_legs with a model table: ``gaits.rollout_legs_host`` per group.  The legs step, like the plant,
    uses `body` (None: the configuration's), never the row; actuators [B,9] (per robot) or None.  Returns what
    ``gaits.rollout_legs_host`` returns."""
    from .gaits import rollout_legs_host
    return _legs_models_host(rollout_legs_host, oracle_lib, cfg_overrides, models, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height,
                             body, {"push": push, "push_ticks": push_ticks, "gains": gains, "actuators": actuators},
                             {"land": land, "substeps": substeps, "leg_substeps": leg_substeps, "inertia": inertia})


def rollout_drive_models_host(oracle_lib, cfg_overrides, models, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land="rule",
                              drive="limited", ground=None, body=None, push=None, push_ticks=None, substeps=DEFAULT_SUBSTEPS, gains=None,
                              leg_substeps=0, inertia=None, actuators=None):
    """Host checker of mpcqp_rollout_drive with a model table: ``gaits.rollout_drive_host`` per group (ground [B] and actuators [B,9] are
    per robot).
    Returns what ``gaits.rollout_drive_host`` returns."""
    from .gaits import rollout_drive_host
    return _legs_models_host(rollout_drive_host, oracle_lib, cfg_overrides, models, x, ref, feet, legs, gait, stand, gain, tick, mu, T,
                             step_height, body, {"push": push, "push_ticks": push_ticks, "gains": gains, "ground": ground, "actuators": actuators},
                             {"land": land, "drive": drive, "substeps": substeps, "leg_substeps": leg_substeps, "inertia": inertia})


def rollout_slip_models_host(oracle_lib, cfg_overrides, models, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, ground,
                             foot_mass, slip=None, land="rule", drive="limited", body=None, push=None, push_ticks=None,
                             substeps=DEFAULT_SUBSTEPS, gains=None, leg_substeps=0, inertia=None, actuators=None):
    """Host checker of mpcqp_rollout_slip with a model table: ``gaits.rollout_slip_host`` per group (ground [B], foot_mass [B] or a
    number, slip [B,4,2] or None and actuators [B,9] are per robot).
    Returns what ``gaits.rollout_slip_host`` returns."""
    from .gaits import rollout_slip_host
    if ground is None or foot_mass is None:
        raise ValueError("rollout_slip_models_host needs ground and foot_mass")
    B = np.asarray(x).shape[0]
    foot_mass = np.broadcast_to(np.asarray(foot_mass, np.float64), (B,))
    slip = None if slip is None else np.asarray(slip, np.float64).reshape(B, 4, 2)
    return _legs_models_host(rollout_slip_host, oracle_lib, cfg_overrides, models, x, ref, feet, legs, gait, stand, gain, tick, mu, T,
                             step_height, body, {"push": push, "push_ticks": push_ticks, "gains": gains, "ground": ground,
                                                 "foot_mass": foot_mass, "slip": slip, "actuators": actuators},
                             {"land": land, "drive": drive, "substeps": substeps, "leg_substeps": leg_substeps, "inertia": inertia})


def replay_rows(logs, pb, tick0, g):
    """Every logged (robot, tick) of a roll-out on a gait clock as an independent QP: the operands of ``solve_batch_phase`` (and of
    ``gaits.phase_expand_host``) for the B T rows, robot-major (row b T + t).  `logs` holds "actual", "desired" [B,T,12] and
    "feet_log" [B,T,4,3] as ``rollout_phase`` / ``rollout_legs`` / ``rollout_drive`` return them, `pb` the robots' constant rows
    ("gait", "stand", "gain" or None, "mu"), `tick0` [B] the tick BEFORE the roll-out, `g` the gravity entry x[:,12] (a scalar or [B]).
    Row (b, t) is x0 = [actual[b,t], g], ref = [desired[0:6], desired[9:12], desired[8]], feet = feet_log[b,t], tick = tick0[b] + t
    with robot b's gait, stand, gain and mu rows: what a COLD engine solved at that tick (a warm-started one also read its previous
    answer).  A model table is tiled the same way: ``np.repeat(models, T, axis=0)``."""
    actual, desired, feet_log = (np.asarray(logs[k]) for k in ("actual", "desired", "feet_log"))
    B, T = actual.shape[:2]
    rep = lambda a: np.repeat(np.asarray(a), T, axis=0)
    gcol = np.broadcast_to(np.asarray(g, actual.dtype).reshape(-1, 1, 1), (B, T, 1))
    x0 = np.concatenate([actual, gcol], axis=2).reshape(B * T, 13)
    ref = np.concatenate([desired[:, :, 0:6], desired[:, :, 9:12], desired[:, :, 8:9]], axis=2).reshape(B * T, 10)
    tick = (np.asarray(tick0, np.int32).reshape(B, 1) + np.arange(T, dtype=np.int32)[None, :]).reshape(B * T)
    return {"x": np.ascontiguousarray(x0), "ref": np.ascontiguousarray(ref), "feet": np.ascontiguousarray(feet_log.reshape(B * T, 4, 3)),
            "gait": rep(pb["gait"]), "tick": tick, "stand": rep(pb["stand"]), "gain": None if pb.get("gain") is None else rep(pb["gain"]),
            "mu": rep(pb["mu"])}
