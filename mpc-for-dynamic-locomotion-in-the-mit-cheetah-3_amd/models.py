"""Per-robot model rows (include/mpcqp_model.h): row helpers and the host checkers.

A model row is ``(m, Ixx, Iyy, Izz, f_min, f_max)`` -- the mass, the principal inertias in the torso frame and the f_z box of ONE
robot's MPC, fp64.  ``MPCBatch.set_models`` hands a table of them to the device engine.  The CPU checker under ``oracle/`` has one
model per handle, so the checkers here group the batch by identical row and solve each group with a handle of its own, created
with that row's ``m``, ``Ibody_inv = 1 / I``, ``f_min`` and ``f_max``.
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
    out = None
    for row, idx in _groups(models, B):
        kw = dict(cfg_overrides); kw.update(row_overrides(row))
        eng = _capi.Engine(oracle_lib, oracle_lib.default_config(**kw))
        o = eng.solve_batch_host(batch["x0"][idx], batch["r"][idx], batch["contact"][idx], batch["xdes"][idx], batch["mu"][idx], want_X=want_X)
        eng.close()
        if out is None:
            out = {k: (None if v is None else np.zeros((B,) + v.shape[1:], v.dtype)) for k, v in o.items()}
        for k, v in o.items():
            if v is not None:
                out[k][idx] = v
    return out


def rollout_plant_models_host(oracle_lib, cfg_overrides, models, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T, body=None, push=None,
                              push_ticks=None, substeps=DEFAULT_SUBSTEPS):
    """Host checker of mpcqp_rollout_plant with a model table: ``plant.rollout_plant_host`` per group of robots with an identical
    row, each with a checker handle of that row's model.  body = None steps the plant with the CONFIGURATION's model
    (`cfg_overrides`), as the device does.  Returns the advanced (x, ref, tick) and the logs, as ``plant.rollout_plant_host``."""
    from .plant import model_body
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    if body is None:
        base = oracle_lib.default_config(**cfg_overrides)
        body = model_body(base.m, list(base.Ibody_inv), B)
    body = np.asarray(body, np.float64)
    sub = lambda a, idx: None if a is None else np.asarray(a)[idx]
    out = None
    for row, idx in _groups(models, B):
        kw = dict(cfg_overrides); kw.update(row_overrides(row))
        eng = _capi.Engine(oracle_lib, oracle_lib.default_config(**kw))
        o = rollout_plant_host(eng, x[idx], np.asarray(ref)[idx], np.asarray(plan_pos)[idx], np.asarray(plan_feet_id)[idx],
                               np.asarray(plan_meta)[idx], np.asarray(tick)[idx], np.asarray(mu)[idx], T, body=body[idx],
                               push=sub(push, idx), push_ticks=sub(push_ticks, idx), substeps=substeps)
        eng.close()
        if out is None:
            out = {k: np.zeros((B,) + v.shape[1:], v.dtype) for k, v in o.items()}
        for k, v in o.items():
            out[k][idx] = v
    return out
