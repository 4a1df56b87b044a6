"""Per-robot actuator rows with a torque-speed curve (include/mpcqp_actuators.h, which has the envelope and the rules): the row
helpers and the host counterpart of the device's clamp, numpy fp64 in the device's order of operations.

A row is ``(tau_max[3], qd_knee[3], qd_free[3])`` for HipX, HipY, Knee: the torque at standstill, the rate up to which it is
available and the no-load rate at which the motoring torque reaches zero.  ``qd_knee = inf`` is the flat box of the inertia row.
`MPCBatch.set_actuators` takes a table of them; `lite3_model.swing_track_host`, `stance_drive_host`, `leg_effort_host` and
`gaits.rollout_legs_host` / `rollout_drive_host` take the same table as ``actuators=``.
"""
from __future__ import annotations

import numpy as np

ROW = 9


def actuator_rows(B, inertia=None, scale=1.0, knee=np.inf, free=np.inf):
    """float64 [B,9] rows from an inertia row (a dict as `lite3_model.leg_inertia`, None = the Lite3): tau_max = inertia["tau_max"] *
    scale, qd_knee = knee * qd_max, qd_free = free * qd_max.  `scale`, `knee` and `free` are scalars, [B] or [B,3]; knee and free are
    fractions of the row's qd_max (inf: no falling part).  The defaults give the flat Lite3: a table that is no table."""
    from . import lite3_model
    inr = lite3_model._inertia_arrays(inertia)

    def cols(v):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 1:
            v = v[:, None]
        return np.broadcast_to(v, (B, 3))

    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray(np.concatenate([inr["tau_max"] * cols(scale), cols(knee) * inr["qd_max"], cols(free) * inr["qd_max"]], axis=1))


def valid_rows(rows):
    """bool [B]: the row passes the conversion kernel's check -- every tau_max finite and >= 0, every qd_knee >= 0, and per joint
    qd_knee = +inf or finite qd_knee < qd_free < inf."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    tm, kn, fr = rows[:, 0:3], rows[:, 3:6], rows[:, 6:9]
    with np.errstate(invalid="ignore"):
        flat = kn == np.inf
        curve = np.isfinite(kn) & np.isfinite(fr) & (fr > kn)
        return (np.isfinite(tm) & (tm >= 0.0) & (kn >= 0.0) & (flat | curve)).all(axis=1)


def _checked(rows, nd):
    """The table as the engine keeps it (an invalid row NaN), as (tau_max, qd_knee, qd_free), each [B,1,..,3] against nd-dim operands."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    rows = np.where(valid_rows(rows)[:, None], rows, np.nan)
    shape = (rows.shape[0],) + (1,) * (nd - 2) + (3,)
    return rows[:, 0:3].reshape(shape), rows[:, 3:6].reshape(shape), rows[:, 6:9].reshape(shape)


def limits_host(rows, qd):
    """(lo, hi) of the envelope at the joint rates qd [B,...,3] under rows [B,9]: hi = avail on the side of qd's sign and tau_max on
    the other, lo likewise; avail = tau_max up to |qd| = qd_knee, then tau_max * (max(qd_free - |qd|, 0) / (qd_free - qd_knee)).  An
    invalid row gives NaN."""
    qd = np.asarray(qd, dtype=np.float64)
    tm, kn, fr = _checked(rows, qd.ndim)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = np.abs(qd)
        d = fr - a
        tmb = np.broadcast_to(tm, a.shape)
        avail = np.where(a > kn, tm * (np.where(d > 0.0, d, 0.0) / (fr - kn)), tmb)
        return np.where(qd < 0.0, -avail, -tmb), np.where(qd > 0.0, avail, tmb)


def clamp_host(rows, cmd, qd):
    """The applied torque of the commanded cmd [B,...,3] at the rates qd under rows [B,9], as the device selects it: cmd > hi ? hi :
    (cmd < lo ? lo : cmd); a NaN cmd stays, an invalid row gives NaN."""
    cmd = np.asarray(cmd, dtype=np.float64)
    lo, hi = limits_host(rows, qd)
    with np.errstate(invalid="ignore"):
        app = np.where(cmd > hi, hi, np.where(cmd < lo, lo, cmd))
    return np.where(np.isnan(lo), np.nan, app)


def margin_host(rows, cmd, qd):
    """[B,...]: the smallest distance |value - threshold| / max(1, |threshold|) over a leg's joints to a comparison that decides its
    clamp: |qd_j| at qd_knee and at qd_free, cmd_j at lo_j and hi_j.  An infinite threshold is never near; an invalid row gives inf."""
    cmd, qd = np.asarray(cmd, dtype=np.float64), np.asarray(qd, dtype=np.float64)
    tm, kn, fr = _checked(rows, qd.ndim)
    lo, hi = limits_host(rows, qd)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        def rel(val, thr):
            m = np.abs(val - thr) / np.maximum(1.0, np.abs(thr))
            return np.where(np.isfinite(thr) & np.isfinite(val), m, np.inf)
        a = np.abs(qd)
        kn, fr = np.broadcast_to(kn, a.shape), np.broadcast_to(fr, a.shape)
        free = np.where(np.isfinite(kn), rel(a, fr), np.inf)      # (a flat row never reads its qd_free)
        m = np.minimum(np.minimum(rel(a, kn), free), np.minimum(rel(cmd, lo), rel(cmd, hi)))
    return m.min(axis=-1)


def tile(rows, T):
    """The table of the B T logged rows of a roll-out, robot-major: row b repeated T times (what `stance_drive` wants next to
    `models.replay_rows`)."""
    return np.repeat(np.asarray(rows, dtype=np.float64).reshape(-1, ROW), int(T), axis=0)
