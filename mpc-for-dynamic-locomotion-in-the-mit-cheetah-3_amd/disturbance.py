"""Host counterpart of the per-robot disturbance wrench rows and the wrench observer (include/mpcqp_disturb.h, which has the rule):
numpy fp64, vectorised over robots.

A constant wrench on the MPC's model adds an affine term to every stage of X[k+1] = Ad X[k] + Bd_k U[k].  With s[0] = 0,
s[k+1] = Ad s[k] + Cd the disturbed QP is the undisturbed one with xdes - s in the place of xdes, and its states are the solver's
plus s.  ``shift_host`` forms s by that recursion with explicit 13 x 13 matrices -- the device writes the closed form --,
``DisturbedEngine`` wraps a checker handle so that every host roll-out of ``gaits`` and ``plant`` runs with a table unchanged,
``disturbance_track_host`` is the observer in the device's operation order, and ``compensated_rollout`` closes the loop between the
two piece by piece, on either side.  ``rollout_compensated_host`` is that loop over ``gaits.rollout_observe_host``: the host counterpart of
mpcqp_rollout_observe_compensated (include/mpcqp_compensate.h), where the device runs the observer inside the roll-out's tick.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from .plant import inertia_inverse, model_body, quat_to_matrix, rollout_loop_host, rotvec_to_quat

ROW = 6                       # (F_x, F_y, F_z, tau_x, tau_y, tau_z): a `push` row
STATE = _capi.DIST_STATE      # d^ (6) | previous row: L (3), v (3), p (3), f (12), feet (12) | live
_PREV, _LIVE = 6, 39
OUT = ("dist", "resid")
# the defaults of mpcqp_default_wrench_observer: inputs, not measurements
OBSERVER_DEFAULTS = {"gravity": -9.81, "kappa": 0.2, "f_lim": float("inf"), "t_lim": float("inf")}


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def wrench_rows(B):
    """The table that tells the MPC nothing: zeros [B,6] fp64.  Fill rows[:, 0:3] with F, rows[:, 3:6] with tau."""
    return np.zeros((int(B), ROW))


def observer_row(**kw):
    """The observer's parameters as a dict: the defaults of mpcqp_default_wrench_observer with `kw` over them, checked as the library
    checks an MpcQpWrenchObserver."""
    unknown = set(kw) - set(OBSERVER_DEFAULTS)
    if unknown:
        raise ValueError(f"MpcQpWrenchObserver has no field {sorted(unknown)}; the fields are {tuple(OBSERVER_DEFAULTS)}")
    row = {k: float(kw.get(k, v)) for k, v in OBSERVER_DEFAULTS.items()}
    if not np.isfinite(row["gravity"]) or not row["gravity"] < 0:
        raise ValueError("wrench observer: gravity must be finite and negative")
    if not 0 <= row["kappa"] <= 1:
        raise ValueError("wrench observer: kappa must be in [0, 1]")
    if not row["f_lim"] >= 0 or not row["t_lim"] >= 0:
        raise ValueError("wrench observer: f_lim and t_lim must be non-negative (infinity: no clamp)")
    return row


def observer_struct(observer):
    """None, an MpcQpWrenchObserver, or a dict of `observer_row`'s fields -> what the binding passes (None = the library's defaults)."""
    if observer is None or isinstance(observer, _capi.MpcQpWrenchObserver):
        return observer
    row = observer_row(**observer)
    par = _capi.MpcQpWrenchObserver()
    par.size = _capi.ctypes.sizeof(_capi.MpcQpWrenchObserver)
    for k, v in row.items():
        setattr(par, k, v)
    return par


SOURCES = {"truth": _capi.WRENCH_TRUTH, "sensed": _capi.WRENCH_SENSED}
COMPENSATE_DEFAULTS = {"source": "truth", "hold": 1, "body": None}     # what a `compensate` dict has besides the observer's fields


def compensate_row(**kw):
    """A `compensate` dict in full: `observer_row`'s fields (checked there), "source" ("truth" or "sensed"; an int goes to the library as
    it is), "hold" (>= 1) and "body" ([B,7], the body the observer believes, or None: the handle's model)."""
    unknown = set(kw) - set(OBSERVER_DEFAULTS) - set(COMPENSATE_DEFAULTS)
    if unknown:
        raise ValueError(f"compensate has no field {sorted(unknown)}; the fields are {tuple(OBSERVER_DEFAULTS) + tuple(COMPENSATE_DEFAULTS)}")
    row = {**COMPENSATE_DEFAULTS, **{k: kw[k] for k in COMPENSATE_DEFAULTS if k in kw}}
    if not isinstance(row["source"], int) and row["source"] not in SOURCES:
        raise ValueError(f"source must be 'truth' or 'sensed', got {row['source']!r}")
    if int(row["hold"]) != row["hold"] or row["hold"] < 1:
        raise ValueError(f"hold must be a whole number >= 1, got {row['hold']!r}")
    row["hold"] = int(row["hold"])
    return {**observer_row(**{k: v for k, v in kw.items() if k in OBSERVER_DEFAULTS}), **row}


def compensate_struct(compensate, gated=False, aided=False):
    """A `compensate` dict ({} = the defaults) or an MpcQpCompensate -> (the structure the binding passes, with the flags of the
    estimator variant that runs, and the observer's body or None).  A structure is passed as it is: the library checks it."""
    if isinstance(compensate, _capi.MpcQpCompensate):
        return compensate, None
    row = compensate_row(**compensate)
    par = _capi.MpcQpCompensate()
    par.size = _capi.ctypes.sizeof(_capi.MpcQpCompensate)
    par.flags = (_capi.COMP_GATED if gated else 0) | (_capi.COMP_AIDED if aided else 0)
    par.source = row["source"] if isinstance(row["source"], int) else SOURCES[row["source"]]
    par.hold = row["hold"]
    par.observer.size = _capi.ctypes.sizeof(_capi.MpcQpWrenchObserver)
    for k in OBSERVER_DEFAULTS:
        setattr(par.observer, k, row[k])
    return par, row["body"]


def offsets_host(x0, rows, cfg, models=None):
    """s [B,N+1,13] of the rule, by the plain recursion s[k+1] = Ad s[k] + Cd on explicit matrices, and which robots are finite [B].
    cfg: the handle's MpcQpConfig (N, delta, disc, m, Ibody_inv); models [B,6] = (m, Ixx, Iyy, Izz, f_min, f_max) or None."""
    x0, rows = _f64(x0), _f64(rows)
    B, N, d = x0.shape[0], int(cfg.N), float(cfg.delta)
    if rows.shape != (B, ROW):
        raise ValueError(f"rows must be [{B},{ROW}], got {rows.shape}")
    inv_m = np.full(B, 1.0 / float(cfg.m))
    ib = np.tile(_f64(list(cfg.Ibody_inv)), (B, 1))
    if models is not None:
        mod = _f64(models)
        ok = np.isfinite(mod).all(axis=1) & (mod[:, :4] > 0).all(axis=1) & (mod[:, 4] >= 0) & (mod[:, 5] >= mod[:, 4])
        with np.errstate(divide="ignore", invalid="ignore"):
            inv_m, ib = np.where(ok, 1.0 / mod[:, 0], np.nan), np.where(ok[:, None], 1.0 / mod[:, 1:4], np.nan)
    fin = np.isfinite(rows).all(axis=1) & np.isfinite(x0[:, 2]) & np.isfinite(inv_m) & np.isfinite(ib).all(axis=1)
    s = np.zeros((B, N + 1, 13))
    eye = np.eye(13)
    for b in np.nonzero(fin)[0]:
        cs, sn = np.cos(x0[b, 2]), np.sin(x0[b, 2])
        Rz = np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]])
        A = np.zeros((13, 13))
        A[0:3, 6:9] = Rz
        A[3:6, 9:12] = np.eye(3)
        A[11, 12] = 1.0
        c = np.zeros(13)
        c[6:9] = Rz @ np.diag(ib[b]) @ Rz.T @ rows[b, 3:6]
        c[9:12] = rows[b, 0:3] * inv_m[b]
        if cfg.disc == _capi.DISC_ZOH:
            Ad, Cd = eye + d * A + 0.5 * d * d * (A @ A), (d * eye + 0.5 * d * d * A) @ c
        else:
            Ad, Cd = eye + d * A, d * c
        for k in range(N):
            s[b, k + 1] = Ad @ s[b, k] + Cd
    return s, fin


def shift_host(x0, xdes, rows, cfg, models=None):
    """mpcqp_disturbance_shift on the host: xdes - s [B,N+1,13], NaN for a robot whose wrench row, model row or yaw is not finite."""
    s, fin = offsets_host(x0, rows, cfg, models)
    return np.where(fin[:, None, None], _f64(xdes) - s, np.nan)


class DisturbedEngine:
    """A checker handle (``Engine`` on the CPU checker library) with a disturbance table: ``solve_batch_host`` solves the tuple with
    xdes - s and returns X + s, and ``rollout_host`` -- the handle's is the checker's C loop, which calls the C solve and never sees the
    table -- runs ``plant.rollout_loop_host``, the same loop in Python over that ``solve_batch_host``, while rows are set.  Every other
    attribute is the handle's.  So the host loops that solve through ``solve_batch_host`` (``gaits.rollout_phase_host``, ``_legs_``,
    ``_drive_``, ``_slip_`` and ``_observe_host``) and those that solve through ``rollout_host`` (``plant.rollout_plant_host``) run under a
    table unchanged.  rows [B,6] or None (no table); `models` [B,6] only where the device has a model table set as well (the handle
    itself has one model: group the robots by row, models.grouped_host, and wrap each group's handle)."""

    def __init__(self, oracle_engine, rows=None, models=None):
        self._engine, self.models = oracle_engine, models
        self.set_rows(rows)

    def set_rows(self, rows):
        self.rows = None if rows is None else _f64(rows).copy()

    def __getattr__(self, name):
        return getattr(self._engine, name)

    def solve_batch_host(self, x0, r, contact, xdes, mu, want_X=True):
        if self.rows is None:
            return self._engine.solve_batch_host(x0, r, contact, xdes, mu, want_X=want_X)
        s, fin = offsets_host(x0, self.rows, self._engine.cfg, self.models)
        out = self._engine.solve_batch_host(x0, r, contact, np.where(fin[:, None, None], _f64(xdes) - s, np.nan), mu, want_X=want_X)
        if want_X and out.get("X") is not None:
            out["X"] = out["X"] + np.where(fin[:, None, None], s, 0.0)
        return out

    def rollout_host(self, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T):
        if self.rows is None:
            return self._engine.rollout_host(x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T)
        return rollout_loop_host(self, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T)


def _mv(R, v):    # R v and R^T v in the device's order (csrc/mpcqp_estimate.h, est_mv / est_mtv); R [B,3,3], v a list of three [B]
    return [(R[:, i, 0] * v[0] + R[:, i, 1] * v[1]) + R[:, i, 2] * v[2] for i in range(3)]


def _mtv(R, v):
    return [(R[:, 0, i] * v[0] + R[:, 1, i] * v[1]) + R[:, 2, i] * v[2] for i in range(3)]


def disturbance_track_host(logs, cfg, body=None, observer=None, state=None, feet="feet_log"):
    """mpcqp_disturbance_track on the host, in the device's operation order: `logs` with "actual", "forces" [B,T,12] and logs[feet]
    [B,T,4,3]; cfg the handle's MpcQpConfig (delta, and m, Ibody_inv for body = None); body [B,7] or None; observer None or a dict of
    `observer_row`'s fields; state [B,40] or None (not modified) -> {"dist", "resid" [B,T,6], "state" [B,40]}."""
    par = observer_row(**(observer or {}))
    actual, forces, ft_log = _f64(logs["actual"]), _f64(logs["forces"]), _f64(logs[feet])
    B, T = actual.shape[:2]
    d, g, kap = float(cfg.delta), par["gravity"], par["kappa"]
    lim = np.array([par["f_lim"]] * 3 + [par["t_lim"]] * 3)
    bd = model_body(cfg.m, list(cfg.Ibody_inv), B) if body is None else _f64(body).reshape(B, 7)
    m, Ib = bd[:, 0], [bd[:, 1 + i] for i in range(6)]
    ok = inertia_inverse(m, Ib)[1].copy()
    st = np.zeros((B, STATE)) if state is None else _f64(state).reshape(B, STATE).copy()
    ok &= np.isfinite(st).all(axis=1)
    live = st[:, _LIVE] != 0.0
    dh, Lp, vp, pp = st[:, 0:6].copy(), st[:, _PREV:_PREV + 3].copy(), st[:, _PREV + 3:_PREV + 6].copy(), st[:, _PREV + 6:_PREV + 9].copy()
    fp, ftp = st[:, _PREV + 9:_PREV + 21].reshape(B, 4, 3).copy(), st[:, _PREV + 21:_PREV + 33].reshape(B, 4, 3).copy()
    dist, resid = np.zeros((B, T, 6)), np.zeros((B, T, 6))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t in range(T):
            row = actual[:, t]
            f = forces[:, t].reshape(B, 4, 3)
            on = (f != 0.0).any(axis=2)
            ft = np.where(on[:, :, None], ft_log[:, t], 0.0)
            ok &= np.isfinite(row).all(axis=1) & np.isfinite(f).all(axis=(1, 2)) & np.isfinite(ft).all(axis=(1, 2))
            R = quat_to_matrix(rotvec_to_quat(row[:, 0:3]))
            wb = _mtv(R, [row[:, 6], row[:, 7], row[:, 8]])
            Lb = [(Ib[0] * wb[0] + Ib[3] * wb[1]) + Ib[4] * wb[2], (Ib[3] * wb[0] + Ib[1] * wb[1]) + Ib[5] * wb[2],
                  (Ib[4] * wb[0] + Ib[5] * wb[1]) + Ib[2] * wb[2]]
            L = np.stack(_mv(R, Lb), axis=1)
            v, p = row[:, 9:12], row[:, 3:6]
            pm = 0.5 * (pp + p)
            onp = (fp != 0.0).any(axis=2)
            r = ftp - pm[:, None, :]
            cr = np.stack([r[..., 1] * fp[..., 2] - r[..., 2] * fp[..., 1], r[..., 2] * fp[..., 0] - r[..., 0] * fp[..., 2],
                           r[..., 0] * fp[..., 1] - r[..., 1] * fp[..., 0]], axis=-1)
            cr = np.where(onp[:, :, None], cr, 0.0)
            Fs = (fp[:, 0] + fp[:, 1]) + (fp[:, 2] + fp[:, 3])
            Ms = (cr[:, 0] + cr[:, 1]) + (cr[:, 2] + cr[:, 3])
            rf = (m[:, None] * (v - vp)) / d - Fs
            rf[:, 2] = rf[:, 2] - m * g
            rt = (L - Lp) / d - Ms
            res = np.where(live[:, None], np.concatenate([rf, rt], axis=1), 0.0)
            upd = dh + kap * (res - dh)
            upd = np.where(upd > lim, lim, np.where(upd < -lim, -lim, upd))
            dh = np.where(live[:, None], upd, dh)
            dist[:, t] = np.where(ok[:, None], dh, np.nan)
            resid[:, t] = np.where(ok[:, None], res, np.nan)
            Lp, vp, pp, fp, ftp = L, v.copy(), p.copy(), f.copy(), ft
            live = np.ones(B, bool)
    out = np.concatenate([dh, Lp, vp, pp, fp.reshape(B, 12), ftp.reshape(B, 12), live[:, None].astype(np.float64)], axis=1)
    return {"dist": dist, "resid": resid, "state": np.where(ok[:, None], out, np.nan)}


def compensated_rollout(step, T, piece, track, setter, state=None):
    """Roll T ticks in pieces of at most `piece` with the observer closing the loop between them (in the style of
    score.scored_rollout): `step(n)` is the caller's closure over one of the in-place roll-outs and returns that piece's logs;
    `track(logs, state)` runs the observer on them with the carried state (`lambda logs, st: sol.disturbance_track(logs, state=st)` on
    the device, which advances `st` in place, or a closure over `disturbance_track_host`) and returns {"dist", "resid", "state"};
    `setter(rows)` makes the last "dist" row, as fp64 [B,6], the table of the next piece (`sol.set_disturbance`, or
    `DisturbedEngine.set_rows`).  piece = 1 is row-by-row adaptation.  On the device everything is enqueued on one stream and nothing is
    synchronised between the pieces.  Returns {"logs": the pieces' logs joined along T ("solved" summed), "dist", "resid" [B,T,6],
    "state"}."""
    T, piece = int(T), int(piece)
    if piece < 1:
        raise ValueError(f"piece must be >= 1, got {piece}")
    pieces, dist, resid, done = [], [], [], 0
    while done < T:
        n = min(piece, T - done)
        logs = step(n)
        out = track(logs, state)
        state = out["state"]
        last = out["dist"][:, -1]
        setter(last.double().contiguous() if hasattr(last, "data_ptr") else np.ascontiguousarray(last, dtype=np.float64))
        pieces.append(logs); dist.append(out["dist"]); resid.append(out["resid"])
        done += n
    return {"logs": _join(pieces), "dist": _cat(dist), "resid": _cat(resid), "state": state}


def _cat(parts):
    if not parts:
        return None
    if hasattr(parts[0], "data_ptr"):
        import torch
        return torch.cat(parts, dim=1)
    return np.concatenate(parts, axis=1)


def _join(pieces):
    """The logs of consecutive pieces as one: every [B,T,...] entry joined along T, "solved" summed, anything else the last piece's."""
    out = {}
    for k in (pieces[-1] if pieces else {}):
        vals = [p[k] for p in pieces]
        if vals[0] is None:
            out[k] = None
        elif k == "solved":
            out[k] = sum(vals[1:], vals[0])
        elif k in ("actual", "desired", "forces") or k.endswith("_log"):
            out[k] = _cat(vals)
        else:
            out[k] = vals[-1]
    return out


SENSED_LOGS = {"actual": "est", "forces": "cmd", "feet_log": "feet_est"}      # what the observer reads of `rollout_observe`'s logs


def sensed_logs(logs):
    """The logs of a `rollout_observe` under the names the observer reads: what a robot has in the place of the plant's truth."""
    return {k: logs[src] for k, src in SENSED_LOGS.items()}


def rollout_compensated_host(oracle_engine, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, ground, foot_mass, compensate=None,
                             dist_state=None, slip=None, est_state=None, att_state=None, noise=None, enc_noise=None, models=None, **kw):
    """mpcqp_rollout_observe_compensated (include/mpcqp_compensate.h, which has the rule) on the CPU checker, composed from what
    exists and nothing else: `compensated_rollout` at piece = hold over `gaits.rollout_observe_host` on a `DisturbedEngine` whose rows
    start from dist_state[:, :6], with `disturbance_track_host` on the truth logs (source "truth") or on "est", "cmd" and "feet_est"
    (source "sensed").  `compensate`: None or a dict as `compensate_row` takes it; dist_state [B,40] or None (a fresh observer);
    slip, est_state, att_state, noise [B,T,6], enc_noise [B,T,4,6] and every keyword of `rollout_observe_host` as there (the noise
    rows are cut to each piece); `models` as `DisturbedEngine` takes it.  Nothing is modified in place.  Returns
    `rollout_observe_host`'s dict for the T ticks plus "dist", "resid" [B,T,6] and "dist_state" [B,40]."""
    from . import gaits
    row = compensate_row(**(compensate or {}))
    if isinstance(row["source"], int) and row["source"] not in SOURCES.values():
        raise ValueError(f"source must be 'truth' or 'sensed', got {row['source']!r}")
    sensed = row["source"] in ("sensed", _capi.WRENCH_SENSED)
    B, T = np.asarray(x).shape[0], int(T)
    state = np.zeros((B, STATE)) if dist_state is None else _f64(dist_state).reshape(B, STATE).copy()
    eng = DisturbedEngine(oracle_engine, state[:, :ROW], models)
    st = {"x": _f64(x), "ref": _f64(ref), "feet": _f64(feet), "legs": _f64(legs), "tick": np.asarray(tick, np.int32), "slip": slip,
          "est_state": est_state, "att_state": att_state}
    done, pieces = [0], []

    def step(n):
        cut = lambda a: None if a is None else _f64(a)[:, done[0]:done[0] + n]
        carried = {k: st[k] for k in ("slip", "est_state")}
        if kw.get("attitude") is not None:
            carried["att_state"] = st["att_state"]
        o = gaits.rollout_observe_host(eng, st["x"], st["ref"], st["feet"], st["legs"], gait, stand, gain, st["tick"], mu, n, step_height, ground,
                                       foot_mass, noise=cut(noise), enc_noise=cut(enc_noise), **carried, **kw)
        st.update({k: o[k] for k in st if k in o})
        done[0] += n
        pieces.append(o)
        return o

    obs = {k: row[k] for k in OBSERVER_DEFAULTS}
    track = lambda logs, s: disturbance_track_host(sensed_logs(logs) if sensed else logs, eng.cfg, body=row["body"], observer=obs, state=s)
    out = compensated_rollout(step, T, row["hold"], track, eng.set_rows, state)
    if not pieces:
        step(0)
    # (`compensated_rollout` joins the logs it knows by name; a leg roll-out's dict has more: every key but the carried state is a log)
    carried = ("x", "ref", "tick", "feet", "legs", "slip", "est_state", "att_state")
    logs = {k: pieces[-1][k] if k in carried else (sum(p[k] for p in pieces) if k == "solved" else np.concatenate([p[k] for p in pieces], axis=1))
            for k in pieces[-1]}
    return {**logs, "dist": np.zeros((B, 0, ROW)) if out["dist"] is None else out["dist"],
            "resid": np.zeros((B, 0, ROW)) if out["resid"] is None else out["resid"], "dist_state": out["state"]}
