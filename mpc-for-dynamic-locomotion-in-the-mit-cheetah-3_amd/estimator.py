"""The torso state estimated from an IMU and leg kinematics, on the host (the counterparts of include/mpcqp_estimate.h, which has the
rule): `imu_log_host` (mpcqp_imu_log), `estimate_track_host` (mpcqp_estimate_track: three 6-state filters with scalar updates, in the
device's operation order) and `estimate_joint_host`, the same filter in its textbook form -- 18 states, all measurements of a row in
one batch update through np.linalg.solve, the orientation through scipy's Rotation -- which shares only the leg kinematics with the
other and is the check that the rule is the Kalman filter it claims to be.  fp64 numpy, vectorised over the robots.
"""
from __future__ import annotations

import numpy as np

from . import lite3_model, plant

EST_STATE = 131            # include/mpcqp_estimate.h, MPCQP_EST_STATE
_XI, _P, _LIVE = 4, 22, 130
DEFAULTS = {"gravity": -9.81, "kappa": 2.0, "q_p": 0.02, "q_v": 0.02, "q_f": 0.002, "r_p": 0.001, "r_v": 0.1, "r_z": 0.001,
            "k_swing": 100.0, "p0_p": 0.01, "p0_v": 1.0, "p0_f": 0.01}
OUT = ("est", "feet", "sigma", "nis")
GATE_DEFAULTS = {"d_lo": 1.0, "d_hi": 4.0}            # include/mpcqp_gate.h, mpcqp_default_trust_gate
ATT_STATE = 8              # include/mpcqp_attitude.h, MPCQP_ATT_STATE
ATT_DEFAULTS = {"k_s": 0.0, "k_v": 2.0, "k_b": 5.0, "b_max": 0.1}            # include/mpcqp_attitude.h, mpcqp_default_attitude


def estimator_row(**kw):
    """The estimator's parameters as a dict: the defaults of mpcqp_default_estimator with `kw` over them, checked as the library checks
    an MpcQpEstimator (finite; gravity negative; kappa, the noises and k_swing non-negative)."""
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"MpcQpEstimator has no field {sorted(unknown)}; the fields are {tuple(DEFAULTS)}")
    row = {k: float(kw.get(k, v)) for k, v in DEFAULTS.items()}
    if not np.isfinite(row["gravity"]) or not row["gravity"] < 0:
        raise ValueError("estimator: gravity must be finite and negative")
    for k, v in row.items():
        if k != "gravity" and (not np.isfinite(v) or not v >= 0):
            raise ValueError(f"estimator: {k} must be finite and non-negative")
    return row


def estimator_struct(estimator):
    """None, an MpcQpEstimator, or a dict of `estimator_row`'s fields -> what the binding passes (None = the library's defaults)."""
    from . import _capi
    if estimator is None or isinstance(estimator, _capi.MpcQpEstimator):
        return estimator
    row = estimator_row(**estimator)
    par = _capi.MpcQpEstimator()
    par.size = _capi.ctypes.sizeof(_capi.MpcQpEstimator)
    for k, v in row.items():
        setattr(par, k, v)
    return par


def _row(estimator):
    return estimator_row(**(estimator or {}))


def gate_row(**kw):
    """The trust gate's thresholds as a dict: the defaults of mpcqp_default_trust_gate with `kw` over them, checked as the library
    checks an MpcQpTrustGate (finite, 0 <= d_lo < d_hi)."""
    unknown = set(kw) - set(GATE_DEFAULTS)
    if unknown:
        raise ValueError(f"MpcQpTrustGate has no field {sorted(unknown)}; the fields are {tuple(GATE_DEFAULTS)}")
    row = {k: float(kw.get(k, v)) for k, v in GATE_DEFAULTS.items()}
    if not (np.isfinite(row["d_lo"]) and np.isfinite(row["d_hi"]) and 0 <= row["d_lo"] < row["d_hi"]):
        raise ValueError("trust gate: d_lo and d_hi must be finite with 0 <= d_lo < d_hi")
    return row


def gate_struct(gate):
    """An MpcQpTrustGate, or a dict of `gate_row`'s fields ({} = the defaults) -> the structure the binding passes."""
    from . import _capi
    if isinstance(gate, _capi.MpcQpTrustGate):
        return gate
    row = gate_row(**gate)
    par = _capi.MpcQpTrustGate()
    par.size = _capi.ctypes.sizeof(_capi.MpcQpTrustGate)
    par.d_lo, par.d_hi = row["d_lo"], row["d_hi"]
    return par


def attitude_row(**kw):
    """The aided attitude rule's gains as a dict: the defaults of mpcqp_default_attitude with `kw` over them, checked as the library
    checks an MpcQpAttitude (finite and non-negative)."""
    unknown = set(kw) - set(ATT_DEFAULTS)
    if unknown:
        raise ValueError(f"MpcQpAttitude has no field {sorted(unknown)}; the fields are {tuple(ATT_DEFAULTS)}")
    row = {k: float(kw.get(k, v)) for k, v in ATT_DEFAULTS.items()}
    for k, v in row.items():
        if not np.isfinite(v) or not v >= 0:
            raise ValueError(f"attitude: {k} must be finite and non-negative")
    return row


def attitude_struct(attitude):
    """An MpcQpAttitude, or a dict of `attitude_row`'s fields ({} = the defaults) -> the structure the binding passes."""
    from . import _capi
    if isinstance(attitude, _capi.MpcQpAttitude):
        return attitude
    row = attitude_row(**attitude)
    par = _capi.MpcQpAttitude()
    par.size = _capi.ctypes.sizeof(_capi.MpcQpAttitude)
    for k, v in row.items():
        setattr(par, k, v)
    return par


def _att_operands(att_state, fresh, B):
    """b^ [B,3] at the start of a call (zero for a fresh robot and without att_state) and whether what was read is finite [B]."""
    if att_state is None:
        return np.zeros((B, 3)), np.ones(B, bool)
    ast = np.array(att_state, dtype=np.float64).reshape(B, ATT_STATE)
    bh = np.where(fresh[:, None], 0.0, ast[:, 0:3])
    return bh, np.isfinite(bh).all(-1)


def _att_state(bh, eb, ok):
    out = np.zeros((bh.shape[0], ATT_STATE))
    out[:, 0:3], out[:, 3:6] = bh, eb
    out[~ok] = np.nan
    return out


def trust_gate(gate, par, xi, P, rhod, c, io_dtype=np.float64):
    """Step 1g of the row (include/mpcqp_gate.h) in the device's order: xi [3,6,B] and P [3,6,6,B] the predicted state, rhod [B,4,3], c
    [B,4] the ungated trust -> (w [B,4] as `io_dtype` holds it, d [B,4])."""
    lo, hi = gate["d_lo"], gate["d_hi"]
    m = []
    for a in range(2):
        e = (-rhod[:, :, a]) - xi[a, 1][:, None]
        S = P[a, 1, 1] + par["r_v"]
        m.append((e * e) / S[:, None])
    d = m[0] + m[1]
    g = np.where(d <= lo, 1.0, np.where(d < hi, (hi - d) / (hi - lo), 0.0))
    return (c * g).astype(io_dtype).astype(np.float64), d


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _mv(R, v):      # R [...,3,3], v [...,3] in the device's order
    return np.stack([(R[..., a, 0] * v[..., 0] + R[..., a, 1] * v[..., 1]) + R[..., a, 2] * v[..., 2] for a in range(3)], axis=-1)


def _mtv(R, v):     # R^T v
    return np.stack([(R[..., 0, a] * v[..., 0] + R[..., 1, a] * v[..., 1]) + R[..., 2, a] * v[..., 2] for a in range(3)], axis=-1)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def quat_mul(a, b):
    """Hamilton product of (w, x, y, z) rows, in the device's order."""
    return np.stack([((a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1]) - a[..., 2] * b[..., 2]) - a[..., 3] * b[..., 3],
                     ((a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]) + a[..., 2] * b[..., 3]) - a[..., 3] * b[..., 2],
                     ((a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3]) + a[..., 2] * b[..., 0]) + a[..., 3] * b[..., 1],
                     ((a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2]) - a[..., 2] * b[..., 1]) + a[..., 3] * b[..., 0]], axis=-1)


def imu_log_host(actual, forces, feet, base_acc=None, body=None, bias=None, noise=None, estimator=None):
    """What an IMU at the CoM reads on every row of a log (mpcqp_imu_log): actual, forces [B,T,12], feet [B,T,4,3] (not read),
    base_acc [B,T,6] = (alpha, a) or None for the unpushed plant's a = sum f / m + g e_z with body [B,7] (None: the default handle's
    model); bias [B,6], noise [B,T,6] or None, added as given -> imu [B,T,6] = (R^T omega, R^T (a - g e_z)) + bias + noise.  A row with a
    non-finite operand that is read is NaN."""
    par = _row(estimator)
    g = par["gravity"]
    actual, forces = _f64(actual), _f64(forces)
    B, T = actual.shape[:2]
    with np.errstate(all="ignore"):
        fin = np.isfinite(actual[..., 0:3]).all(-1) & np.isfinite(actual[..., 6:9]).all(-1)
        R = plant.quat_to_matrix(plant.rotvec_to_quat(actual[..., 0:3]))
        if base_acc is not None:
            base_acc = _f64(base_acc)
            aw = base_acc[..., 3:6]
            fin &= np.isfinite(base_acc).all(-1)
        else:
            bd = np.broadcast_to(lite3_model._BODY, (B, 7)) if body is None else _f64(body)
            _, okb = plant.inertia_inverse(bd[:, 0], [bd[:, 1 + i] for i in range(6)])
            f = forces.reshape(B, T, 4, 3)
            Fs = (f[:, :, 0] + f[:, :, 1]) + (f[:, :, 2] + f[:, :, 3])
            m = bd[:, 0][:, None]
            aw = np.stack([Fs[..., 0] / m, Fs[..., 1] / m, Fs[..., 2] / m + g], axis=-1)
            fin &= okb[:, None] & np.isfinite(forces).all(-1)
        sp = np.stack([aw[..., 0], aw[..., 1], aw[..., 2] - g], axis=-1)
        out = np.concatenate([_mtv(R, actual[..., 6:9]), _mtv(R, sp)], axis=-1)
        if bias is not None:
            bias = _f64(bias)
            out = out + bias[:, None, :]
            fin &= np.isfinite(bias).all(-1)[:, None]
        if noise is not None:
            noise = _f64(noise)
            out = out + noise
            fin &= np.isfinite(noise).all(-1)
    return np.where(fin[..., None], out, np.nan)


def leg_kinematics(q, qd, R, gyro):
    """Step 1 of the row, shared by the two forms: q, qd [B,4,3], R [B,3,3], gyro [B,3] -> (rho, rhod) [B,4,3], the feet and their
    velocities relative to the CoM in world axes: rho = R p_foot(q), rhod = R (gyro x p_foot(q) + J(q) qd)."""
    (_, _, _), (z0, z1, z2), (p1, p2, p3, pf) = lite3_model._leg_chain(q)
    J = np.stack([np.cross(z0, pf - p1), np.cross(z1, pf - p2), np.cross(z2, pf - p3)], axis=-1)
    jq = _mv(J, qd)
    Rl = R[:, None, :, :]
    return _mv(Rl, pf), _mv(Rl, _cross(gyro[:, None, :], pf) + jq)


def _operands(imu, q, qd, contact_log, init, trust, height, state):
    imu, q, qd, init = _f64(imu), _f64(q), _f64(qd), _f64(init)
    B, T = imu.shape[:2]
    tr = (np.asarray(contact_log) != 0).astype(np.float64) if trust is None else _f64(trust)
    hz = None if height is None else _f64(height)
    st = None if state is None else np.array(state, dtype=np.float64).reshape(B, EST_STATE)
    fresh = np.ones(B, bool) if st is None else st[:, _LIVE] == 0.0
    with np.errstate(all="ignore"):
        q0 = plant.rotvec_to_quat(init[:, 0:3])
    # what is finite before row 0: init where it is read, a live state (P: its upper triangle), height
    ok = np.isfinite(init[:, 0:6]).all(-1) & np.isfinite(init[:, 9:12]).all(-1)
    if st is not None:
        iu = np.triu_indices(6)
        Pu = st[:, _P:_LIVE].reshape(B, 3, 6, 6)[:, :, iu[0], iu[1]].reshape(B, -1)
        live_ok = np.isfinite(st[:, :_P]).all(-1) & np.isfinite(Pu).all(-1) & np.isfinite(st[:, _LIVE])
        ok = np.where(fresh, ok, live_ok)
    if hz is not None:
        ok = ok & np.isfinite(hz).all(-1)
    rows_ok = (np.isfinite(imu).all(-1) & np.isfinite(q).all((-1, -2)) & np.isfinite(qd).all((-1, -2)) & np.isfinite(tr).all(-1))
    return imu, q, qd, init, tr, hz, st, fresh, q0, ok, rows_ok, B, T


def _kappa(par, sf):
    """The tilt correction's gain and direction of a row: (kap [B], s^ [B,3])."""
    sn = np.sqrt((sf[:, 0] * sf[:, 0] + sf[:, 1] * sf[:, 1]) + sf[:, 2] * sf[:, 2])
    ga = abs(par["gravity"])
    pull = sn > 0.0
    sh = np.where(pull[:, None], sf / np.where(pull, sn, 1.0)[:, None], 0.0)
    c0 = 1.0 - np.abs(sn - ga) / ga
    kap = np.where(pull, par["kappa"] * np.where(c0 < 0.0, 0.0, np.where(c0 > 1.0, 1.0, c0)), 0.0)
    return kap, sh


def _update(xi, P, kind, c, z, r):
    """One scalar measurement on an axis: xi [6,B], P [6,6,B] in place; returns e e / S [B]."""
    if kind == 0:
        w = [P[i, c] - P[i, 0] for i in range(6)]
        hw, hx = w[c] - w[0], xi[c] - xi[0]
    else:
        col = 1 if kind == 1 else c
        w = [P[i, col].copy() for i in range(6)]
        hw, hx = w[col], xi[col].copy()
    S, e = hw + r, z - hx
    k = [w[i] / S for i in range(6)]
    for i in range(6):
        xi[i] = xi[i] + k[i] * e
    for i in range(6):
        for j in range(i, 6):
            P[i, j] = P[i, j] - k[i] * w[j]
            P[j, i] = P[i, j]
    return (e * e) / S


def estimate_track_host(imu, q, qd, contact_log, init, trust=None, height=None, state=None, estimator=None, delta=0.03, gate=None,
                        io_dtype=np.float64, attitude=None, att_state=None):
    """The filter over the rows of a log (mpcqp_estimate_track), per axis and measurement by measurement in the device's order: imu
    [B,T,6], q, qd [B,T,4,3], contact_log [B,T,4], init [B,12], trust [B,T,4] or None (contact != 0), height [B,4] or None, state
    [B,131] or None (not modified) -> {"est" [B,T,12], "feet" [B,T,4,3], "sigma" [B,T,6], "nis" [B,T], "state" [B,131]: the predicted
    state for row T, live = 1, to be passed to the next piece}.  A robot with a non-finite operand is NaN from that row on and its
    returned state is NaN.
    gate: None, or a dict of `gate_row`'s fields ({} = the defaults) for mpcqp_estimate_track_gated (include/mpcqp_gate.h): every row's
    trust is gated on the legs' velocity innovations before the row's updates, w is rounded through `io_dtype` (the handle's I/O type:
    with it this is the counterpart of either handle), and the result has "trust" [B,T,4] = w and "gate_d" [B,T,4] = d.
    attitude: None, or a dict of `attitude_row`'s fields ({} = the defaults) for mpcqp_estimate_track_aided (include/mpcqp_attitude.h,
    which has the rule), with att_state [B,8] or None (not modified; read where `state` is live): the rows use g' = gyro - b^, the
    velocity update's correction steers the orientation and b^, and the result has "gyro_bias" [B,T,3] = b^ as each row found it and
    "att_state" [B,8], to be passed to the next piece with "state"."""
    par = _row(estimator)
    gpar = None if gate is None else gate_row(**gate)
    apar = None if attitude is None else attitude_row(**attitude)
    if apar is None and att_state is not None:
        raise ValueError("att_state needs attitude")
    imu, q, qd, init, tr, hz, st, fresh, q0, ok, rows_ok, B, T = _operands(imu, q, qd, contact_log, init, trust, height, state)
    if apar is not None:
        bh, bok = _att_operands(att_state, fresh, B)
        ok = ok & bok
        eb, blog = np.zeros((B, 3)), np.zeros((B, T, 3))
        dg, kbd = float(delta) * abs(par["gravity"]), apar["k_b"] * float(delta)
    d, hd2, g = float(delta), 0.5 * float(delta) * float(delta), par["gravity"]
    est, feet, sigma, nis = np.zeros((B, T, 12)), np.zeros((B, T, 4, 3)), np.zeros((B, T, 6)), np.zeros((B, T))
    wlog, dlog = np.zeros((B, T, 4)), np.zeros((B, T, 4))
    with np.errstate(all="ignore"):
        qh = q0 if st is None else np.where(fresh[:, None], q0, st[:, 0:4])
        xi, P = np.zeros((3, 6, B)), np.zeros((3, 6, 6, B))
        for a in range(3):
            xi[a, 0], xi[a, 1] = init[:, 3 + a], init[:, 9 + a]
            for i in range(6):
                P[a, i, i] = par["p0_p"] if i == 0 else (par["p0_v"] if i == 1 else par["p0_f"])
            if st is not None:
                sx, sp = st[:, _XI + 6 * a:_XI + 6 * a + 6], st[:, _P + 36 * a:_P + 36 * a + 36].reshape(B, 6, 6)
                xi[a] = np.where(fresh, xi[a], sx.T)
                for i in range(6):
                    for j in range(i, 6):
                        P[a, i, j] = np.where(fresh, P[a, i, j], sp[:, i, j])
                        P[a, j, i] = P[a, i, j]
        for t in range(T):
            ok = ok & rows_ok[:, t]
            gy, sf = imu[:, t, 0:3], imu[:, t, 3:6]
            R = plant.quat_to_matrix(qh)
            if apar is not None:
                blog[:, t] = bh
                gy = gy - bh
            rho, rhod = leg_kinematics(q[:, t], qd[:, t], R, gy)
            if t == 0:
                for a in range(3):
                    for l in range(4):
                        xi[a, 2 + l] = np.where(fresh, xi[a, 0] + rho[:, l, a], xi[a, 2 + l])
            vpred = xi[0:2, 1].copy()
            w = tr[:, t]
            if gpar is not None:
                w, dlog[:, t] = trust_gate(gpar, par, xi, P, rhod, w, io_dtype)
                wlog[:, t] = w
            s = [1.0 + (1.0 - w[:, l]) * par["k_swing"] for l in range(4)]
            na = []
            for a in range(3):
                n = np.zeros(B)
                for l in range(4):
                    n = n + _update(xi[a], P[a], 0, 2 + l, rho[:, l, a], par["r_p"] * s[l])
                    n = n + _update(xi[a], P[a], 1, 2 + l, -rhod[:, l, a], par["r_v"] * s[l])
                    if a == 2 and hz is not None:
                        n = n + _update(xi[a], P[a], 2, 2 + l, hz[:, l], par["r_z"] * s[l])
                na.append(n)
            if apar is not None:
                dv = xi[0:2, 1] - vpred
                eb = _mtv(R, np.stack([(-dv[1]) / dg, dv[0] / dg, np.zeros(B)], axis=-1))
            est[:, t, 0:3] = plant.quat_to_rotvec(qh)
            est[:, t, 6:9] = _mv(R, gy)
            for a in range(3):
                est[:, t, 3 + a], est[:, t, 9 + a] = xi[a, 0], xi[a, 1]
                feet[:, t, :, a] = xi[a, 2:6].T
                sigma[:, t, a], sigma[:, t, 3 + a] = np.sqrt(P[a, 0, 0]), np.sqrt(P[a, 1, 1])
            nis[:, t] = (na[0] + na[1]) + na[2]
            bad = ~ok
            est[bad, t], feet[bad, t], sigma[bad, t], nis[bad, t], wlog[bad, t] = np.nan, np.nan, np.nan, np.nan, np.nan
            if apar is not None:
                blog[bad, t] = np.nan
            # predict
            for a in range(3):
                aw = (R[:, a, 0] * sf[:, 0] + R[:, a, 1] * sf[:, 1]) + R[:, a, 2] * sf[:, 2]
                if a == 2:
                    aw = aw + g
                xi[a, 0] = (xi[a, 0] + d * xi[a, 1]) + hd2 * aw
                xi[a, 1] = xi[a, 1] + d * aw
                Pa = P[a]
                Pa[0, 0] = (Pa[0, 0] + d * Pa[0, 1]) + d * (Pa[0, 1] + d * Pa[1, 1])
                for j in range(1, 6):
                    Pa[0, j] = Pa[0, j] + d * Pa[1, j]
                    Pa[j, 0] = Pa[0, j]
                Pa[0, 0] = Pa[0, 0] + d * par["q_p"]
                Pa[1, 1] = Pa[1, 1] + d * par["q_v"]
                for l in range(4):
                    Pa[2 + l, 2 + l] = Pa[2 + l, 2 + l] + d * (par["q_f"] * s[l])
            kap, sh = _kappa(par, sf)
            if apar is None:
                wh = _mv(R, gy + kap[:, None] * _cross(sh, R[:, 2, :]))
            else:
                wh = _mv(R, (gy + (apar["k_s"] * kap)[:, None] * _cross(sh, R[:, 2, :])) + apar["k_v"] * eb)
                nb = bh - kbd * eb
                bh = np.where(nb < -apar["b_max"], -apar["b_max"], np.where(nb > apar["b_max"], apar["b_max"], nb))
            n = quat_mul(plant.rotvec_to_quat(d * wh), qh)
            nq = np.sqrt(((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) + n[:, 3] * n[:, 3])
            qh = n / nq[:, None]
    out_state = np.empty((B, EST_STATE))
    out_state[:, 0:4] = qh
    for a in range(3):
        out_state[:, _XI + 6 * a:_XI + 6 * a + 6] = xi[a].T
        out_state[:, _P + 36 * a:_P + 36 * a + 36] = P[a].transpose(2, 0, 1).reshape(B, 36)
    out_state[:, _LIVE] = 1.0
    out_state[~ok] = np.nan
    res = {"est": est, "feet": feet, "sigma": sigma, "nis": nis, "state": out_state}
    if apar is not None:
        res.update(gyro_bias=blog, att_state=_att_state(bh, eb, ok))
    return res if gpar is None else dict(res, trust=wlog, gate_d=dlog)


def estimate_joint_host(imu, q, qd, contact_log, init, trust=None, height=None, state=None, estimator=None, delta=0.03, attitude=None,
                        att_state=None):
    """`estimate_track_host` in the textbook form: one filter with the 18 states (p, v, c_FL, c_FR, c_HL, c_HR), every measurement of a
    row in one batch update -- K = P H^T S^-1 by np.linalg.solve, P = (I - K H) P, nis = e^T S^-1 e -- and the orientation through
    scipy's Rotation.  Operands and results as there (the state's layout too); only `leg_kinematics`, the operand check and the tilt
    gain are shared.  attitude / att_state as there (include/mpcqp_attitude.h): dv is read off the batch update's state step, e_b, the
    rate and b^ are formed with numpy's matrix products, cross and clip, and the result has "gyro_bias" and "att_state"."""
    from scipy.spatial.transform import Rotation
    par = _row(estimator)
    apar = None if attitude is None else attitude_row(**attitude)
    if apar is None and att_state is not None:
        raise ValueError("att_state needs attitude")
    imu, q, qd, init, tr, hz, st, fresh, q0, ok, rows_ok, B, T = _operands(imu, q, qd, contact_log, init, trust, height, state)
    if apar is not None:
        bh, bok = _att_operands(att_state, fresh, B)
        ok = ok & bok
        bh, eb, blog = np.nan_to_num(bh), np.zeros((B, 3)), np.zeros((B, T, 3))
    d, g = float(delta), par["gravity"]
    est, feet, sigma, nis = np.zeros((B, T, 12)), np.zeros((B, T, 4, 3)), np.zeros((B, T, 6)), np.zeros((B, T))
    nz = np.nan_to_num                      # (a poisoned robot is masked by `ok`; its rows are computed on zeros)
    init, st = nz(init), None if st is None else nz(st)
    idx = lambda k, a: 3 * k + a            # state index of entry k (0 p, 1 v, 2 + l foot) along axis a
    with np.errstate(all="ignore"):
        qh = q0 if st is None else np.where(fresh[:, None], q0, st[:, 0:4])
        x, P = np.zeros((B, 18)), np.zeros((B, 18, 18))
        for a in range(3):
            x[:, idx(0, a)], x[:, idx(1, a)] = init[:, 3 + a], init[:, 9 + a]
            for k in range(6):
                P[:, idx(k, a), idx(k, a)] = par["p0_p"] if k == 0 else (par["p0_v"] if k == 1 else par["p0_f"])
        if st is not None:
            for a in range(3):
                sp = st[:, _P + 36 * a:_P + 36 * a + 36].reshape(B, 6, 6)
                sp = np.triu(sp) + np.transpose(np.triu(sp, 1), (0, 2, 1))
                for k in range(6):
                    x[:, idx(k, a)] = np.where(fresh, x[:, idx(k, a)], st[:, _XI + 6 * a + k])
                    for j in range(6):
                        P[:, idx(k, a), idx(j, a)] = np.where(fresh, P[:, idx(k, a), idx(j, a)], sp[:, k, j])
        A = np.eye(18)
        for a in range(3):
            A[idx(0, a), idx(1, a)] = d
        # measurement rows: per leg 3 relative positions, 3 relative velocities, then the heights
        M = 24 + (4 if hz is not None else 0)
        H = np.zeros((M, 18))
        for l in range(4):
            for a in range(3):
                H[6 * l + a, idx(2 + l, a)], H[6 * l + a, idx(0, a)] = 1.0, -1.0
                H[6 * l + 3 + a, idx(1, a)] = 1.0
            if hz is not None:
                H[24 + l, idx(2 + l, 2)] = 1.0
        for t in range(T):
            ok = ok & rows_ok[:, t]
            gy, sf = nz(imu[:, t, 0:3]), nz(imu[:, t, 3:6])
            rot = Rotation.from_quat(nz(qh)[:, [1, 2, 3, 0]] + np.where(np.isfinite(qh).all(-1), 0.0, 1.0)[:, None] * np.array([0, 0, 0, 1.0]))
            R = rot.as_matrix()
            if apar is not None:
                blog[:, t] = bh
                gy = gy - bh
            rho, rhod = leg_kinematics(nz(q[:, t]), nz(qd[:, t]), R, gy)
            if t == 0:
                for l in range(4):
                    for a in range(3):
                        x[:, idx(2 + l, a)] = np.where(fresh, x[:, idx(0, a)] + rho[:, l, a], x[:, idx(2 + l, a)])
            s = np.stack([1.0 + (1.0 - nz(tr[:, t, l])) * par["k_swing"] for l in range(4)], axis=-1)      # [B,4]
            z, rv = np.zeros((B, M)), np.zeros((B, M))
            for l in range(4):
                z[:, 6 * l:6 * l + 3], z[:, 6 * l + 3:6 * l + 6] = rho[:, l], -rhod[:, l]
                rv[:, 6 * l:6 * l + 3], rv[:, 6 * l + 3:6 * l + 6] = par["r_p"] * s[:, l, None], par["r_v"] * s[:, l, None]
                if hz is not None:
                    z[:, 24 + l], rv[:, 24 + l] = nz(hz[:, l]), par["r_z"] * s[:, l]
            e = z - x @ H.T
            PHt = P @ H.T
            S = H @ PHt + rv[:, :, None] * np.eye(M)
            K = np.transpose(np.linalg.solve(S, np.transpose(PHt, (0, 2, 1))), (0, 2, 1))       # (S symmetric)
            nis[:, t] = np.einsum("bi,bi->b", e, np.linalg.solve(S, e[:, :, None])[:, :, 0])
            step = np.einsum("bij,bj->bi", K, e)
            x = x + step
            if apar is not None:        # dv = what the update did to v_x and v_y
                ew = np.stack([-step[:, idx(1, 1)], step[:, idx(1, 0)], np.zeros(B)], axis=-1) / (d * abs(g))
                eb = np.einsum("bji,bj->bi", R, ew)
            P = P - K @ (H @ P)
            P = 0.5 * (P + np.transpose(P, (0, 2, 1)))
            est[:, t, 0:3], est[:, t, 6:9] = rot.as_rotvec(), np.einsum("bij,bj->bi", R, gy)
            for a in range(3):
                est[:, t, 3 + a], est[:, t, 9 + a] = x[:, idx(0, a)], x[:, idx(1, a)]
                sigma[:, t, a], sigma[:, t, 3 + a] = np.sqrt(P[:, idx(0, a), idx(0, a)]), np.sqrt(P[:, idx(1, a), idx(1, a)])
                for l in range(4):
                    feet[:, t, l, a] = x[:, idx(2 + l, a)]
            bad = ~ok
            est[bad, t], feet[bad, t], sigma[bad, t], nis[bad, t] = np.nan, np.nan, np.nan, np.nan
            if apar is not None:
                blog[bad, t] = np.nan
            # predict
            aw = np.einsum("bij,bj->bi", R, sf) + np.array([0.0, 0.0, g])
            Bu = np.zeros((B, 18))
            Bu[:, 0:3], Bu[:, 3:6] = 0.5 * d * d * aw, d * aw
            x = x @ A.T + Bu
            Q = np.zeros((B, 18))
            Q[:, 0:3], Q[:, 3:6] = par["q_p"], par["q_v"]
            for l in range(4):
                Q[:, 6 + 3 * l:9 + 3 * l] = par["q_f"] * s[:, l, None]
            P = A @ P @ A.T + d * Q[:, :, None] * np.eye(18)
            kap, sh = _kappa(par, sf)
            if apar is None:
                wb = gy + kap[:, None] * np.cross(sh, R[:, 2, :])
            else:
                wb = gy + apar["k_s"] * kap[:, None] * np.cross(sh, R[:, 2, :]) + apar["k_v"] * eb
                bh = np.clip(bh - apar["k_b"] * d * eb, -apar["b_max"], apar["b_max"])
            rot = Rotation.from_rotvec(d * np.einsum("bij,bj->bi", R, wb)) * rot
            qh = rot.as_quat()[:, [3, 0, 1, 2]]
    out_state = np.empty((B, EST_STATE))
    out_state[:, 0:4] = qh
    for a in range(3):
        for k in range(6):
            out_state[:, _XI + 6 * a + k] = x[:, idx(k, a)]
            for j in range(6):
                out_state[:, _P + 36 * a + 6 * k + j] = P[:, idx(k, a), idx(j, a)]
    out_state[:, _LIVE] = 1.0
    out_state[~ok] = np.nan
    res = {"est": est, "feet": feet, "sigma": sigma, "nis": nis, "state": out_state}
    return res if apar is None else dict(res, gyro_bias=blog, att_state=_att_state(bh, eb, ok))
