"""Host checker of the rigid-body plant (include/mpcqp_sim.h): numpy fp64, vectorised over robots.

``srb_step`` is one control period of the plant for B robots -- the same equations, in the same operation order and with the
same rotation-vector / quaternion conversions as the device (csrc/mpcqp_plant.h), so that the two agree to rounding.
``rollout_plant_host`` is the closed loop of ``mpcqp_rollout_plant`` on the CPU checker: per tick the checker's own roll-out of
one tick supplies the solve, the log rows, the reference roll-forward and the tick advance, and ``srb_step`` replaces its world
step.  Conventions (state, body rows, wrench rows) are the header's.
"""
from __future__ import annotations

import numpy as np

DEFAULT_SUBSTEPS, MAX_SUBSTEPS = 10, 1000
SERIES_ANGLE = 1e-3          # below this angle the conversions use their series (exact in the limit 0)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def rotvec_to_quat(theta):
    """Rotation vectors [..., 3] -> unit quaternions [..., 4] = (w, x, y, z) with w >= 0 for |theta| <= pi."""
    t = _f64(theta)
    t0, t1, t2 = t[..., 0], t[..., 1], t[..., 2]
    a = np.sqrt((t0 * t0 + t1 * t1) + t2 * t2)
    a2 = a * a
    with np.errstate(divide="ignore", invalid="ignore"):
        big = np.sin(0.5 * a) / a
    s = np.where(a <= SERIES_ANGLE, (0.5 - a2 / 48.0) + (a2 * a2) / 3840.0, big)
    return np.stack([np.cos(0.5 * a), s * t0, s * t1, s * t2], axis=-1)


def quat_to_rotvec(q):
    """Quaternions [..., 4] = (w, x, y, z) -> rotation vectors [..., 3] with |theta| <= pi (the sign with w >= 0 is taken)."""
    q = _f64(q)
    sg = np.where(q[..., 0] < 0.0, -1.0, 1.0)
    w, x, y, z = sg * q[..., 0], sg * q[..., 1], sg * q[..., 2], sg * q[..., 3]
    nv = np.sqrt((x * x + y * y) + z * z)
    a = 2.0 * np.arctan2(nv, w)
    a2 = a * a
    with np.errstate(divide="ignore", invalid="ignore"):
        big = a / np.sin(0.5 * a)
    sc = np.where(a <= SERIES_ANGLE, (2.0 + a2 / 12.0) + 7.0 * (a2 * a2) / 2880.0, big)
    return np.stack([sc * x, sc * y, sc * z], axis=-1)


def quat_to_matrix(q):
    """(w, x, y, z) [..., 4] -> rotation matrices [..., 3, 3] (the formula of the derivative, for a unit q)."""
    q = _f64(q)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
         2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]
    return np.stack(R, axis=-1).reshape(q.shape[:-1] + (3, 3))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _symv(S, v):   # S = (xx, yy, zz, xy, xz, yz)
    return [(S[0] * v[0] + S[3] * v[1]) + S[4] * v[2],
            (S[3] * v[0] + S[1] * v[1]) + S[5] * v[2],
            (S[4] * v[0] + S[5] * v[1]) + S[2] * v[2]]


def inertia_inverse(m, I):
    """Cofactor inverse of the torso-frame inertia (I = xx, yy, zz, xy, xz, yz; each [B]) and the row validity of the header:
    finite entries, m > 0 and positive definite by Sylvester's criterion."""
    xx, yy, zz, xy, xz, yz = I
    with np.errstate(invalid="ignore", over="ignore"):
        c00, c01, c02 = yy * zz - yz * yz, xz * yz - xy * zz, xy * yz - xz * yy
        c11, c12, c22 = xx * zz - xz * xz, xy * xz - xx * yz, xx * yy - xy * xy
        det = (xx * c00 + xy * c01) + xz * c02
        ok = np.isfinite(m) & (m > 0.0) & (xx > 0.0) & (c22 > 0.0) & (det > 0.0) & np.isfinite(det)
    for v in I:
        ok = ok & np.isfinite(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        Ii = [c00 / det, c11 / det, c22 / det, c01 / det, c02 / det, c12 / det]
    return Ii, ok


def _deriv(y, acc, M0, Ff, Ib, Ii):
    """y = [q (4), p (3), omega (3), v (3)], a list of [B] arrays -> dy/dt (csrc/mpcqp_plant.h, plant_deriv)."""
    w, qx, qy, qz = y[0], y[1], y[2], y[3]
    R = [1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - w * qz), 2.0 * (qx * qz + w * qy),
         2.0 * (qx * qy + w * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - w * qx),
         2.0 * (qx * qz - w * qy), 2.0 * (qy * qz + w * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]
    p, om = y[4:7], y[7:10]
    pf = _cross(p, Ff)
    tau = [M0[i] - pf[i] for i in range(3)]                                   # sum (foot_l - p) x f_l + tau_push
    wb = [(R[i] * om[0] + R[3 + i] * om[1]) + R[6 + i] * om[2] for i in range(3)]
    tb = [(R[i] * tau[0] + R[3 + i] * tau[1]) + R[6 + i] * tau[2] for i in range(3)]
    L = _symv(Ib, wb)
    gy = _cross(wb, L)
    r = [tb[i] - gy[i] for i in range(3)]
    e = _symv(Ii, r)
    d = [0.5 * (-((om[0] * qx + om[1] * qy) + om[2] * qz)),
         0.5 * (w * om[0] + (om[1] * qz - om[2] * qy)),
         0.5 * (w * om[1] + (om[2] * qx - om[0] * qz)),
         0.5 * (w * om[2] + (om[0] * qy - om[1] * qx))]
    d += [y[10 + i] for i in range(3)]
    d += [(R[3 * i] * e[0] + R[3 * i + 1] * e[1]) + R[3 * i + 2] * e[2] for i in range(3)]
    d += [acc[i] for i in range(3)]
    return d


def model_body(m, Ibody_inv, B=1):
    """Body rows [B,7] of the MPC's model (MpcQpConfig.m, diag(1 / Ibody_inv)): what body = None means."""
    Ii = _f64(Ibody_inv)
    row = np.array([float(m), 1.0 / Ii[0], 1.0 / Ii[1], 1.0 / Ii[2], 0.0, 0.0, 0.0])
    return np.tile(row, (B, 1))


def srb_step(x, f, feet, contact, body, wrench=None, delta=0.03, substeps=DEFAULT_SUBSTEPS):
    """One control period of the plant for B robots (include/mpcqp_sim.h, mpcqp_plant_step), fp64.
    x [B,13], f [B,12], feet [B,4,3], contact [B,4] (nonzero = stance), body [B,7] (m, Ixx, Iyy, Izz, Ixy, Ixz, Iyz; use
    ``model_body`` for the model's), wrench [B,6] or None, substeps 0 = 10.  Returns x_out [B,13]; invalid body rows give NaN in
    x_out[:, :12]."""
    substeps = int(substeps)
    if substeps < 0 or substeps > MAX_SUBSTEPS:
        raise ValueError(f"substeps must be in [0, {MAX_SUBSTEPS}], got {substeps}")
    n = substeps or DEFAULT_SUBSTEPS
    x = _f64(x).reshape(-1, 13)
    B = x.shape[0]
    f = _f64(f).reshape(B, 12); feet = _f64(feet).reshape(B, 12)
    st = np.asarray(contact).reshape(B, 4) != 0
    body = _f64(body).reshape(B, 7)
    wr = np.zeros((B, 6)) if wrench is None else _f64(wrench).reshape(B, 6)
    m, g = body[:, 0], x[:, 12]
    Ib = [body[:, 1 + i] for i in range(6)]
    Ii, ok = inertia_inverse(m, Ib)
    zero = np.zeros(B)
    Ff, M0 = [zero] * 3, [zero] * 3
    for l in range(4):   # a swing leg's force and foot are ignored
        fl = [np.where(st[:, l], f[:, 3 * l + a], 0.0) for a in range(3)]
        rl = [np.where(st[:, l], feet[:, 3 * l + a], 0.0) for a in range(3)]
        cr = _cross(rl, fl)
        Ff = [Ff[a] + fl[a] for a in range(3)]
        M0 = [M0[a] + cr[a] for a in range(3)]
    M0 = [M0[a] + wr[:, 3 + a] for a in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = [(Ff[a] + wr[:, a]) / m for a in range(3)]
    acc[2] = acc[2] + g
    q = rotvec_to_quat(x[:, 0:3])
    y = [q[:, i] for i in range(4)] + [x[:, 3 + i] for i in range(9)]
    h = float(delta) / n
    hh, h6 = 0.5 * h, h / 6.0
    with np.errstate(all="ignore"):
        for _ in range(n):   # classical RK4: s = ((k1 + 2 k2) + 2 k3) + k4, y += h / 6 s
            k = _deriv(y, acc, M0, Ff, Ib, Ii)
            s = list(k); t = [y[i] + hh * k[i] for i in range(13)]
            k = _deriv(t, acc, M0, Ff, Ib, Ii)
            s = [s[i] + 2.0 * k[i] for i in range(13)]; t = [y[i] + hh * k[i] for i in range(13)]
            k = _deriv(t, acc, M0, Ff, Ib, Ii)
            s = [s[i] + 2.0 * k[i] for i in range(13)]; t = [y[i] + h * k[i] for i in range(13)]
            k = _deriv(t, acc, M0, Ff, Ib, Ii)
            y = [y[i] + h6 * (s[i] + k[i]) for i in range(13)]
            nq = np.sqrt(((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]) + y[3] * y[3])
            y = [y[i] / nq for i in range(4)] + y[4:]
        out = np.empty((B, 13))
        out[:, 0:3] = quat_to_rotvec(np.stack(y[0:4], axis=-1))
    for i in range(9):
        out[:, 3 + i] = y[4 + i]
    out[:, 12] = g
    out[~ok, :12] = np.nan
    return out


def stance_feet(plan_pos, plan_feet_id, plan_meta, tick):
    """Feet and contact of each robot's current tick, by the roll-out's stage-0 rule (include/mpcqp_sim.h): the step
    min(t / (ss + ds), S_b - 1) of t = max(tick, 0) (plan_meta clamped as in mpcqp_rollout), stance = feet_id during the step's
    first ss ticks, else all stance.  Returns (feet [B,4,3], contact uint8 [B,4])."""
    pos = _f64(plan_pos); fid = np.asarray(plan_feet_id); meta = np.asarray(plan_meta).astype(np.int64)
    B, Smax = pos.shape[0], pos.shape[1]
    S = np.minimum(np.maximum(meta[:, 0], 1), Smax)
    ss = np.maximum(meta[:, 1], 0)
    period = np.maximum(ss + np.maximum(meta[:, 2], 0), 1)
    t0 = np.maximum(np.asarray(tick).astype(np.int64), 0)
    step = np.minimum(t0 // period, S - 1)
    tin = t0 - step * period
    rows = np.arange(B)
    feet = pos[rows, step]
    contact = np.where((tin < ss)[:, None], fid[rows, step] != 0, True).astype(np.uint8)
    return feet, contact


def push_wrench(push, push_ticks, tick):
    """The wrench of each robot at its own tick: push[b] on push_ticks[b][0] <= tick[b] < push_ticks[b][1], else zero."""
    push = _f64(push); pt = np.asarray(push_ticks).astype(np.int64); tk = np.asarray(tick).astype(np.int64)
    on = (pt[:, 0] <= tk) & (tk < pt[:, 1])
    return np.where(on[:, None], push, 0.0)


def _plan_clock(plan_pos, plan_meta, tick):
    """The clamped plan row of mpcqp_rollout (include/mpcqp.h): S_b in [1, S], ss >= 0, ss + ds >= 1, t0 = max(tick, 0), and the
    gate on the reference velocities, 0 on the plan's last step.  Each [B]."""
    meta = np.asarray(plan_meta).astype(np.int64)
    S = np.minimum(np.maximum(meta[:, 0], 1), np.shape(plan_pos)[1])
    ss = np.maximum(meta[:, 1], 0)
    period = np.maximum(ss + np.maximum(meta[:, 2], 0), 1)
    t0 = np.maximum(np.asarray(tick).astype(np.int64), 0)
    gate = np.where(np.minimum(t0 // period, S - 1) == S - 1, 0.0, 1.0)
    return S, ss, period, t0, gate


def plan_expand_host(x, ref, plan_pos, plan_feet_id, plan_meta, tick, N, delta):
    """The operator tuple of one tick of mpcqp_rollout (include/mpcqp.h), numpy fp64 in the checker's operation order: stage k lies in
    step min((t0 + k) / (ss + ds), S_b - 1) of the clamped plan row (``stance_feet``'s arithmetic), every foot stands on the plan,
    and the reference velocities are gated off on the plan's last step.  Returns {"r" [B,N,4,3], "contact" [B,N,4], "xdes" [B,N+1,13]}."""
    x, ref, pos = _f64(x), _f64(ref), _f64(plan_pos)
    fid = np.asarray(plan_feet_id)
    B, N, d = x.shape[0], int(N), float(delta)
    S, ss, period, t0, gate = _plan_clock(pos, plan_meta, tick)
    kd = (np.arange(N + 1) * d)[None, :] * gate[:, None]                                          # (k delta) gate, [B,N+1]
    xdes = np.zeros((B, N + 1, 13))
    xdes[:, :, 0], xdes[:, :, 1] = ref[:, None, 0], ref[:, None, 1]
    xdes[:, :, 2] = ref[:, None, 2] + kd * ref[:, None, 9]
    xdes[:, :, 3:6] = ref[:, None, 3:6] + kd[:, :, None] * ref[:, None, 6:9]
    xdes[:, :, 8] = (gate * ref[:, 9])[:, None]
    xdes[:, :, 9:12] = (gate[:, None] * ref[:, 6:9])[:, None, :]
    xdes[:, :, 12] = x[:, None, 12]
    tau = t0[:, None] + np.arange(N)[None, :]
    st = np.minimum(tau // period[:, None], (S - 1)[:, None])
    tin = tau - st * period[:, None]
    rows = np.arange(B)[:, None]
    contact = np.where((tin < ss[:, None])[:, :, None], fid[rows, st] != 0, True).astype(np.uint8)
    com = xdes[:, :N, 3:6].copy()
    com[:, 0] = x[:, 3:6]
    return {"r": pos[rows, st] - com[:, :, None, :], "contact": contact, "xdes": xdes}


def rollout_loop_host(engine, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T):
    """mpcqp_rollout tick by tick in Python, on any object with `cfg` and `solve_batch_host` (a checker ``Engine``, or a
    ``disturbance.DisturbedEngine`` -- whose table the checker's C loop cannot see).  Per tick: ``plan_expand_host``, one
    ``solve_batch_host`` with want_X, the log rows, x[:, :12] <- X[:, 1, :12], the reference rolled forward, the tick advanced.
    Without a table it reproduces ``Engine.rollout_host``, and it returns what that returns."""
    cfg = engine.cfg
    N, d = int(cfg.N), float(cfg.delta)
    x = _f64(x).copy(); ref = _f64(ref).copy(); mu = _f64(mu)
    tick = np.asarray(tick, dtype=np.int32).copy()
    B, T = x.shape[0], int(T)
    actual = np.zeros((B, T, 12)); desired = np.zeros((B, T, 12)); forces = np.zeros((B, T, 12)); solved = np.zeros(B, np.int32)
    for t in range(T if B else 0):
        gate = _plan_clock(plan_pos, plan_meta, tick)[4]
        e = plan_expand_host(x, ref, plan_pos, plan_feet_id, plan_meta, tick, N, d)
        o = engine.solve_batch_host(x, e["r"], e["contact"], e["xdes"], mu, want_X=True)
        actual[:, t] = x[:, :12]
        desired[:, t, 0:6] = ref[:, 0:6]
        desired[:, t, 8] = gate * ref[:, 9]
        desired[:, t, 9:12] = gate[:, None] * ref[:, 6:9]
        forces[:, t] = np.asarray(o["u"], np.float64).reshape(B, N, 12)[:, 0]
        solved += np.isin(o["status"], (1, 2)).astype(np.int32)
        x[:, :12] = np.asarray(o["X"], np.float64).reshape(B, N + 1, 13)[:, 1, :12]
        ref[:, 3:6] += (gate[:, None] * ref[:, 6:9]) * d
        ref[:, 2] += (gate * ref[:, 9]) * d
        tick += 1
    return {"x": x, "ref": ref, "tick": tick, "actual": actual, "desired": desired, "forces": forces, "solved": solved}


def rollout_plant_host(oracle_engine, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T, body=None, push=None, push_ticks=None,
                       substeps=DEFAULT_SUBSTEPS):
    """Closed loop of mpcqp_rollout_plant on the CPU checker (host memory, fp64).  Per tick: the checker's roll-out of one tick
    (solve, log rows, ref roll-forward, tick advance) with its world step discarded, then ``srb_step`` under the stage-0 forces it
    logged.  `oracle_engine` is a checker ``Engine`` or a ``disturbance.DisturbedEngine``, whose ``rollout_host`` makes that tick's solve
    under its table.  Returns the advanced (x, ref, tick) and the logs, as ``Engine.rollout_host``."""
    if push is not None and push_ticks is None:
        raise ValueError("push needs push_ticks")
    cfg = oracle_engine.cfg
    x = _f64(x).copy(); ref = _f64(ref).copy(); tick = np.asarray(tick, dtype=np.int32).copy()
    B = x.shape[0]
    body = model_body(cfg.m, list(cfg.Ibody_inv), B) if body is None else _f64(body)
    actual = np.zeros((B, T, 12)); desired = np.zeros((B, T, 12)); forces = np.zeros((B, T, 12)); solved = np.zeros(B, np.int32)
    for t in range(T):
        feet, contact = stance_feet(plan_pos, plan_feet_id, plan_meta, tick)
        wr = None if push is None else push_wrench(push, push_ticks, tick)
        o = oracle_engine.rollout_host(x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, 1)
        actual[:, t], desired[:, t], forces[:, t] = o["actual"][:, 0], o["desired"][:, 0], o["forces"][:, 0]
        solved += o["solved"]
        x = srb_step(x, o["forces"][:, 0], feet, contact, body, wr, cfg.delta, substeps)
        ref, tick = o["ref"], o["tick"]
    return {"x": x, "ref": ref, "tick": tick, "actual": actual, "desired": desired, "forces": forces, "solved": solved}
