"""Host counterpart of the per-leg periodic gaits (include/mpcqp_plan.h: mpcqp_phase_expand, mpcqp_solve_batch_phase,
mpcqp_phase_swing; include/mpcqp_sim.h: mpcqp_rollout_phase, mpcqp_rollout_legs): numpy fp64, vectorised over robots, in the device's operation order
(csrc/mpcqp_gaits.h) so that the two agree to rounding.

The clock.  A gait row is ``(P, offset[4], stance[4])`` in ticks, legs FL, FR, HL, HR.  Leg l is in stance at tick t >= 0 when
``phi_l(t) = (t + offset_l) mod P < stance_l`` (the convention of ``synth.perleg_contact``) and touches down at t exactly when
``0 < stance_l < P`` and ``phi_l(t) = 0``.  Rows are clamped as the device clamps them: P into [1, 65535], offset reduced into
[0, P), stance into [0, P], negative ticks to 0.

The rule.  ``p_xy = c_xy + Rz(psi) stand_xy + (Ts / 2) v_ref_xy + gain (v_xy - v_ref_xy)``, ``p_z = stand_z`` with
``Ts = stance_l * delta``: the nominal foot under the hip, half a stance of travel ahead, moved by the velocity error.

Named rows (``gait_rows``).  Each is (touchdown time of FL, FR, HL, HR as a fraction of the period, duty factor); leg l lands at
ticks t = round(touchdown_l P) (mod P) and stays down for round(duty P) ticks, at least 1 and at most P - 1.  The fractions are
this project's choice of a plain representative of each gait, not a measurement of an animal or of the Cheetah 3:

    trot         diagonal pairs (FL+HR, FR+HL) half a period apart, duty 0.6: the pairs overlap, there is always support
    flying_trot  the same pairs, duty 0.4: a flight phase of a tenth of the period between the pairs
    pace         lateral pairs (FL+HL, FR+HR), duty 0.6
    bound        front pair and hind pair half a period apart, duty 0.5
    pronk        all four together, duty 0.5: half of the period is flight
    gallop       transverse: FL 0, FR 0.1, HL 0.5, HR 0.6, duty 0.3: a flight phase of a tenth of the period after each pair
    walk         four beats a quarter apart in lateral sequence (FL 0, HR 0.25, FR 0.5, HL 0.75), duty 0.75: one leg swings at a time
    stand        stance = P: no leg ever lifts
"""
from __future__ import annotations

import numpy as np

from .plant import DEFAULT_SUBSTEPS, model_body, push_wrench, rotvec_to_quat, srb_step

MAX_PERIOD = 65535

# name: ((touchdown fraction of FL, FR, HL, HR), duty factor); duty None = never lifts
GAITS = {
    "trot": ((0.0, 0.5, 0.5, 0.0), 0.6),
    "flying_trot": ((0.0, 0.5, 0.5, 0.0), 0.4),
    "pace": ((0.0, 0.5, 0.0, 0.5), 0.6),
    "bound": ((0.0, 0.0, 0.5, 0.5), 0.5),
    "pronk": ((0.0, 0.0, 0.0, 0.0), 0.5),
    "gallop": ((0.0, 0.1, 0.5, 0.6), 0.3),
    "walk": ((0.0, 0.5, 0.75, 0.25), 0.75),
    "stand": ((0.0, 0.0, 0.0, 0.0), None),
}


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def gait_rows(names, period):
    """int32 [B,9] gait rows of the named gaits (GAITS) at `period` ticks (a scalar or one per name)."""
    names = [names] if isinstance(names, str) else list(names)
    P = np.broadcast_to(np.asarray(period, dtype=np.int64), (len(names),))
    rows = np.zeros((len(names), 9), np.int32)
    for i, name in enumerate(names):
        land, duty = GAITS[name]
        p = int(P[i])
        if not 1 <= p <= MAX_PERIOD:
            raise ValueError(f"period must be in [1, {MAX_PERIOD}], got {p}")
        rows[i, 0] = p
        for l in range(4):   # landing at tick t0 means phi(t0) = 0: offset = -t0 mod P
            rows[i, 1 + l] = (-int(np.floor(land[l] * p + 0.5))) % p
            rows[i, 5 + l] = p if duty is None else min(max(int(np.floor(duty * p + 0.5)), 1), max(p - 1, 1))
    return rows


def clamp_gait(gait):
    """The clamped row of the device (csrc/mpcqp_gaits.h, gait_leg): (P [B], offset [B,4], stance [B,4]) as int64."""
    g = np.asarray(gait).astype(np.int64).reshape(-1, 9)
    P = np.clip(g[:, 0], 1, MAX_PERIOD)
    off = np.mod(g[:, 1:5], P[:, None])            # numpy's mod has the divisor's sign: a non-negative residue
    st = np.clip(g[:, 5:9], 0, P[:, None])
    return P, off, st


def phase(gait, tick):
    """phi [B,...,4] of every leg at the ticks `tick` [B,...] (clamped at >= 0)."""
    P, off, _ = clamp_gait(gait)
    t = np.maximum(np.asarray(tick).astype(np.int64), 0)
    ex = (slice(None),) + (None,) * (t.ndim - 1)
    return np.mod(t[..., None] + off[ex], P[ex + (None,)])


def phase_contact(gait, tick, N):
    """contact uint8 [B,N,4]: the clock at tick + k, k < N."""
    _, _, st = clamp_gait(gait)
    t = np.maximum(np.asarray(tick).astype(np.int64), 0)[:, None] + np.arange(N)[None, :]
    return (phase(gait, t) < st[:, None, :]).astype(np.uint8)


def touchdown_mask(gait, tick):
    """bool [B,4]: leg l touches down at `tick` [B]."""
    P, _, st = clamp_gait(gait)
    steps = (st > 0) & (st < P[:, None])
    return steps & (phase(gait, tick) == 0)


def touchdown_foothold(com, psi, v, v_ref, stand, gain, gait, delta):
    """The foothold rule for all four legs: com [B,>=2], psi [B], v and v_ref [B,>=2], stand [B,4,3], gain [B] or None, the gait
    rows (for the stance time) -> p [B,4,3]."""
    com, v, vr, stand = _f64(com), _f64(v), _f64(v_ref), _f64(stand)
    B = stand.shape[0]
    psi = _f64(psi).reshape(B)
    gain = np.zeros(B) if gain is None else _f64(gain).reshape(B)
    _, _, st = clamp_gait(gait)
    half_ts = 0.5 * (st.astype(np.float64) * float(delta))                                   # [B,4]
    cs, sn = np.cos(psi)[:, None], np.sin(psi)[:, None]
    sx, sy = stand[:, :, 0], stand[:, :, 1]
    rot = [cs * sx - sn * sy, sn * sx + cs * sy]
    p = np.empty((B, 4, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(2):
            p[:, :, a] = ((com[:, None, a] + rot[a]) + half_ts * vr[:, None, a]) + gain[:, None] * (v[:, None, a] - vr[:, None, a])
    p[:, :, 2] = stand[:, :, 2]
    return p


def measured_yaw(theta):
    """Yaw of a rotation vector [B,3] the way the roll-out's advance reads it: atan2(R10, R00) of the plant's quaternion."""
    q = rotvec_to_quat(theta)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.arctan2(2.0 * (x * y + w * z), 1.0 - 2.0 * (y * y + z * z))


def _xdes(x0, ref, N, delta):
    B = len(x0)
    k = np.arange(N + 1)[None, :, None]
    xdes = np.zeros((B, N + 1, 13))
    xdes[:, :, 0], xdes[:, :, 1] = ref[:, None, 0], ref[:, None, 1]
    xdes[:, :, 2] = ref[:, None, 2] + k[:, :, 0] * delta * ref[:, None, 9]
    xdes[:, :, 3:6] = ref[:, None, 3:6] + k * delta * ref[:, None, 6:9]
    xdes[:, :, 8] = ref[:, None, 9]
    xdes[:, :, 9:12] = ref[:, None, 6:9]
    xdes[:, :, 12] = x0[:, None, 12]
    return xdes


def phase_expand_host(x0, ref, feet, gait, tick, stand, gain, N=10, delta=0.03):
    """mpcqp_phase_expand on the host: {"r" [B,N,4,3], "contact" uint8 [B,N,4], "xdes" [B,N+1,13]}."""
    x0, ref, feet, stand = _f64(x0), _f64(ref), _f64(feet), _f64(stand)
    B = len(x0)
    gainv = np.zeros(B) if gain is None else _f64(gain).reshape(B)
    P, _, st = clamp_gait(gait)
    xdes = _xdes(x0, ref, N, delta)
    t = np.maximum(np.asarray(tick).astype(np.int64), 0)[:, None] + np.arange(N)[None, :]
    phi = phase(gait, t)                                                                      # [B,N,4]
    contact = (phi < st[:, None, :]).astype(np.uint8)
    j = np.arange(N)[None, :, None] - phi
    ruled = ((st > 0) & (st < P[:, None]))[:, None, :] & (j >= 1)
    foot = np.broadcast_to(feet[:, None], (B, N, 4, 3)).copy()
    jd = np.maximum(j, 0) * float(delta)                                                      # [B,N,4]
    with np.errstate(invalid="ignore", over="ignore"):
        psi = ref[:, None, None, 2] + jd * ref[:, None, None, 9]
        cs, sn = np.cos(psi), np.sin(psi)
        sx, sy = stand[:, None, :, 0], stand[:, None, :, 1]
        rot = [cs * sx - sn * sy, sn * sx + cs * sy]
        half_ts = 0.5 * (st.astype(np.float64) * float(delta))[:, None, :]
        for a in range(2):
            c = ref[:, None, None, 3 + a] + jd * ref[:, None, None, 6 + a]
            vr = ref[:, None, None, 6 + a]
            p = ((c + rot[a]) + half_ts * vr) + gainv[:, None, None] * (x0[:, None, None, 9 + a] - vr)
            foot[:, :, :, a] = np.where(ruled, p, foot[:, :, :, a])
        foot[:, :, :, 2] = np.where(ruled, np.broadcast_to(stand[:, None, :, 2], (B, N, 4)), foot[:, :, :, 2])
        r = foot - xdes[:, :N, None, 3:6]
        r[:, 0] = foot[:, 0] - x0[:, None, 3:6]
    bad = ~(np.isfinite(stand).all(axis=(1, 2)) & np.isfinite(gainv))
    r[bad, 0] = np.nan            # the stage-0 lever arms, which never read the rule: the tuple is non-finite whatever the clock
    return {"r": r, "contact": contact, "xdes": xdes}


def rollout_phase_host(oracle_engine, x, ref, feet, gait, stand, gain, tick, mu, T, body=None, push=None, push_ticks=None,
                       substeps=DEFAULT_SUBSTEPS):
    """Closed loop of mpcqp_rollout_phase on the CPU checker (host memory, fp64).  Per tick: ``phase_expand_host``, the checker's
    ``solve_batch_host`` on that tuple, the log rows, ``plant.srb_step`` under the stage-0 forces with the held feet and the clock's
    stance mask, the reference roll-forward and the tick advance, then ``touchdown_foothold`` at the measured state for the legs that
    land at the new tick.  Returns the advanced (x, ref, tick, feet) and the logs."""
    if push is not None and push_ticks is None:
        raise ValueError("push needs push_ticks")
    cfg = oracle_engine.cfg
    N, delta = cfg.N, cfg.delta
    x = _f64(x).copy(); ref = _f64(ref).copy(); feet = _f64(feet).copy(); tick = np.asarray(tick, dtype=np.int32).copy()
    B = x.shape[0]
    body = model_body(cfg.m, list(cfg.Ibody_inv), B) if body is None else _f64(body)
    actual = np.zeros((B, T, 12)); desired = np.zeros((B, T, 12)); forces = np.zeros((B, T, 12)); solved = np.zeros(B, np.int32)
    feet_log = np.zeros((B, T, 4, 3)); contact_log = np.zeros((B, T, 4), np.uint8)
    for t in range(T):
        e = phase_expand_host(x, ref, feet, gait, tick, stand, gain, N, delta)
        o = oracle_engine.solve_batch_host(x, e["r"], e["contact"], e["xdes"], mu, want_X=False)
        actual[:, t] = x[:, :12]
        desired[:, t, 0:6] = ref[:, 0:6]; desired[:, t, 8] = ref[:, 9]; desired[:, t, 9:12] = ref[:, 6:9]
        forces[:, t] = o["u"][:, 0]
        solved += ((o["status"] == 1) | (o["status"] == 2)).astype(np.int32)
        feet_log[:, t], contact_log[:, t] = feet, e["contact"][:, 0]
        wr = None if push is None else push_wrench(push, push_ticks, tick)
        x = srb_step(x, forces[:, t], feet, e["contact"][:, 0], body, wr, delta, substeps)
        ref[:, 3:6] = ref[:, 3:6] + ref[:, 6:9] * delta
        ref[:, 2] = ref[:, 2] + ref[:, 9] * delta
        tick = tick + 1
        td = touchdown_mask(gait, tick)
        if td.any():
            p = touchdown_foothold(x[:, 3:6], measured_yaw(x[:, 0:3]), x[:, 9:12], ref[:, 6:9], stand, gain, gait, delta)
            feet = np.where(td[:, :, None], p, feet)
    return {"x": x, "ref": ref, "tick": tick, "feet": feet, "actual": actual, "desired": desired, "forces": forces, "solved": solved,
            "feet_log": feet_log, "contact_log": contact_log}


def swing_target(actual, desired, gait, stand, gain, rem, delta):
    """The target of a swing (mpcqp_phase_swing): the foothold rule at the touchdown predicted `rem` [...,4] ticks ahead of the log
    rows actual, desired [...,12] of robots [B,...] -- CoM and yaw carried (rem delta) ahead at the measured velocity and the reference
    yaw rate desired[8], v measured, v_ref = desired[9..11] -> p1 [...,4,3].  With rem = 0 it is `touchdown_foothold` at the row."""
    actual, desired, stand = _f64(actual), _f64(desired), _f64(stand)
    B = stand.shape[0]
    lead = actual.shape[1:-1]
    ex = (slice(None),) + (None,) * len(lead)
    gainv = (np.zeros(B) if gain is None else _f64(gain).reshape(B))[ex + (None,)]
    _, _, st = clamp_gait(gait)
    half_ts = (0.5 * (st.astype(np.float64) * float(delta)))[ex]                              # [B,...,4]
    ahead = _f64(rem) * float(delta)                                                          # [B,...,4]
    sx, sy = stand[ex + (slice(None), 0)], stand[ex + (slice(None), 1)]
    p = np.empty(actual.shape[:-1] + (4, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        psi = measured_yaw(actual[..., 0:3])[..., None] + ahead * desired[..., None, 8]
        cs, sn = np.cos(psi), np.sin(psi)
        rot = [cs * sx - sn * sy, sn * sx + cs * sy]
        for a in range(2):
            c = actual[..., None, 3 + a] + ahead * actual[..., None, 9 + a]
            v, vr = actual[..., None, 9 + a], desired[..., None, 9 + a]
            p[..., a] = ((c + rot[a]) + half_ts * vr) + gainv * (v - vr)
    p[..., 2] = np.broadcast_to(stand[ex + (slice(None), 2)], p.shape[:-1])
    return p


def swing_profile(s, p0, p1, step_height, t_swing):
    """The swing curve of mpcqp_phase_swing at s [...] in [0, 1] between p0 and a frozen p1 [...,3], apex step_height [...], swing
    time t_swing [...]: pos = p0 + b(s) (p1 - p0) + z_b(s) e_z with b = 3 s^2 - 2 s^3 and z_b = 16 H s^2 (1 - s)^2, and its first and
    second time derivatives -> (pos, vel, acc) [...,3]."""
    s, p0, p1, hh, tsw = _f64(s), _f64(p0), _f64(p1), _f64(step_height), _f64(t_swing)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s2, u = s * s, s * (1.0 - s)
        b0, b1, b2 = s2 * (3.0 - 2.0 * s), 6.0 * u, 6.0 - 12.0 * s
        z0, z1, z2 = (16.0 * hh) * (u * u), (32.0 * hh) * (u * (1.0 - 2.0 * s)), (32.0 * hh) * ((1.0 - 6.0 * s) + 6.0 * s2)
        dp = p1 - p0
        pos, vel, acc = p0 + b0[..., None] * dp, b1[..., None] * dp, b2[..., None] * dp
        pos[..., 2] = pos[..., 2] + z0
        vel[..., 2] = vel[..., 2] + z1
        acc[..., 2] = acc[..., 2] + z2
        return pos, vel / tsw[..., None], acc / (tsw * tsw)[..., None]


def phase_swing_host(actual, desired, feet_log, gait, tick0, stand, gain, step_height, delta=0.03):
    """mpcqp_phase_swing on the host, from the logs of a roll-out on a gait clock: actual, desired [B,T,12], feet_log [B,T,4,3], gait
    [B,9], tick0 [B] the tick BEFORE the roll-out, stand [B,4,3], gain [B] or None, step_height [B] -> {"swing": [B,T,4,4,3] (pos,
    vel, acc, target), "feet_des": [B,T,4,3] = pos}.  A swing leg runs from its lift-off foot feet_log[b,t,l] to `swing_target` at
    rem = P - phi along `swing_profile` at s = (phi - stance) / (P - stance); every other leg keeps its feet_log row, vel = acc = 0."""
    actual, desired, feet_log, stand, hh = _f64(actual), _f64(desired), _f64(feet_log), _f64(stand), _f64(step_height)
    B, T = actual.shape[:2]
    hh = hh.reshape(B)
    gainv = np.zeros(B) if gain is None else _f64(gain).reshape(B)
    P, _, st = clamp_gait(gait)
    tick = np.minimum(np.maximum(np.asarray(tick0).astype(np.int64).reshape(B, 1) + np.arange(T)[None, :], 0), 2 ** 31 - 1)
    phi = phase(gait, tick)                                                                   # [B,T,4]
    up = ((st > 0) & (st < P[:, None]))[:, None, :] & (phi >= st[:, None, :])
    n = np.where(up, P[:, None, None] - st[:, None, :], 1)
    s = np.where(up, phi - st[:, None, :], 0).astype(np.float64) / n.astype(np.float64)
    p1 = swing_target(actual, desired, gait, stand, gain, P[:, None, None] - phi, delta)
    pos, vel, acc = swing_profile(s, feet_log, p1, hh[:, None, None], n.astype(np.float64) * float(delta))
    m = up[..., None]
    out = np.stack([np.where(m, pos, feet_log), np.where(m, vel, 0.0), np.where(m, acc, 0.0), np.where(m, p1, feet_log)], axis=3)
    fin = (np.isfinite(stand).all(axis=(1, 2)) & np.isfinite(gainv) & np.isfinite(hh))[:, None, None]
    fin = fin & (np.isfinite(actual).all(axis=2) & np.isfinite(desired[:, :, 8:11]).all(axis=2))[:, :, None]
    fin = fin & np.isfinite(feet_log).all(axis=3)
    out = np.where(fin[..., None, None], out, np.nan)
    return {"swing": out, "feet_des": out[:, :, :, 0].copy()}


def log_wrench(push, push_ticks, tick0, T):
    """The push acting at every row of a roll-out's log, [B,T,6]: `plant.push_wrench` at the ticks tick0 + t (zeros for push = None)."""
    tick0 = np.asarray(tick0, dtype=np.int32)
    B = tick0.shape[0]
    if push is None:
        return np.zeros((B, T, 6))
    return np.stack([push_wrench(push, push_ticks, tick0 + t) for t in range(T)], axis=1)


LEGS_LOGS = ("swing", "q", "qd", "tau", "foot", "err", "flag", "miss")


def leg_feet_host(x, legs):
    """Where the legs hold their feet: c + R p_foot(q) [B,4,3] of the states x [B,>=12] as stored and the leg states legs [B,4,7]."""
    from . import lite3_model, plant
    x, legs = _f64(x), _f64(legs)
    R = plant.quat_to_matrix(rotvec_to_quat(x[:, 0:3]))
    with np.errstate(invalid="ignore"):
        return x[:, None, 3:6] + lite3_model._mv(R[:, None], lite3_model._leg_chain(legs[:, :, 0:3])[2][3])


def rollout_legs_host(oracle_engine, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land="rule", body=None, push=None,
                      push_ticks=None, substeps=DEFAULT_SUBSTEPS, gains=None, leg_substeps=0, inertia=None, actuators=None):
    """Closed loop of mpcqp_rollout_legs on the CPU checker (host memory, fp64): `rollout_phase_host`'s loop with, per tick, one row of
    `phase_swing_host` and one row of `lite3_model.swing_track_host` (the state carried in `legs` [B,4,7]) formed from the live
    buffers before the plant steps, under `lite3_model.plant_base_acc_host` with the robot's push; after the step the landing miss
    |c + R p_foot(q) - rule foothold| of every leg that touches down at the new tick and, with land="actual", that foot's xy in place of
    the rule's.  actuators [B,9]: per-robot actuator rows (actuators.py, include/mpcqp_actuators.h) in place of the inertia row's tau_max, or
    None.  Returns what `rollout_phase_host` returns plus "legs" and the logs LEGS_LOGS."""
    return _rollout_legs_loop(oracle_engine, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land, body, push, push_ticks,
                              substeps, gains, leg_substeps, inertia, None, None, actuators)


def rollout_drive_host(oracle_engine, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land="rule", drive="limited",
                       ground=None, body=None, push=None, push_ticks=None, substeps=DEFAULT_SUBSTEPS, gains=None, leg_substeps=0,
                       inertia=None, actuators=None):
    """Closed loop of mpcqp_rollout_drive on the CPU checker: `rollout_legs_host`'s loop with `lite3_model.stance_drive_host` between the
    solve and the legs step.  The legs step's torso acceleration, the plant and "forces" get the applied forces, "cmd" [B,T,12] the
    commanded ones; on stance rows "tau" is the rule's torque and "flag" gains its bits 2 / 16 / 32 (0xff for a poisoned leg); "drive_margin"
    [B,T,4] (host only) is the rule's margin.  The solver is not told: the next solve starts from what the last returned.  drive =
    "limited" clamps at the inertia row's tau_max -- with actuators [B,9] at each robot's envelope, at the stance rate with the foot at rest
    (actuators.py) --, "ideal" does not; ground [B] the ground's friction coefficient or None."""
    if drive not in ("ideal", "limited"):
        raise ValueError(f"drive must be 'ideal' or 'limited', got {drive!r}")
    return _rollout_legs_loop(oracle_engine, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land, body, push, push_ticks,
                              substeps, gains, leg_substeps, inertia, drive, ground, actuators)


def rollout_slip_host(oracle_engine, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, ground, foot_mass, slip=None,
                      land="rule", drive="limited", body=None, push=None, push_ticks=None, substeps=DEFAULT_SUBSTEPS, gains=None,
                      leg_substeps=0, inertia=None, actuators=None):
    """Closed loop of mpcqp_rollout_slip (include/mpcqp_slip.h) on the CPU checker: `rollout_drive_host`'s loop with
    `lite3_model.stance_slip_host` in the place of `stance_drive_host` and, after the landing, the foot move: every leg that was in
    stance on the row's tick and does not touch down on the new one has its foot's xy moved by how far it slid; a leg that touches
    down is at rest.  ground [B] and foot_mass [B] (or a number) are required; slip [B,4,2] the feet's velocities (None: at rest).
    Returns `rollout_drive_host`'s dict -- "flag" with bit 128 on the rows of a sliding leg -- plus "slip" [B,4,2], "slip_log"
    [B,T,4,2] the velocities at the start of each row and "disp" [B,T,4,2] what was added to the feet after the row."""
    if drive not in ("ideal", "limited"):
        raise ValueError(f"drive must be 'ideal' or 'limited', got {drive!r}")
    if ground is None or foot_mass is None:
        raise ValueError("rollout_slip_host needs ground and foot_mass")
    B = np.asarray(x).shape[0]
    state = {"foot_mass": np.broadcast_to(_f64(foot_mass), (B,)).copy(),
             "slip": np.zeros((B, 4, 2)) if slip is None else _f64(slip).reshape(B, 4, 2).copy()}
    return _rollout_legs_loop(oracle_engine, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land, body, push, push_ticks,
                              substeps, gains, leg_substeps, inertia, drive, ground, actuators, state)


def rollout_observe_host(oracle_engine, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, ground, foot_mass, slip=None,
                         est_state=None, feed="estimate", est_init=None, height=None, bias=None, noise=None, enc_noise=None, estimator=None,
                         land="rule", drive="limited", body=None, push=None, push_ticks=None, substeps=DEFAULT_SUBSTEPS, gains=None,
                         leg_substeps=0, inertia=None, actuators=None, gate=None, attitude=None, att_state=None):
    """Closed loop of mpcqp_rollout_observe (include/mpcqp_observe.h, which has the rule) on the CPU checker: `rollout_slip_host`'s loop
    with, per tick, the encoder and gyro rows read off the live state, one row of `estimator.estimate_track_host` on est_state [B,131]
    (None: every filter starts, from est_init [B,12] or the robot's x) and, once the slip rule has given the applied forces, the
    accelerometer row and the filter's predict.  feed="estimate": the expand and the solve read the estimate of the torso state and of
    the feet; feed="truth": they read x and feet, and every shared key is `rollout_slip_host`'s.  height [B,4], bias [B,6], noise
    [B,T,6], enc_noise [B,T,4,6] or None.  Returns `rollout_slip_host`'s dict (the plant's truth) plus "imu" [B,T,6], "q_enc", "qd_enc"
    [B,T,4,3], "est" [B,T,12], "feet_est" [B,T,4,3], "sigma" [B,T,6], "nis" [B,T] and "est_state" [B,131].
    gate: None, or a dict of estimator.gate_row's fields ({} = the defaults) for mpcqp_rollout_observe_gated (include/mpcqp_gate.h): the
    row's trust is the clock's gated on the legs' velocity innovations, and the result has "trust" [B,T,4].
    attitude: None, or a dict of estimator.attitude_row's fields ({} = the defaults) for mpcqp_rollout_observe_aided
    (include/mpcqp_attitude.h), with att_state [B,8] or None (zeros): the rows are `estimate_track_host`'s with attitude=, the controller
    reads the aided estimate, and the result has "gyro_bias" [B,T,3] and "att_state" [B,8].
    The device uses every sensor value, and a stance foot's slip velocity in its encoder row, as its I/O type holds it; nothing is rounded
    here, which is that rule only because the checker's I/O type is fp64: this is the counterpart of an fp64-I/O handle."""
    if drive not in ("ideal", "limited"):
        raise ValueError(f"drive must be 'ideal' or 'limited', got {drive!r}")
    if feed not in ("truth", "estimate"):
        raise ValueError(f"feed must be 'truth' or 'estimate', got {feed!r}")
    if ground is None or foot_mass is None:
        raise ValueError("rollout_observe_host needs ground and foot_mass")
    B = np.asarray(x).shape[0]
    state = {"foot_mass": np.broadcast_to(_f64(foot_mass), (B,)).copy(),
             "slip": np.zeros((B, 4, 2)) if slip is None else _f64(slip).reshape(B, 4, 2).copy()}
    opt = lambda a: None if a is None else _f64(a)
    observe = {"feed": feed, "state": None if est_state is None else _f64(est_state).copy(), "init": opt(est_init), "height": opt(height),
               "bias": opt(bias), "noise": opt(noise), "enc_noise": opt(enc_noise), "estimator": estimator, "gate": gate,
               "attitude": attitude, "att_state": None if attitude is None else (np.zeros((B, 8)) if att_state is None else _f64(att_state).copy())}
    if attitude is None and att_state is not None:
        raise ValueError("att_state needs attitude")
    return _rollout_legs_loop(oracle_engine, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land, body, push, push_ticks,
                              substeps, gains, leg_substeps, inertia, drive, ground, actuators, state, observe)


def _observe_sense(ob, t, x, ref, feet, legs, slip, contact, gait, tick, stand, gain, step_height, delta):
    """Step 1 of mpcqp_rollout_observe's tick on the host: the encoder and gyro rows of tick t from the live state, and the row's
    estimate from a one-row call of `estimate_track_host` with the gyro alone (the row's outputs do not depend on the specific force)
    -> (q_enc, qd_enc [B,4,3], gyro [B,3], est row [B,12], feet_est row [B,4,3])."""
    from . import estimator as _est, lite3_model
    B = x.shape[0]
    act = x[:, None, :12]
    des = np.zeros((B, 1, 12))
    des[:, 0, 0:6] = ref[:, 0:6]; des[:, 0, 8] = ref[:, 9]; des[:, 0, 9:12] = ref[:, 6:9]
    sw = phase_swing_host(act, des, feet[:, None], gait, tick, stand, gain, step_height, delta)["swing"]
    stance = contact != 0
    vel = np.where(stance[..., None], np.concatenate([slip, np.zeros((B, 4, 1))], axis=-1), sw[:, 0, :, 1])
    on = lite3_model.joint_rates_host(act, np.zeros((B, 1, 12)), sw[:, :, :, 0], vel[:, None])
    carried = (~stance & (legs[:, :, 6] != 0.0))[..., None]
    q, qd = np.where(carried, legs[:, :, 0:3], on[0][:, 0]), np.where(carried, legs[:, :, 3:6], on[1][:, 0])
    if ob["enc_noise"] is not None:
        with np.errstate(invalid="ignore"):
            q, qd = q + ob["enc_noise"][:, t, :, 0:3], qd + ob["enc_noise"][:, t, :, 3:6]
    nz = None if ob["noise"] is None else ob["noise"][:, t:t + 1]
    gyro = _est.imu_log_host(act, np.zeros((B, 1, 12)), feet[:, None], base_acc=np.zeros((B, 1, 6)), bias=ob["bias"], noise=nz,
                             estimator=ob["estimator"])[:, 0, 0:3]
    if ob["state"] is None:
        ob["state"] = np.zeros((B, _est.EST_STATE))
    if ob["init"] is None:
        ob["init"] = x[:, :12].copy()
    imu = np.concatenate([gyro, np.zeros((B, 3))], axis=-1)[:, None]
    row = _est.estimate_track_host(imu, q[:, None], qd[:, None], contact[:, None], ob["init"], height=ob["height"], state=ob["state"],
                                   estimator=ob["estimator"], delta=delta, gate=ob["gate"], attitude=ob["attitude"], att_state=ob["att_state"])
    return q, qd, gyro, row["est"][:, 0], row["feet"][:, 0]


def _observe_predict(ob, t, out, x, forces, feet, contact, q, qd, gyro, bd, wr, delta):
    """Step 4: the accelerometer row under the applied forces and the push, the row's logs and the filter's state after its predict."""
    from . import estimator as _est, lite3_model
    B = x.shape[0]
    act = x[:, None, :12]
    g = _est.estimator_row(**(ob["estimator"] or {}))["gravity"]
    acc = lite3_model.plant_base_acc_host(act, forces[:, None], feet[:, None], bd, g, None if wr is None else wr[:, None])
    nz = None if ob["noise"] is None else ob["noise"][:, t:t + 1]
    sf = _est.imu_log_host(act, forces[:, None], feet[:, None], base_acc=acc, bias=ob["bias"], noise=nz, estimator=ob["estimator"])[:, 0, 3:6]
    with np.errstate(invalid="ignore"):
        imu = np.where(np.isfinite(sf).all(-1)[:, None], np.concatenate([gyro, sf], axis=-1), np.nan)
    row = _est.estimate_track_host(imu[:, None], q[:, None], qd[:, None], contact[:, None], ob["init"], height=ob["height"], state=ob["state"],
                                   estimator=ob["estimator"], delta=delta, gate=ob["gate"], attitude=ob["attitude"], att_state=ob["att_state"])
    ob["state"] = row["state"]
    if ob["attitude"] is not None:
        ob["att_state"] = row["att_state"]
        out["gyro_bias"][:, t] = row["gyro_bias"][:, 0]
    if ob["gate"] is not None:
        out["trust"][:, t] = row["trust"][:, 0]
    out["imu"][:, t], out["q_enc"][:, t], out["qd_enc"][:, t] = imu, q, qd
    for k, src in (("est", "est"), ("feet_est", "feet"), ("sigma", "sigma"), ("nis", "nis")):
        out[k][:, t] = row[src][:, 0]


def _rollout_legs_loop(oracle_engine, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land, body, push, push_ticks, substeps,
                       gains, leg_substeps, inertia, drive, ground, actuators=None, slide=None, observe=None):
    """The loop of `rollout_legs_host` (drive = None), `rollout_drive_host`, `rollout_slip_host` (slide = its foot_mass and slip) and
    `rollout_observe_host` (observe = its feed, filter state and sensor operands; None: the controller reads the plant's state)."""
    from . import lite3_model
    if push is not None and push_ticks is None:
        raise ValueError("push needs push_ticks")
    if land not in ("rule", "actual"):
        raise ValueError(f"land must be 'rule' or 'actual', got {land!r}")
    cfg = oracle_engine.cfg
    N, delta = cfg.N, cfg.delta
    x = _f64(x).copy(); ref = _f64(ref).copy(); feet = _f64(feet).copy(); tick = np.asarray(tick, dtype=np.int32).copy()
    legs = _f64(legs).copy()
    B = x.shape[0]
    bd = model_body(cfg.m, list(cfg.Ibody_inv), B) if body is None else _f64(body)
    grav = lite3_model._inertia_arrays(inertia)["gravity"]
    # what the stance rule adds to a stance row's flag
    rule_bits = lite3_model.DRIVE_CLAMPED | lite3_model.DRIVE_UNRESOLVED | lite3_model.DRIVE_GROUND
    if slide is not None:
        rule_bits |= lite3_model.DRIVE_SLIDING
    actual = np.zeros((B, T, 12)); desired = np.zeros((B, T, 12)); forces = np.zeros((B, T, 12)); solved = np.zeros(B, np.int32)
    feet_log = np.zeros((B, T, 4, 3)); contact_log = np.zeros((B, T, 4), np.uint8)
    out = {"swing": np.zeros((B, T, 4, 4, 3)), "err": np.zeros((B, T, 4)), "flag": np.zeros((B, T, 4), np.uint8), "miss": np.zeros((B, T, 4)),
           "margin": np.full((B, T, 4), np.inf), **{k: np.zeros((B, T, 4, 3)) for k in ("q", "qd", "tau", "foot")}}
    if drive is not None:
        out["cmd"], out["drive_margin"] = np.zeros((B, T, 12)), np.full((B, T, 4), np.inf)
    if slide is not None:
        out["slip_log"], out["disp"] = np.zeros((B, T, 4, 2)), np.zeros((B, T, 4, 2))
    if observe is not None:
        out.update({"imu": np.zeros((B, T, 6)), "est": np.zeros((B, T, 12)), "sigma": np.zeros((B, T, 6)), "nis": np.zeros((B, T)),
                    **{k: np.zeros((B, T, 4, 3)) for k in ("q_enc", "qd_enc", "feet_est")}})
        if observe["gate"] is not None:
            out["trust"] = np.zeros((B, T, 4))
        if observe["attitude"] is not None:
            out["gyro_bias"] = np.zeros((B, T, 3))
    for t in range(T):
        e = phase_expand_host(x, ref, feet, gait, tick, stand, gain, N, delta)
        xc = x
        if observe is not None:     # sense and update; with feed = "estimate" the controller reads the estimate (the contact is the clock's)
            sense = _observe_sense(observe, t, x, ref, feet, legs, slide["slip"], e["contact"][:, 0], gait, tick, stand, gain, step_height, delta)
            if observe["feed"] == "estimate":
                xc = np.concatenate([sense[3], x[:, 12:]], axis=1)
                e = dict(phase_expand_host(xc, ref, sense[4], gait, tick, stand, gain, N, delta), contact=e["contact"])
        o = oracle_engine.solve_batch_host(xc, e["r"], e["contact"], e["xdes"], mu, want_X=False)
        actual[:, t] = x[:, :12]
        desired[:, t, 0:6] = ref[:, 0:6]; desired[:, t, 8] = ref[:, 9]; desired[:, t, 9:12] = ref[:, 6:9]
        forces[:, t] = o["u"][:, 0]
        if drive is not None:      # the applied forces take the place of the commanded ones from here on
            akw = {} if actuators is None else {"actuators": actuators}
            if slide is None:
                dv = lite3_model.stance_drive_host(x, o["u"][:, 0], feet, e["contact"][:, 0], ground, drive, inertia, **akw)
            else:
                out["slip_log"][:, t] = slide["slip"]
                dv = lite3_model.stance_slip_host(x, o["u"][:, 0], feet, e["contact"][:, 0], ground, slide["foot_mass"], slide["slip"], drive,
                                                  inertia, delta=delta, substeps=substeps, **akw)
            out["cmd"][:, t], forces[:, t], out["drive_margin"][:, t] = o["u"][:, 0], dv["f"], dv["margin"]
        solved += ((o["status"] == 1) | (o["status"] == 2)).astype(np.int32)
        feet_log[:, t], contact_log[:, t] = feet, e["contact"][:, 0]
        wr = None if push is None else push_wrench(push, push_ticks, tick)
        if observe is not None:
            _observe_predict(observe, t, out, x, forces[:, t], feet, contact_log[:, t], *sense[:3], bd, wr, delta)
        # the legs step: the row of the logs at this tick, through phase_swing and swing_track
        row = lambda a: a[:, t:t + 1]
        sw = phase_swing_host(row(actual), row(desired), row(feet_log), gait, tick, stand, gain, step_height, delta)["swing"]
        acc = lite3_model.plant_base_acc_host(row(actual), row(forces), row(feet_log), bd, grav, None if wr is None else wr[:, None])
        trk = lite3_model.swing_track_host(row(actual), row(forces), row(feet_log), row(contact_log), sw, acc, gains=gains, state=legs,
                                           substeps=leg_substeps, delta=delta, inertia=inertia,
                                           **({} if actuators is None else {"actuators": actuators}))
        legs = trk["state"]
        out["swing"][:, t] = sw[:, 0]
        for k in ("q", "qd", "tau", "foot", "err", "flag", "margin"):
            out[k][:, t] = trk[k][:, 0]
        if drive is not None:      # stance rows the legs step did not poison: the rule's torque and bits
            m = (contact_log[:, t] != 0) & (out["flag"][:, t] != 0xff)
            out["tau"][:, t] = np.where(m[..., None], dv["tau"], out["tau"][:, t])
            out["flag"][:, t] = np.where(m, np.where(dv["flag"] == 0xff, 0xff, out["flag"][:, t] | (dv["flag"] & rule_bits)), out["flag"][:, t])
        x = srb_step(x, forces[:, t], feet, e["contact"][:, 0], bd, wr, delta, substeps)
        ref[:, 3:6] = ref[:, 3:6] + ref[:, 6:9] * delta
        ref[:, 2] = ref[:, 2] + ref[:, 9] * delta
        tick = tick + 1
        td = touchdown_mask(gait, tick)
        if td.any():
            p = touchdown_foothold(x[:, 3:6], measured_yaw(x[:, 0:3]), x[:, 9:12], ref[:, 6:9], stand, gain, gait, delta)
            pa = leg_feet_host(x, legs)
            dlt = pa - p
            with np.errstate(invalid="ignore"):
                miss = np.sqrt((dlt[..., 0] * dlt[..., 0] + dlt[..., 1] * dlt[..., 1]) + dlt[..., 2] * dlt[..., 2])
            out["miss"][:, t] = np.where(td, miss, 0.0)
            if land == "actual":
                p[:, :, 0:2] = pa[:, :, 0:2]
            feet = np.where(td[:, :, None], p, feet)
        if slide is not None:      # the foot move: a leg that stays down, or lifts off, carries its slide; a landing foot is at rest
            move = (contact_log[:, t] != 0) & ~td
            out["disp"][:, t] = np.where(move[..., None], dv["disp"], 0.0)
            with np.errstate(invalid="ignore"):
                feet[:, :, 0:2] = np.where(move[..., None], feet[:, :, 0:2] + dv["disp"], feet[:, :, 0:2])
            slide["slip"] = np.where(td[..., None], 0.0, dv["slip"])
    return {"x": x, "ref": ref, "tick": tick, "feet": feet, "legs": legs, "actual": actual, "desired": desired, "forces": forces,
            "solved": solved, "feet_log": feet_log, "contact_log": contact_log, **out,
            **({} if slide is None else {"slip": slide["slip"]}), **({} if observe is None else {"est_state": observe["state"]}),
            **({} if observe is None or observe["attitude"] is None else {"att_state": observe["att_state"]})}


def make_phase_batch(B, names=("trot", "bound"), period=12, seed=20251018, mus=(0.5, 0.7, 1.0), v_ref=(0.18, 0.0, 0.0), theta_dot=0.0,
                     gain=0.03):
    """B robots at the start of a walk on a gait clock: state, reference descriptor, feet under the nominal stance, gait rows (robot
    b gets names[b mod len(names)]), stand rows (synth.NOMINAL_FEET x / y, ground height synth.FOOT_Z) and gains (0 for the first
    half of the robots)."""
    from .synth import FOOT_Z, G_ACC, H_COM, NOMINAL_FEET
    rng = np.random.default_rng(seed)
    names = [names] if isinstance(names, str) else list(names)
    x = np.zeros((B, 13)); ref = np.zeros((B, 10))
    com = np.array([0.0, 0.0, H_COM])[None] + rng.normal(0.0, 0.005, (B, 3)) * np.array([1.0, 1.0, 0.5])
    x[:, 3:6] = com; x[:, 6:9] = rng.normal(0.0, 0.02, (B, 3)); x[:, 9:12] = rng.normal(0.0, 0.02, (B, 3)); x[:, 12] = G_ACC
    ref[:, 3:5] = com[:, :2]; ref[:, 5] = H_COM; ref[:, 6:9] = np.asarray(v_ref, float); ref[:, 9] = theta_dot
    stand = np.tile(np.concatenate([NOMINAL_FEET[:, :2], np.full((4, 1), FOOT_Z)], axis=1), (B, 1, 1))
    stand[:, :, :2] += rng.normal(0.0, 0.003, (B, 4, 2))
    feet = stand.copy()
    feet[:, :, :2] += com[:, None, :2]
    gains = np.where(np.arange(B) < B // 2, 0.0, gain)
    mu = np.asarray(mus, float)[rng.integers(0, len(mus), B)]
    gait = gait_rows([names[b % len(names)] for b in range(B)], period)
    return {"x": x, "ref": ref, "feet": feet, "gait": gait, "stand": stand, "gain": gains, "tick": np.zeros(B, np.int32), "mu": mu}
