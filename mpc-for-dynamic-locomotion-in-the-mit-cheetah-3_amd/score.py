"""The score row of a roll-out (include/mpcqp_sim.h, mpcqp_rollout_score): the field names in the C order, the numpy counterpart of the
device reduction, the per-robot figures a study reads off a score row, and the loop that scores a long roll-out piece by piece.

`MPCBatch.score(logs)` reduces the logs of `rollout`, `rollout_plant`, `rollout_phase` or `rollout_legs` on the device into one float64
row of `len(FIELDS)` values per robot; `score_host` does the same arithmetic in numpy on the same logs (every row term with the same
operations in the same order, so the two differ by the order of the sum over the ticks alone); `summarize` turns rows into RMS errors,
distance, duty factors, joint work, cost of transport, falls and landing misses; `scored_rollout` carries one score row through the pieces
of a roll-out, so that 1000 ticks of 65 536 robots need the log memory of one piece.

The logs of `rollout_drive` score like `rollout_legs`': "forces" holds the APPLIED forces, so fz_max, fric_max and f_sq are what the
plant received.  `clamp_rows` and `singular_rows` count bits 2 and 16 on any leg-row, so on a drive log they include the stance rows
whose torque the drive clamped or could not resolve (`summarize`'s clamp_share still divides by the swing rows: on a drive log count
the swing rows' bit 2 yourself if the share of saturated swings is what is wanted); bit 32, the ground's, is not counted by any field."""
from __future__ import annotations

import numpy as np

from . import _capi

# The fields in the C order (MPCQP_SCORE_* of include/mpcqp_sim.h; tests/test_score_host.py compares the two).
FIELDS = ("rows", "bad_rows", "fall_row", "z_sq", "z_max", "vel_sq", "vel_max", "ang_sq", "ang_max", "tilt_max", "vx_sum", "vy_sum",
          "fz_max", "fric_max", "f_sq", "stance_rows_0", "stance_rows_1", "stance_rows_2", "stance_rows_3", "flight_rows",
          "tau_max", "tau_sq", "work_pos", "work_abs", "swing_rows", "clamp_rows", "qlim_rows", "rate_rows", "singular_rows", "poisoned_rows",
          "landings", "miss_max", "miss_sq")
INDEX = {name: i for i, name in enumerate(FIELDS)}
MAX_FIELDS = ("z_max", "vel_max", "ang_max", "tilt_max", "fz_max", "fric_max", "tau_max", "miss_max")   # combine by max; fall_row by "the
SUM_FIELDS = tuple(n for n in FIELDS if n not in MAX_FIELDS and n != "fall_row")                        # first"; the rest add
GROUPS = {"body": FIELDS[:12], "forces": FIELDS[12:20], "legs": FIELDS[20:30], "miss": FIELDS[30:]}
Z_FRAC, TILT_MAX = 0.5, 0.7     # MPCQP_SCORE_RULE_Z_FRAC, MPCQP_SCORE_RULE_TILT_MAX: the header's convention of a fallen row
FLAG_BITS = {"swing_rows": 1, "clamp_rows": 2, "qlim_rows": 4, "rate_rows": 8, "singular_rows": 16}
POISONED = 0xff


def rule_pair(rule):
    """(z_frac, tilt_max) of a rule given as None (the defaults), a pair or a dict with either key."""
    if rule is None:
        return Z_FRAC, TILT_MAX
    if isinstance(rule, dict):
        unknown = set(rule) - {"z_frac", "tilt_max"}
        if unknown:
            raise ValueError(f"score rule: unknown key(s) {sorted(unknown)}")
        return float(rule.get("z_frac", Z_FRAC)), float(rule.get("tilt_max", TILT_MAX))
    z_frac, tilt_max = rule
    return float(z_frac), float(tilt_max)


def rule_struct(rule):
    """The MpcQpScoreRule of a rule, or None for the defaults (the library checks the values)."""
    if rule is None:
        return None
    r = _capi.MpcQpScoreRule()
    r.size = _capi.ctypes.sizeof(r)
    r.z_frac, r.tilt_max = rule_pair(rule)
    return r


def identity(B):
    """The score of no rows: zeros, fall_row -1."""
    s = np.zeros((B, len(FIELDS)))
    s[:, INDEX["fall_row"]] = -1.0
    return s


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def score_host(logs, score=None, rule=None):
    """The numpy counterpart of `MPCBatch.score`: `logs` as a roll-out returns them (arrays or tensors: "actual", "desired", "forces"
    [B,T,12], "contact_log" [B,T,4]; the leg group when "tau", "qd" and "flag" are all there; "miss" when it is), `score` float64
    [B, len(FIELDS)] to combine with (None: a fresh row; an array is combined IN PLACE and returned), `rule` as `rule_pair` takes it.
    All arithmetic in float64, every row term as csrc/mpcqp_score.h forms it."""
    z_frac, tilt_lim = rule_pair(rule)
    if not (np.isfinite(z_frac) and np.isfinite(tilt_lim) and z_frac > 0 and tilt_lim > 0):
        raise ValueError("score rule: z_frac and tilt_max must be finite and positive")
    f64 = lambda k: np.asarray(_host(logs[k]), dtype=np.float64)
    xa, xd, f = f64("actual"), f64("desired"), f64("forces")
    st = _host(logs["contact_log"]) != 0
    B, T = xa.shape[:2]
    legs = [logs.get(k) is not None for k in ("tau", "qd", "flag")]
    if any(legs) and not all(legs):
        raise ValueError("the leg group is tau, qd and flag: all three or none")
    prev = identity(B) if score is None else np.array(_host(score), dtype=np.float64)
    if prev.shape != (B, len(FIELDS)):
        raise ValueError(f"score must be {(B, len(FIELDS))}, got {prev.shape}")
    new = identity(B)
    put = lambda name, v: new.__setitem__((slice(None), INDEX[name]), v)
    fin = np.isfinite(xa).all(-1) & np.isfinite(xd).all(-1) & np.isfinite(f).all(-1)          # [B,T]: not a bad row
    xa, xd, f = (np.where(fin[..., None], a, 0.0) for a in (xa, xd, f))
    total = lambda term, ok=fin: np.where(ok, term, 0.0).sum(axis=1)
    worst = lambda term, ok=fin: np.where(ok, term, 0.0).max(axis=1, initial=0.0)
    count = lambda ok: ok.sum(axis=1).astype(np.float64)
    # ---- body
    put("rows", count(fin)); put("bad_rows", count(~fin))
    dz = xa[..., 5] - xd[..., 5]
    put("z_sq", total(dz * dz)); put("z_max", worst(np.abs(dz)))
    dvx, dvy = xa[..., 9] - xd[..., 9], xa[..., 10] - xd[..., 10]
    ev = dvx * dvx + dvy * dvy
    put("vel_sq", total(ev)); put("vel_max", worst(np.sqrt(ev)))
    d = xa[..., :3] - xd[..., :3]
    ea = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    put("ang_sq", total(ea)); put("ang_max", worst(np.sqrt(ea)))
    tilt = np.sqrt(xa[..., 0] * xa[..., 0] + xa[..., 1] * xa[..., 1])
    put("tilt_max", worst(tilt))
    put("vx_sum", total(xa[..., 9])); put("vy_sum", total(xa[..., 10]))
    down = ~fin | (xa[..., 5] < z_frac * xd[..., 5]) | (tilt > tilt_lim)
    base = prev[:, INDEX["rows"]] + prev[:, INDEX["bad_rows"]]
    first = np.where(down.any(axis=1), base + down.argmax(axis=1), -1.0) if T else np.full(B, -1.0)
    # ---- forces, stance legs only
    fl = f.reshape(B, T, 4, 3)
    fx, fy, fz = fl[..., 0], fl[..., 1], fl[..., 2]
    e = np.where(st, (fx * fx + fy * fy) + fz * fz, 0.0)
    put("f_sq", total(((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3]))
    on = st & fin[..., None]
    up = on & (fz > 0.0)
    put("fz_max", np.where(on, fz, 0.0).max(axis=(1, 2), initial=0.0))
    put("fric_max", np.where(up, np.maximum(np.abs(fx), np.abs(fy)) / np.where(up, fz, 1.0), 0.0).max(axis=(1, 2), initial=0.0))
    for l in range(4):
        put(f"stance_rows_{l}", count(on[..., l]))
    put("flight_rows", count(fin & ~st.any(-1)))
    # ---- legs
    if all(legs):
        tq, qd = f64("tau"), f64("qd")
        flag = _host(logs["flag"]).astype(np.int64)
        ok = fin[..., None] & (flag != POISONED) & np.isfinite(tq).all(-1) & np.isfinite(qd).all(-1)      # [B,T,4]
        tq, qd = np.where(ok[..., None], tq, 0.0), np.where(ok[..., None], qd, 0.0)
        e = (tq[..., 0] * tq[..., 0] + tq[..., 1] * tq[..., 1]) + tq[..., 2] * tq[..., 2]
        p = (tq[..., 0] * qd[..., 0] + tq[..., 1] * qd[..., 1]) + tq[..., 2] * qd[..., 2]
        legsum = lambda a: ((a[..., 0] + a[..., 1]) + a[..., 2]) + a[..., 3]
        put("tau_sq", total(legsum(e))); put("work_pos", total(legsum(np.maximum(p, 0.0)))); put("work_abs", total(legsum(np.abs(p))))
        put("tau_max", np.abs(tq).max(axis=(1, 2, 3), initial=0.0))
        for name, bit in FLAG_BITS.items():
            put(name, (ok & ((flag & bit) != 0)).sum(axis=(1, 2)).astype(np.float64))
        put("poisoned_rows", (fin[..., None] & ~ok).sum(axis=(1, 2)).astype(np.float64))
    # ---- landing misses
    if logs.get("miss") is not None:
        m = f64("miss")
        okm = fin[..., None] & np.isfinite(m)
        put("landings", (fin[..., None] & (m != 0.0)).sum(axis=(1, 2)).astype(np.float64))
        m = np.where(okm, m, 0.0)
        put("miss_sq", total(((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]) + m[..., 3] * m[..., 3]))
        put("miss_max", m.max(axis=(1, 2), initial=0.0))
    # ---- the row carried in and this piece
    out = prev.copy()
    for name in SUM_FIELDS:
        out[:, INDEX[name]] = prev[:, INDEX[name]] + new[:, INDEX[name]]
    for name in MAX_FIELDS:
        out[:, INDEX[name]] = np.maximum(prev[:, INDEX[name]], new[:, INDEX[name]])
    was = prev[:, INDEX["fall_row"]]
    out[:, INDEX["fall_row"]] = np.where(was >= 0, was, first)
    if isinstance(score, np.ndarray) and score.dtype == np.float64:
        score[...] = out
        return score
    return out


def summarize(score, delta, mass=None, g=9.81):
    """Per-robot figures of score rows [B, len(FIELDS)] (a numpy array or a tensor on any device; the result is of the same kind), with
    the tick length `delta` [s] and, for the cost of transport, `mass` [kg] (a number or [B]).  Rates are per scored row (`rows`; a
    robot without one gets NaN), RMS values are sqrt(sum / rows):
      rows, bad_rows, fell, fall_row, fall_time [s] (NaN where the robot did not fall)
      z_rms, z_max [m]; vel_rms, vel_max [m/s]; ang_rms, ang_max, tilt_max [rad]
      v_mean [m/s] = |sum v| / rows, distance [m] = |sum v| delta
      duty [B,4] = stance_rows / rows, flight = flight_rows / rows; fz_max [N], fric_max, f_rms [N] (the four legs' |f| per row)
      tau_max [N m], tau_rms (the twelve joints' |tau| per row), work_pos, work_abs [J] = work delta, cot = work_pos delta / (m g
      distance) where mass is given and distance > 0, NaN otherwise
      clamp_share = clamp_rows / swing_rows (0 without a swing row), qlim_rows, rate_rows, singular_rows, poisoned_rows
      landings, miss_rms [m] = sqrt(miss_sq / landings) (0 without a landing), miss_max [m]"""
    xp = np if isinstance(score, np.ndarray) else __import__("torch")
    col = lambda name: score[:, INDEX[name]]
    nan, one = float("nan"), 1.0
    rows = col("rows")
    some = rows > 0
    per_row = lambda v: xp.where(some, v / xp.where(some, rows, rows + one), rows + nan)
    rms = lambda name: xp.sqrt(per_row(col(name)))
    fell = col("fall_row") >= 0
    vsum = xp.sqrt(col("vx_sum") * col("vx_sum") + col("vy_sum") * col("vy_sum"))
    out = {"rows": rows, "bad_rows": col("bad_rows"), "fell": fell, "fall_row": col("fall_row"),
           "fall_time": xp.where(fell, col("fall_row") * delta, rows + nan),
           "z_rms": rms("z_sq"), "z_max": col("z_max"), "vel_rms": rms("vel_sq"), "vel_max": col("vel_max"),
           "ang_rms": rms("ang_sq"), "ang_max": col("ang_max"), "tilt_max": col("tilt_max"),
           "v_mean": per_row(vsum), "distance": vsum * delta,
           "duty": xp.stack([per_row(col(f"stance_rows_{l}")) for l in range(4)], -1), "flight": per_row(col("flight_rows")),
           "fz_max": col("fz_max"), "fric_max": col("fric_max"), "f_rms": rms("f_sq"),
           "tau_max": col("tau_max"), "tau_rms": rms("tau_sq"), "work_pos": col("work_pos") * delta, "work_abs": col("work_abs") * delta}
    moved = out["distance"] > 0
    if mass is None:
        out["cot"] = rows + nan
    else:
        out["cot"] = xp.where(moved, out["work_pos"] / (mass * g * xp.where(moved, out["distance"], rows + one)), rows + nan)
    swing, landed = col("swing_rows") > 0, col("landings") > 0
    out["clamp_share"] = xp.where(swing, col("clamp_rows") / xp.where(swing, col("swing_rows"), rows + one), rows * 0)
    for name in ("qlim_rows", "rate_rows", "singular_rows", "poisoned_rows", "landings"):
        out[name] = col(name)
    out["miss_rms"] = xp.sqrt(xp.where(landed, col("miss_sq") / xp.where(landed, col("landings"), rows + one), rows * 0))
    out["miss_max"] = col("miss_max")
    return out


def scored_rollout(step, T, piece, scorer=None, rule=None):
    """Roll T ticks in pieces of at most `piece` and score them into one carried row: `step(n)` is the caller's closure over one of the
    in-place roll-outs (`lambda n: sol.rollout_legs(x, ref, feet, legs, ..., tick, mu, n, ...)`; x, ref, feet, legs and tick advance in
    place, so the pieces chain by themselves) and returns that piece's logs; `scorer` is `sol.score` for device logs (required for them:
    nothing falls back to the host) and defaults to `score_host` for numpy logs.  Each piece's logs are dropped once scored, so the log
    memory is one piece's.  Returns the score row [B, len(FIELDS)]."""
    T, piece = int(T), int(piece)
    if piece < 1:
        raise ValueError(f"piece must be >= 1, got {piece}")
    score, done = None, 0
    while done < T or score is None:
        n = min(piece, T - done)
        logs = step(n)
        if scorer is None:
            if not isinstance(logs["actual"], np.ndarray):
                raise ValueError("scored_rollout: device logs need scorer=MPCBatch.score")
            scorer = score_host
        score = scorer(logs, score=score, rule=rule)
        del logs
        done += n
    return score
