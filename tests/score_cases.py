"""Helpers shared by tests/test_score_host.py and tests/test_gpu_score.py (include/mpcqp_sim.h, mpcqp_rollout_score): the direct
row-by-row restatement of the score fields, the comparison under the bounds the two files hold the device and the host to, and the
synthetic logs of the device test."""
import math

import numpy as np

from conftest import REPO                                                       # (first: it puts the repository on the path)  # noqa: F401
from mpcqp import score

U = 2.0 ** -52
I = score.INDEX
LOG_KEYS = ("actual", "desired", "forces", "contact_log", "tau", "qd", "flag", "miss")
COUNTS = tuple(n for n in score.SUM_FIELDS if n.endswith("rows") or n.startswith("stance_rows") or n == "landings")
SUMS = tuple(n for n in score.SUM_FIELDS if n not in COUNTS and n not in ("vx_sum", "vy_sum"))      # the non-negative ones


def logs_of(o, rows=slice(None), robots=slice(None)):
    return {k: np.array(o[k][robots, rows]) for k in LOG_KEYS}


def direct(logs, z_frac=score.Z_FRAC, tilt_lim=score.TILT_MAX, base=0):
    """The fields as the header words them, one robot and one row at a time, on Python floats."""
    B, T = logs["actual"].shape[:2]
    out = np.zeros((B, len(score.FIELDS)))
    for b in range(B):
        s = dict.fromkeys(score.FIELDS, 0.0)
        s["fall_row"] = -1.0
        for t in range(T):
            xa, xd, f = (np.asarray(logs[k][b, t], dtype=np.float64) for k in ("actual", "desired", "forces"))
            if not (np.isfinite(xa).all() and np.isfinite(xd).all() and np.isfinite(f).all()):
                s["bad_rows"] += 1
                s["fall_row"] = base + t if s["fall_row"] < 0 else s["fall_row"]
                continue
            s["rows"] += 1
            dz, dv, da = xa[5] - xd[5], xa[9:11] - xd[9:11], xa[0:3] - xd[0:3]
            tilt = math.hypot(xa[0], xa[1])
            s["z_sq"] += dz ** 2; s["z_max"] = max(s["z_max"], abs(dz))
            s["vel_sq"] += float(dv @ dv); s["vel_max"] = max(s["vel_max"], float(np.linalg.norm(dv)))
            s["ang_sq"] += float(da @ da); s["ang_max"] = max(s["ang_max"], float(np.linalg.norm(da)))
            s["tilt_max"] = max(s["tilt_max"], tilt)
            s["vx_sum"] += xa[9]; s["vy_sum"] += xa[10]
            if (xa[5] < z_frac * xd[5] or tilt > tilt_lim) and s["fall_row"] < 0:
                s["fall_row"] = base + t
            stance = [l for l in range(4) if logs["contact_log"][b, t, l] != 0]
            s["flight_rows"] += not stance
            for l in stance:
                fx, fy, fz = f[3 * l:3 * l + 3]
                s[f"stance_rows_{l}"] += 1
                s["fz_max"] = max(s["fz_max"], fz)
                s["f_sq"] += fx ** 2 + fy ** 2 + fz ** 2
                if fz > 0:
                    s["fric_max"] = max(s["fric_max"], max(abs(fx), abs(fy)) / fz)
            for l in range(4):
                if logs.get("tau") is not None:
                    tq, qd, fl = logs["tau"][b, t, l].astype(np.float64), logs["qd"][b, t, l].astype(np.float64), int(logs["flag"][b, t, l])
                    if fl == 0xff or not (np.isfinite(tq).all() and np.isfinite(qd).all()):
                        s["poisoned_rows"] += 1
                    else:
                        p = float(tq @ qd)
                        s["tau_max"] = max(s["tau_max"], float(np.abs(tq).max())); s["tau_sq"] += float(tq @ tq)
                        s["work_pos"] += max(p, 0.0); s["work_abs"] += abs(p)
                        for name, bit in score.FLAG_BITS.items():
                            s[name] += bool(fl & bit)
                if logs.get("miss") is not None:
                    m = float(logs["miss"][b, t, l])
                    s["landings"] += m != 0
                    if math.isfinite(m):
                        s["miss_max"] = max(s["miss_max"], m); s["miss_sq"] += m ** 2
        out[b] = [s[n] for n in score.FIELDS]
    return out


def agree(a, b, T, vabs=None):
    """Counts, fall_row and bad_rows equal; maxima within 8 u; non-negative sums within (T + 8) u; the velocity sums within the same
    factor times sum |v| (`vabs` [B,2])."""
    worst = {"max": 0.0, "sum": 0.0, "v": 0.0}
    for n in COUNTS + ("fall_row",):
        assert np.array_equal(a[:, I[n]], b[:, I[n]]), n
    rel = lambda x, y: np.abs(x - y) / np.where(np.maximum(np.abs(x), np.abs(y)) > 0, np.maximum(np.abs(x), np.abs(y)), 1.0)
    for n in score.MAX_FIELDS:
        worst["max"] = max(worst["max"], float(rel(a[:, I[n]], b[:, I[n]]).max(initial=0.0)) / U)
    for n in SUMS:
        worst["sum"] = max(worst["sum"], float(rel(a[:, I[n]], b[:, I[n]]).max(initial=0.0)) / U)
    if vabs is not None:
        for j, n in enumerate(("vx_sum", "vy_sum")):
            d = np.abs(a[:, I[n]] - b[:, I[n]]) / np.where(vabs[:, j] > 0, vabs[:, j], 1.0)
            worst["v"] = max(worst["v"], float(d.max(initial=0.0)) / U)
    print(f"worst differences in units of 2^-52: maxima {worst['max']:.2f} (bound 8), sums {worst['sum']:.2f}, velocity sums {worst['v']:.2f} (bound {T + 8})")
    assert worst["max"] <= 8 and worst["sum"] <= T + 8 and worst["v"] <= T + 8
    return worst


def vabs_of(logs):
    a = np.asarray(logs["actual"], dtype=np.float64)
    fin = np.isfinite(a).all(-1) & np.isfinite(logs["desired"]).all(-1) & np.isfinite(logs["forces"]).all(-1)
    return np.where(fin[..., None], np.abs(np.nan_to_num(a[..., 9:11])), 0.0).sum(axis=1)


def synthetic_logs(B, T, seed, dtype=np.float32, bad=True):
    """Random logs [B,T,...] of the given float type, shaped to reach every branch of the reduction: f_z > 0 on stance legs (any sign on
    swing legs, which are not read), rows without a stance leg, flags from the real bit set plus some 0xff (their tau / qd NaN, as the
    roll-outs write them), misses mostly 0 with a few NaN, robots that sink or tilt past the default rule, and (bad=True) a few rows
    with a NaN or an infinity in actual, desired or forces.  Values are rounded to `dtype`, so both I/O types can hold them."""
    rng = np.random.default_rng(seed)
    actual, desired = 0.1 * rng.normal(size=(B, T, 12)), 0.1 * rng.normal(size=(B, T, 12))
    desired[..., 5] = 0.3 + 0.01 * rng.normal(size=(B, T))
    actual[..., 5] = desired[..., 5] * (1.0 - 0.1 * np.abs(rng.normal(size=(B, T))))
    sink, tilt = rng.random((B, T)) < 0.03, rng.random((B, T)) < 0.03
    actual[..., 5] = np.where(sink, 0.3 * desired[..., 5], actual[..., 5])
    actual[..., 0] = np.where(tilt, 0.9, actual[..., 0])
    contact = (rng.random((B, T, 4)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (B, T, 4)).astype(np.uint8)
    contact[rng.random((B, T)) < 0.1] = 0
    forces = 20.0 * rng.normal(size=(B, T, 4, 3))
    forces[..., 2] = np.where(contact != 0, np.abs(forces[..., 2]) + 1.0, forces[..., 2])
    flag = rng.choice(np.array([0, 0, 1, 1, 3, 5, 9, 17, 31, 2, 0xff], np.uint8), (B, T, 4))
    tau, qd = 5.0 * rng.normal(size=(B, T, 4, 3)), 3.0 * rng.normal(size=(B, T, 4, 3))
    tau[flag == 0xff], qd[flag == 0xff] = np.nan, np.nan
    miss = np.where(rng.random((B, T, 4)) < 0.15, 0.02 * np.abs(rng.normal(size=(B, T, 4))), 0.0)
    miss[rng.random((B, T, 4)) < 0.02] = np.nan
    if bad:
        for k, a in enumerate((actual, desired, forces.reshape(B, T, 12))):
            hit = rng.random((B, T)) < 0.02
            a[hit, rng.integers(0, 12)] = (np.nan, np.inf, -np.inf)[k]
    f = lambda a: np.ascontiguousarray(a, dtype=dtype)
    return {"actual": f(actual), "desired": f(desired), "forces": f(forces.reshape(B, T, 12)), "contact_log": contact, "tau": f(tau),
            "qd": f(qd), "flag": flag, "miss": f(miss)}


def rule_margin(logs, z_frac=score.Z_FRAC, tilt_max=score.TILT_MAX):
    """The smallest distance of a finite row of these logs from either threshold of the fall rule."""
    a, d = np.asarray(logs["actual"], np.float64), np.asarray(logs["desired"], np.float64)
    with np.errstate(invalid="ignore"):
        m = np.minimum(np.abs(a[..., 5] - z_frac * d[..., 5]), np.abs(np.hypot(a[..., 0], a[..., 1]) - tilt_max))
    return float(np.nanmin(m)) if m.size else np.inf
