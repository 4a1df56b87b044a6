"""Per-robot actuator rows with a torque-speed curve on the host (mpcqp.actuators; the `actuators=` argument of
lite3_model.swing_track_host / stance_drive_host / leg_effort_host and gaits.rollout_legs_host / rollout_drive_host;
include/mpcqp_actuators.h), no GPU: the envelope, the stance rule on a draw with one row per robot, the closed loop of the eight named
gaits under uniform and mixed tables, the growth factors the device comparisons use, and the symbol set.  The loops' counts are
printed; profiles/r19_actuators.txt and the documents quote them.  The tests assert directions, not those values."""
import os
import re

import numpy as np
import pytest

import actuator_cases as ac
import drive_cases as dc
import legsim_cases
import mpcqp
from conftest import REPO
from legsim_cases import DELTA
from mpcqp import actuators, gaits, lite3_model

INR = lite3_model.leg_inertia()
TAU_MAX, QD_MAX = INR["tau_max"], INR["qd_max"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind == "f")


# ---------------------------------------------------------------------------------------------------------------------- 1. envelope
def test_a_flat_row_is_the_box_bit_for_bit():
    rng = np.random.default_rng(1)
    B = 64
    cmd, qd = rng.normal(0.0, 40.0, (B, 4, 3)), rng.normal(0.0, 20.0, (B, 4, 3))
    cmd[0, 0], cmd[1, 0], cmd[2, 0] = [0.0, -0.0, np.nan], [24.0, -24.0, 36.0], [np.inf, -np.inf, -0.0]
    qd[3, 0], qd[4, 0] = [0.0, -0.0, np.nan], [np.inf, -np.inf, 1.0]
    scale = rng.uniform(0.3, 1.5, B)
    for free in (np.inf, 0.5, 0.0):                                             # (a flat row never reads its qd_free)
        rows = actuators.actuator_rows(B, None, scale, np.inf, free)
        assert actuators.valid_rows(rows).all() and rows.shape == (B, actuators.ROW) and rows.dtype == np.float64
        tmax = rows[:, None, 0:3]
        assert np.array_equal(rows[:, 0:3], TAU_MAX * scale[:, None])           # the product drive_cases.weak_row forms
        with np.errstate(invalid="ignore"):
            box = np.minimum(np.maximum(cmd, -tmax), tmax)
        assert np.array_equal(_bits(actuators.clamp_host(rows, cmd, qd)), _bits(box))
        lo, hi = actuators.limits_host(rows, qd)
        assert np.array_equal(lo, np.broadcast_to(-tmax, lo.shape)) and np.array_equal(hi, np.broadcast_to(tmax, hi.shape))
    assert np.array_equal(actuators.actuator_rows(3), np.tile(np.concatenate([TAU_MAX, np.full(6, np.inf)]), (3, 1)))
    assert actuators.tile(rows, 3).shape == (3 * B, 9) and np.array_equal(actuators.tile(rows, 3)[3:6], np.tile(rows[1], (3, 1)))


def test_the_curve_falls_on_the_motoring_side_only():
    rows = actuators.actuator_rows(1, None, 0.8, 0.1, 0.4)
    tm, kn, fr = rows[0, 0:3], rows[0, 3:6], rows[0, 6:9]
    assert np.allclose(kn, 0.1 * QD_MAX) and np.allclose(fr, 0.4 * QD_MAX) and np.array_equal(tm, 0.8 * TAU_MAX)
    a = np.linspace(0.0, 1.2, 241)[:, None] * fr                                # |rate| from 0 to beyond the no-load rate
    for sign in (1.0, -1.0):
        qd = (sign * a)[None]
        lo, hi = actuators.limits_host(rows, qd)
        motor, brake = (hi, -lo) if sign > 0 else (-lo, hi)
        assert np.array_equal(brake[0], np.broadcast_to(tm, a.shape))           # a braking joint keeps the full torque
        avail = motor[0]
        assert np.array_equal(avail[a <= kn], np.broadcast_to(tm, a.shape)[a <= kn]) and np.all(avail[a >= fr] == 0.0)
        assert np.all(np.diff(avail, axis=0) <= 0.0) and np.all((avail >= 0.0) & (avail <= tm))
        mid = (a > kn) & (a < fr)
        assert mid.sum() > 100 and np.allclose(avail[mid], (np.broadcast_to(tm, a.shape) * (fr - a) / (fr - kn))[mid], rtol=1e-14)
        # commanded torques either side of the envelope
        big = 100.0 * np.ones_like(qd)
        assert np.array_equal(actuators.clamp_host(rows, sign * big, qd)[0], sign * avail)
        assert np.array_equal(actuators.clamp_host(rows, -sign * big, qd)[0], np.broadcast_to(-sign * tm, a.shape))
        small = 1e-3 * np.ones_like(qd)
        inside = avail > 1e-3
        assert np.array_equal(actuators.clamp_host(rows, sign * small, qd)[0][inside], (sign * small[0])[inside])
    # the margin counts the envelope's own comparisons
    m = actuators.margin_host(rows, np.array([[0.0, 0.0, 0.0]]), np.array([kn * [1.0, 0.5, 0.5]]))
    assert m[0] == 0.0 and actuators.margin_host(actuators.actuator_rows(1), np.zeros((1, 3)), np.array([kn]))[0] == 1.0


def test_valid_rows_rejects_each_invalid_kind():
    good = actuators.actuator_rows(1, None, 1.0, 0.05, 0.25)[0]
    assert actuators.valid_rows(good[None]).all()
    kinds = {"tau_max nan": (0, np.nan), "tau_max inf": (1, np.inf), "tau_max negative": (2, -1.0), "knee negative": (3, -0.5),
             "knee nan": (4, np.nan), "free below knee": (6, good[3] * 0.5), "free equal knee": (7, good[4]), "free inf at a finite knee": (8, np.inf),
             "free nan at a finite knee": (6, np.nan), "knee -inf": (5, -np.inf)}
    rows = np.tile(good, (len(kinds), 1))
    for i, (col, val) in enumerate(kinds.values()):
        rows[i, col] = val
    ok = actuators.valid_rows(rows)
    for name, v in zip(kinds, ok):
        assert not v, name
    for edge in ((0, 0.0), (3, 0.0), (3, np.inf)):                              # tau_max = 0, knee = 0 and a flat joint are valid
        r = good.copy(); r[edge[0]] = edge[1]
        assert actuators.valid_rows(r[None]).all(), edge
    # an invalid row poisons its own robot: NaN from the clamp, nobody else changes
    mixed = np.stack([good, rows[5], good])
    out = actuators.clamp_host(mixed, np.full((3, 4, 3), 50.0), np.full((3, 4, 3), 3.0))
    assert np.isnan(out[1]).all() and np.array_equal(out[0], out[2]) and np.isfinite(out[0]).all()


# ------------------------------------------------------------------------------------------------------------ 2. the stance rule
def test_stance_drive_with_one_row_per_robot():
    c = ac.drive_draw()
    B = c["x"].shape[0]
    assert B == 33 and not actuators.valid_rows(c["rows"])[ac.INVALID_ROBOT] and actuators.valid_rows(c["rows"]).sum() == B - 1
    h64, h32 = ac.drive(c), ac.drive(ac.as_io(c, np.float32))
    st = (c["contact"] != 0)
    live = st & (h64["flag"] != 0xff)
    app = actuators.clamp_host(c["rows"], h64["tau_cmd"], h64["rate"])
    fall, flat, moving = ac.classify(c["rows"], h64["tau_cmd"], app, h64["rate"])
    print(f"draw: {int(live.sum())} live stance legs, {int((fall & live).sum())} clamped on the falling part, {int((flat & live).sum())} at tau_max, "
          f"{int((moving & live).sum())} moving and not clamped; largest stance rate {np.abs(h64['rate'][live]).max():.1f} rad/s")
    assert (fall & live).sum() >= 20 and (flat & live).sum() >= 10 and (moving & live).sum() >= 10
    assert np.array_equal(((h64["flag"] & 2) != 0)[live], (fall | flat)[live])
    for h in (h64, h32):
        near = dc.near_threshold(h)
        print(f"{int(near.sum())} of {near.size} legs near a threshold, smallest margin {h['margin'].min():.2e}")
        assert near.mean() <= dc.MARGIN_SHARE
    assert np.array_equal(h64["flag"], h32["flag"])
    # the invalid row: its robot's stance legs are NaN / 0xff; every other robot is what a run without that row gives
    b = ac.INVALID_ROBOT
    fo = h64["f"].reshape(B, 4, 3)
    assert st[b].any() and np.all(h64["flag"][b][st[b]] == 0xff) and np.isnan(fo[b][st[b]]).all() and np.isnan(h64["tau"][b][st[b]]).all()
    assert np.array_equal(_bits(fo[b][~st[b]]), _bits(c["f"].reshape(B, 4, 3)[b][~st[b]])) and not np.any(h64["flag"][np.arange(B) != b] == 0xff)
    mended = dict(c, rows=c["rows"].copy())
    mended["rows"][b] = actuators.actuator_rows(1)[0]
    hm = ac.drive(mended)
    others = np.arange(B) != b
    for k in ("f", "tau", "flag", "margin"):
        assert _same(h64[k][others], hm[k][others]), k
    # flat rows reproduce the inertia row with tau_max scaled, robot by robot and bit for bit
    assert c["flat"].sum() >= 5
    for r in np.nonzero(c["flat"])[0]:
        ref = lite3_model.stance_drive_host(c["x"], c["f"], c["feet"], c["contact"], c["ground"], inertia=dc.weak_row(c["row_scale"][r]))
        for k in ("f", "tau", "flag", "tau_cmd", "q", "reach", "margin"):
            assert _same(h64[k][r], ref[k][r]), (r, k)
    # ideal does not read the table
    ideal, ref = ac.drive(c, drive="ideal"), lite3_model.stance_drive_host(c["x"], c["f"], c["feet"], c["contact"], c["ground"], "ideal")
    for k in ("f", "tau", "flag"):
        assert _same(ideal[k], ref[k]), k
    # leg_effort's limit bit 4 on the same rows: outside the envelope at the row's rate; the invalid robot is 0xff
    a = [c["x"][:, None, :12], c["f"][:, None], c["feet"][:, None]]
    e0, e1 = lite3_model.leg_effort_host(*a), lite3_model.leg_effort_host(*a, actuators=c["rows"])
    lo, hi = actuators.limits_host(c["rows"], e1["qd"])
    with np.errstate(invalid="ignore"):
        beyond = ((e1["tau"] > hi) | (e1["tau"] < lo)).any(axis=-1)
    assert np.all(e1["limit"][b] == 0xff) and np.array_equal((e1["limit"][others] & 4) != 0, beyond[others]) and beyond[others].sum() >= 20
    assert np.array_equal(e1["limit"][others] & ~np.uint8(4), e0["limit"][others] & ~np.uint8(4)) and _same(e1["tau"], e0["tau"])
    flat_rows = actuators.actuator_rows(B)
    assert np.array_equal(lite3_model.leg_effort_host(*a, actuators=flat_rows)["limit"], e0["limit"])


# ----------------------------------------------------------------------------------------------------------------- 3. closed loop
@pytest.fixture(scope="module")
def loops(oracle_lib):
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config(N=10, delta=DELTA, max_iter=4000))
    pb = dc.loop_batch()
    run = lambda **kw: dc.run_loop(eng, pb, drive="limited", **kw)
    out = {"parent": run(), "flat": run(actuators=actuators.actuator_rows(dc.LOOP_B))}
    for name, cls in (("half", ac.HALF), ("curve", ac.CURVE), ("weak_curve", ac.WEAK_CURVE)):
        out[name] = run(actuators=ac.rows_of((cls,), dc.LOOP_B))
    out["mixed"] = run(actuators=ac.rows_of(ac.CLASSES, dc.LOOP_B))
    return pb, out


def _rows(o, bit, stance):
    m = ((o["flag"] & bit) != 0) & (o["flag"] != 0xff) & ((o["contact_log"] != 0) if stance else (o["contact_log"] == 0))
    return m.sum(axis=(1, 2))


def test_the_flat_table_is_the_parents_loop(loops):
    _, r = loops
    assert set(r["flat"]) == set(r["parent"])
    for k in r["parent"]:
        assert _same(r["parent"][k], r["flat"][k]), k
    assert not _rows(r["parent"], 2, False).any() and not _rows(r["parent"], 2, True).any()   # the Lite3's box clamps no leg-row


def test_the_curve_limits_the_swing_legs_of_every_stepping_gait(loops):
    pb, r = loops
    o = r["curve"]
    swing, stance = dict(zip(pb["names"], _rows(o, 2, False))), dict(zip(pb["names"], _rows(o, 2, True)))
    for n in pb["names"]:
        print(f"(1, 0.05, 0.25): {n:12s} {int(swing[n]):3d} clamped swing leg-rows, {int(stance[n]):3d} clamped stance leg-rows")
    assert all(swing[n] > 0 for n in pb["names"] if n != "stand") and swing["stand"] == 0 and stance["stand"] > 0
    assert np.all(o["solved"] == dc.LOOP_T) and np.isfinite(o["x"]).all() and not np.any(o["flag"] == 0xff)
    up = o["contact_log"] == 0
    print(f"swing joint rates up to {np.round(np.abs(o['qd'][up]).max(axis=0), 1)} rad/s, stance up to "
          f"{np.round(np.abs(o['qd'][~up]).max(axis=0), 1)} rad/s")


def test_the_weak_curve_also_limits_the_stance_legs_of_bound_and_gallop(loops):
    pb, r = loops
    o = r["weak_curve"]
    swing, stance = dict(zip(pb["names"], _rows(o, 2, False))), dict(zip(pb["names"], _rows(o, 2, True)))
    low = {n: (r["parent"]["actual"][b, :, 5].min(), o["actual"][b, :, 5].min()) for b, n in enumerate(pb["names"])}
    for n in pb["names"]:
        print(f"(0.5, 0.1, 0.4): {n:12s} {int(swing[n]):3d} clamped swing leg-rows, {int(stance[n]):3d} clamped stance leg-rows, "
              f"lowest CoM {low[n][0]:.3f} -> {low[n][1]:.3f} m")
    assert stance["bound"] > 0 and stance["gallop"] > 0
    assert np.all(o["solved"] == dc.LOOP_T) and np.isfinite(o["x"]).all()


def test_a_mixed_table_is_the_uniform_runs_robot_by_robot(loops):
    pb, r = loops
    uniform = {0: r["flat"], 1: r["half"], 2: r["curve"], 3: r["weak_curve"]}
    # (the flat half-strength table is the inertia row with tau_max halved: the parent's own study)
    mixed = r["mixed"]
    for b in range(dc.LOOP_B):
        ref = uniform[b % 4]
        for k in mixed:
            assert _same(mixed[k][b], ref[k][b]), (b, k)
    assert not _same(r["curve"]["q"], r["flat"]["q"]) and not _same(r["half"]["forces"], r["flat"]["forces"])


def test_flat_half_rows_are_the_halved_inertia_row(loops, oracle_lib):
    pb, r = loops
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config(N=10, delta=DELTA, max_iter=4000))
    idx = [pb["names"].index("bound"), pb["names"].index("gallop")]             # where the half row bites
    sub = {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in pb.items()}
    ref = dc.run_loop(eng, sub, drive="limited", inertia=dc.weak_row(0.5))
    assert ((ref["flag"] & 2) != 0)[ref["contact_log"] != 0].sum() > 0
    for k in ref:
        assert _same(ref[k], r["half"][k][idx]), k


# ------------------------------------------------------------------------------------------------------------- 4. growth factors
def measure_growth(oracle_lib):
    """{"draw", "rollout"}: the stance draw's outputs against the rate that enters the envelope, and swing_track_host with the table of
    the device's row-by-row test over the 16 x 25 roll-out batch (the host's own loop makes the logs)."""
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config(N=10, delta=DELTA, max_iter=4000))
    pb, rows = legsim_cases.rollout_batch()
    table = ac.rollout_rows()
    pb = dict(pb, legs=np.zeros((legsim_cases.ROLL_B, 4, 7)))
    a = [pb[k] for k in ("x", "ref", "feet", "legs", "gait", "stand", "gain", "tick", "mu")]
    logs = gaits.rollout_drive_host(eng, *a, legsim_cases.ROLL_T, np.full(legsim_cases.ROLL_B, legsim_cases.STEP_HEIGHT), land="actual",
                                    body=rows["body"], push=rows["push"], push_ticks=rows["push_ticks"], actuators=table)
    return {"draw": ac.draw_growth(), "rollout": ac.track_growth(logs, logs["swing"], rows["body"], table)}, logs


def test_the_recorded_growth_factors_are_the_hosts_own(oracle_lib):
    got, logs = measure_growth(oracle_lib)
    rec = ac.recorded_growth()
    print(f"growth factors: draw {got['draw']:.1f} (recorded {rec['draw']:.1f}), roll-out {got['rollout']:.1f} (recorded {rec['rollout']:.1f})")
    assert set(rec) == {"draw", "rollout"}
    for k in rec:
        assert 1.0 <= rec[k] < 1e3 and abs(got[k] - rec[k]) <= 0.02 * rec[k], k
    # the batch the device tests run is not vacuous on the host either: class 3 clamps swing rows, class 4 stance rows
    cls = np.arange(legsim_cases.ROLL_B) % 4
    cl = ((logs["flag"] & 2) != 0) & (logs["flag"] != 0xff)
    up = logs["contact_log"] == 0
    print(f"16 x 25 batch: clamped swing rows per class {[int((cl & up)[cls == c].sum()) for c in range(4)]}, "
          f"stance rows {[int((cl & ~up)[cls == c].sum()) for c in range(4)]}")
    assert (cl & up)[cls == 2].sum() > 0 and (cl & ~up)[cls == 3].sum() > 0


# ------------------------------------------------------------------------------------------------------------------ 5. symbol set
def test_actuators_header_declares_the_pair_product_only(oracle_lib):
    capi = mpcqp._capi
    hdr = open(os.path.join(REPO, "include", capi.ACTUATORS_HEADER)).read()
    protos = re.findall(r"^int (mpcqp_[a-z_]+)\(([^;{]*)\);", hdr, re.M)
    assert [p[0] for p in protos] == list(capi.ACTUATOR_SYMBOLS) == ["mpcqp_set_actuators", "mpcqp_clear_actuators"]
    assert "product library libmpcqp.so ONLY" in hdr and '#include "mpcqp.h"' in hdr
    table = {name: argtypes for name, _, argtypes in capi.ACTUATORS_ABI[capi.ACTUATORS_HEADER]}
    for name, params in protos:
        assert len(table[name]) == len(params.split(",")), name
    assert capi.ACTUATORS_HEADER not in capi.ABI                                 # the five headers' table is what it was
    plib = mpcqp.product_library()
    assert plib.has_actuators and all(plib.calls[s][0] is not None for s in capi.ACTUATOR_SYMBOLS) and plib.version() == 0x00010301
    assert not oracle_lib.has_actuators and not any(hasattr(oracle_lib.lib, s) for s in capi.ACTUATOR_SYMBOLS)
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    for call in (lambda: eng.set_actuators_ptr(1, 1), eng.clear_actuators):
        with pytest.raises(mpcqp.MpcQpError, match=r"does not export include/mpcqp_actuators.h \(product library only\)"):
            call()
    oracle_src = open(os.path.join(REPO, "oracle", "mpcqp_oracle.c")).read()
    assert "actuators" not in oracle_src
