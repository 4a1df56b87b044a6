"""Host counterpart of the per-leg periodic gaits (mpcqp.gaits; include/mpcqp_plan.h, mpcqp_sim.h): the phase clock against the
two contact generators the project already has, its clamp rules, the expansion on a stand row, the foothold rule, a short closed loop
on the CPU checker and the C interface's symbol set.  No GPU: the device is held to this module in tests/test_gpu_gaits.py."""
import os
import re

import numpy as np
import pytest

import mpcqp
from conftest import ORACLE_SO, REPO
from mpcqp import gaits, synth

NEW_SYMBOLS = {"mpcqp_plan.h": ("mpcqp_phase_expand", "mpcqp_solve_batch_phase"), "mpcqp_sim.h": ("mpcqp_rollout_phase",)}


def _row(P, off, st):
    return np.array([[P, *off, *st]], np.int32)


def test_phase_contact_is_the_perleg_clock():
    for N in (10, 24):
        b = synth.make_perleg_batch(300, N=N)
        tm = b["timing"]
        gait = np.concatenate([tm["period"][:, None], tm["offset"], tm["stance"]], axis=1).astype(np.int32)
        assert np.array_equal(gaits.phase_contact(gait, b["t0"], N), synth.perleg_contact(tm, b["t0"], N))
        assert np.array_equal(gaits.phase_contact(gait, b["t0"], N), b["contact"])


@pytest.mark.parametrize("name", ["trot", "gallop"])
def test_two_beat_gait_as_a_phase_gait_reproduces_the_contact_schedule(name):
    ss, ds, N = synth.SS_TICKS, synth.DS_TICKS, 40
    P = 2 * (ss + ds)
    base = np.asarray(synth.GAITS[name])
    # a leg that swings in a step's first ss ticks (base 0) has phase P - ss at tick 0; the other pair swings a step later
    off = np.where(base == 0, P - ss, P - 2 * ss - ds)
    gait = _row(P, off, [P - ss] * 4)
    t0 = np.array([0, 1, ss - 1, ss, ss + ds - 1, ss + ds, P - 1, P, 7 * P + 3, 12345])
    want = synth.contact_schedule(np.zeros(len(t0), int), t0, N, gaits=[synth.GAITS[name]])
    assert np.array_equal(gaits.phase_contact(np.repeat(gait, len(t0), axis=0), t0, N), want)
    assert want.min() == 0 and want[:, :, 0].max() == 1


def test_hostile_rows_are_clamped():
    big = 2 ** 31 - 1
    P, off, st = gaits.clamp_gait(np.array([[0, 5, -1, 7, 0, 3, 0, 1, 9],            # P <= 0 -> 1: every offset 0, stance into [0, 1]
                                            [-7, 1, 2, 3, 4, -5, 0, 1, 2],
                                            [10, -1, -10, -13, 25, 11, -3, 10, 0],   # negative offsets, stance > P, stance < 0
                                            [70000, 65536, -65536, 1, 2, 70000, 65535, 1, 2],
                                            [7, big, -big - 1, big - 3, 0, 3, 3, 3, 3]]))
    assert P.tolist() == [1, 1, 10, 65535, 7]
    assert off.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [9, 0, 7, 5], [1, 65534, 1, 2], [big % 7, (-big - 1) % 7, (big - 3) % 7, 0]]
    assert st.tolist() == [[1, 0, 1, 1], [0, 0, 1, 1], [10, 0, 10, 0], [65535, 65535, 1, 2], [3, 3, 3, 3]]
    assert (off >= 0).all() and (off < P[:, None]).all()
    # negative ticks clamp to 0; tick + offset near 2^31 does not wrap
    g = _row(10, [3, 0, 9, 5], [5, 5, 5, 5])
    assert np.array_equal(gaits.phase_contact(g, [-4], 6), gaits.phase_contact(g, [0], 6))
    g = _row(65535, [65534, 0, 1, 2], [30000] * 4)
    c = gaits.phase_contact(g, [big - 2], 8)
    t = big - 2 + np.arange(8, dtype=object)
    want = [[int((int(tt) + o) % 65535 < 30000) for o in (65534, 0, 1, 2)] for tt in t]
    assert c[0].tolist() == want
    # stance = P never lifts, stance = 0 never lands, and neither has a touchdown
    g = _row(6, [0, 0, 2, 3], [6, 0, 3, 3])
    c = gaits.phase_contact(g, [0], 18)[0]
    assert c[:, 0].all() and not c[:, 1].any()
    td = np.array([gaits.touchdown_mask(g, [t])[0] for t in range(12)])
    assert not td[:, 0].any() and not td[:, 1].any()
    assert np.flatnonzero(td[:, 2]).tolist() == [4, 10] and np.flatnonzero(td[:, 3]).tolist() == [3, 9]
    assert np.array_equal(td[1:, 2], (c[1:12, 2] == 1) & (c[:11, 2] == 0))          # a touchdown is a 0 -> 1 edge of the mask


def test_expand_on_a_stand_row_is_the_gait_expansion_on_the_held_feet():
    for N in (10, 24):
        g = synth.make_gait_batch(64, N=N)
        B = len(g["x0"])
        g["ref"][:, 9] = np.random.default_rng(1).normal(0.0, 0.3, B)              # a turning reference
        held = dict(g, footholds=np.repeat(g["feet0"][:, None], 2, axis=1), feet_id=np.ones((B, 2, 4), np.uint8))
        want = synth.expand_gait_batch(held, N=N)
        gait = np.repeat(_row(9, [1, 2, 3, 4], [9] * 4), B, axis=0)
        stand = np.full((B, 4, 3), 5.0)                                             # never read: no leg steps
        e = gaits.phase_expand_host(g["x0"], g["ref"], g["feet0"], gait, np.arange(B), stand, None, N=N)
        assert np.array_equal(e["r"], want["r"]) and np.array_equal(e["xdes"], want["xdes"]) and e["contact"].all()


def test_foothold_rule_and_its_velocity_feedback():
    # dyadic inputs: every operation of the rule is exact, so the displacement is exactly gain (v - v_ref)
    com = np.array([[0.5, -0.25, 0.3125]]); v = np.array([[0.75, -0.5, 0.0]]); vr = np.array([[0.25, 0.125, 0.0]])
    stand = np.array([[[0.125, 0.25, 0.0625], [0.125, -0.25, 0.0625], [-0.25, 0.25, 0.0], [-0.25, -0.25, 0.0]]])
    gait = _row(16, [0, 8, 8, 0], [8, 8, 4, 4])
    p0 = gaits.touchdown_foothold(com, [0.0], v, vr, stand, None, gait, 0.03125)
    p1 = gaits.touchdown_foothold(com, [0.0], v, vr, stand, [0.25], gait, 0.03125)
    assert np.array_equal(p1[0, :, :2] - p0[0, :, :2], np.tile(0.25 * (v - vr)[0, :2], (4, 1)))
    assert np.array_equal(p0[0, :, 2], stand[0, :, 2]) and np.array_equal(p1[0, :, 2], stand[0, :, 2])
    half_ts = 0.5 * np.array([8, 8, 4, 4]) * 0.03125
    assert np.array_equal(p0[0, :, :2], com[0, None, :2] + stand[0, :, :2] + half_ts[:, None] * vr[0, None, :2])
    # a quarter turn carries the stand row round with it
    pq = gaits.touchdown_foothold(com, [np.pi / 2], vr, vr, stand, [0.25], gait, 0.03125)
    want = com[0, None, :2] + np.stack([-stand[0, :, 1], stand[0, :, 0]], axis=1) + half_ts[:, None] * vr[0, None, :2]
    assert np.abs(pq[0, :, :2] - want).max() <= 1e-15
    # the yaw the roll-out measures is the yaw of a yaw-only rotation vector
    assert np.abs(gaits.measured_yaw(np.array([[0.0, 0.0, 0.7], [0.0, 0.0, -2.5], [0.0, 0.0, 0.0]])) - [0.7, -2.5, 0.0]).max() <= 1e-15


def test_expand_uses_the_rule_at_the_reference_pose_of_the_touchdown_stage():
    N, d = 10, 0.03
    pb = gaits.make_phase_batch(8, ("trot", "bound"), 8, theta_dot=0.4)
    e = gaits.phase_expand_host(pb["x"], pb["ref"], pb["feet"], pb["gait"], pb["tick"] + 3, pb["stand"], pb["gain"], N, d)
    assert np.array_equal(e["contact"], gaits.phase_contact(pb["gait"], pb["tick"] + 3, N))
    phi = gaits.phase(pb["gait"], (pb["tick"] + 3)[:, None] + np.arange(N)[None, :])
    seen = set()
    for b in range(8):
        for k in range(N):
            for l in range(4):
                j = k - phi[b, k, l]
                com = pb["x"][b, 3:6] if k == 0 else pb["ref"][b, 3:6] + k * d * pb["ref"][b, 6:9]
                if j >= 1:
                    ref_j = pb["ref"][b:b + 1, 3:6] + j * d * pb["ref"][b:b + 1, 6:9]
                    p = gaits.touchdown_foothold(ref_j, pb["ref"][b:b + 1, 2] + j * d * 0.4, pb["x"][b:b + 1, 9:12], pb["ref"][b:b + 1, 6:9],
                                                 pb["stand"][b:b + 1], pb["gain"][b:b + 1], pb["gait"][b:b + 1], d)[0, l]
                else:
                    p = pb["feet"][b, l]
                seen.add(j >= 1)
                assert np.abs(e["r"][b, k, l] - (p - com)).max() <= 1e-15, (b, k, l)
    assert seen == {True, False}
    bad = pb["stand"].copy(); bad[2, 1, 0] = np.inf
    eb = gaits.phase_expand_host(pb["x"], pb["ref"], pb["feet"], pb["gait"], pb["tick"], bad, pb["gain"], N, d)
    assert np.isnan(eb["r"][2, 0]).all() and np.isfinite(np.delete(eb["r"], 2, axis=0)).all()      # stage 0 is poisoned whatever the clock


def test_named_rows():
    rows = gaits.gait_rows(list(gaits.GAITS), 20)
    assert set(gaits.GAITS) == {"trot", "flying_trot", "pace", "bound", "pronk", "gallop", "walk", "stand"}
    c = {n: gaits.phase_contact(rows[i:i + 1], [0], 20)[0] for i, n in enumerate(gaits.GAITS)}
    assert c["stand"].all()
    assert np.array_equal(c["trot"][:, 0], c["trot"][:, 3]) and np.array_equal(c["trot"][:, 1], c["trot"][:, 2])
    assert c["trot"].sum(axis=1).min() == 2 and c["trot"].sum(axis=1).max() == 4
    assert c["flying_trot"].sum(axis=1).min() == 0 and c["pronk"].sum(axis=1).tolist().count(0) == 10
    assert np.array_equal(c["pace"][:, 0], c["pace"][:, 2]) and np.array_equal(c["bound"][:, 0], c["bound"][:, 1])
    assert set(c["walk"].sum(axis=1).tolist()) == {3} and c["gallop"].sum(axis=1).min() == 0
    for n in gaits.GAITS:
        assert np.all(c[n].sum(axis=0) == c[n][:, 0].sum()), n                      # one duty factor per gait
    with pytest.raises(ValueError, match="period"):
        gaits.gait_rows("trot", 0)


def test_short_closed_loop_on_the_checker():
    lib = mpcqp.Library(ORACLE_SO)
    eng = mpcqp.Engine(lib, lib.default_config(N=10, delta=0.03, max_iter=4000))
    P, B = 8, 4
    T = 2 * P
    pb = gaits.make_phase_batch(B, ("trot", "bound"), P, seed=3)
    o = gaits.rollout_phase_host(eng, pb["x"], pb["ref"], pb["feet"], pb["gait"], pb["stand"], pb["gain"], pb["tick"], pb["mu"], T)
    assert np.all(o["solved"] == T) and np.all(o["tick"] == T)
    assert np.array_equal(o["contact_log"], gaits.phase_contact(pb["gait"], pb["tick"], T))
    assert np.array_equal(o["feet_log"][:, 0], pb["feet"])
    cl, fl = o["contact_log"], o["feet_log"]
    landed = (cl[:, 1:] == 1) & (cl[:, :-1] == 0)
    assert landed.any(axis=1).all() and landed.sum() == 2 * 4 * B - 2 * B            # (the pair that starts in stance lands once)
    same = (fl[:, 1:] == fl[:, :-1]).all(axis=3)
    assert same[~landed].all() and not same[landed].any()                            # held feet: bitwise constant between touchdowns
    # every landing is the rule at the state the log holds
    for t in range(T - 1):
        x = o["actual"][:, t + 1]
        p = gaits.touchdown_foothold(x[:, 3:6], gaits.measured_yaw(x[:, 0:3]), x[:, 9:12], pb["ref"][:, 6:9], pb["stand"], pb["gain"],
                                     pb["gait"], 0.03)
        assert np.array_equal(fl[:, t + 1][landed[:, t]], p[landed[:, t]])
    a = o["actual"]
    assert np.abs(a[:, :, 5] - 0.285).max() < 0.05 and np.abs(a[:, :, 0:2]).max() < 0.1


def test_headers_declare_the_calls_and_the_library_exports_them():
    lib = mpcqp.product_library()
    for header, names in NEW_SYMBOLS.items():
        text = open(os.path.join(REPO, "include", header)).read()
        table = [row[0] for row in mpcqp._capi.ABI[header]]
        for name in names:
            assert re.search(rf"^int {name}\(", text, re.M), name
            assert name in table and hasattr(lib.lib, name), name
    assert len(mpcqp._capi.ABI) == 5 and lib.version() == 0x00010301
    for name in ("phase_expand", "solve_batch_phase", "rollout_phase"):
        assert callable(getattr(mpcqp.MPCBatch, name)) and callable(getattr(mpcqp.Engine, name + "_ptr"))
