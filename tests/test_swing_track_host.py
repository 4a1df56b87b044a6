"""Host counterparts of the swing-leg plant (mpcqp.lite3_model.leg_accel_host, swing_track_host; include/mpcqp_joints.h,
mpcqp_leg_accel / mpcqp_swing_track): the forward dynamics against the inverse, the order of the integrator, recovery from an offset,
saturation, the stability bound behind the default control period, stance rows against joint_rates_host, the landing miss, and a log
tracked in two pieces.  No GPU: the device is held to this module in tests/test_gpu_swing_track.py.

Measured when the tests were written (DESIGN.md has them too): lambda = 106.5 / s over the joint box; feed-forward landing error 4.98 /
2.49 / 1.24 mm at 15 / 30 / 60 control periods per tick; recovery from 2 cm to 0.48 mm over a five-tick swing."""
import functools

import numpy as np

import mpcqp
from conftest import ORACLE_SO
from legsim_cases import (DELTA, GROWTH_NPZ, ROLL_T, STEP_HEIGHT, box_rows, flag_margins, growth_factor, parabola_logs, rollout_batch,
                          track, turning_logs)
from mpcqp import gaits, lite3_model


# ------------------------------------------------------------------------------------------------------------ 1. forward dynamics
def test_leg_accel_inverts_leg_dynamics():
    q, ops = box_rows()
    tau = lite3_model.leg_dynamics_host(q, ops["qd"], ops["qdd"], ops["rot"], ops["base"])[0]
    qdd, det = lite3_model.leg_accel_host(q, tau, ops["qd"], ops["rot"], ops["base"])
    back = lite3_model.leg_dynamics_host(q, ops["qd"], qdd, ops["rot"], ops["base"])[0]
    print(f"leg_accel round trip: |tau' - tau| {np.abs(back - tau).max():.3e} N m, |qdd' - qdd| {np.abs(qdd - ops['qdd']).max():.3e} rad/s^2, "
          f"det M in [{det.min():.3e}, {det.max():.3e}]")
    assert np.abs(back - tau).max() <= 1e-12 and np.all(det > 0.0)
    for drop in (("qd",), ("rot",), ("base",), ("qd", "rot", "base")):            # each optional operand absent
        use = {k: (None if k in drop else ops[k]) for k in ("qd", "rot", "base")}
        a = lite3_model.leg_accel_host(q, tau, **use)[0]
        assert np.abs(lite3_model.leg_dynamics_host(q, use["qd"], a, use["rot"], use["base"])[0] - tau).max() <= 1e-12, drop
    # massless legs do not accelerate; a non-finite operand stays in its own leg / row
    none = lite3_model.leg_inertia()
    for k in ("mass", "com", "inertia"):
        none[k] = np.zeros_like(none[k])
    a0, d0 = lite3_model.leg_accel_host(q, tau, ops["qd"], ops["rot"], ops["base"], inertia=none)
    assert not a0.any() and not d0.any()
    t2, b2 = tau.copy(), ops["base"].copy()
    t2[3, 1, 0] = np.nan; b2[5, 4] = np.inf
    a2 = lite3_model.leg_accel_host(q, t2, ops["qd"], ops["rot"], b2)[0]
    hit = np.zeros(q.shape[:2], bool); hit[3, 1] = True; hit[5] = True
    assert np.isnan(a2[hit]).all() and np.array_equal(a2[~hit], qdd[~hit])


# --------------------------------------------------------------------------------------------------- 2. the order of the integrator
def test_pure_feed_forward_is_first_order():
    """Kp = Kd = 0 on parabolas (the desired arc of a row is exact): the landing miss is the semi-implicit Euler step's truncation."""
    s = parabola_logs(5, B=2)
    zero = np.zeros((2, 2))
    miss = {}
    for n in (15, 30, 60):
        o = track(s, substeps=n, gains=zero)
        assert np.all(o["flag"][:, 1:-1] == 1) and np.all(o["flag"][:, -1] == 64) and np.all(o["err"][:, 1] <= 1e-12)
        miss[n] = float(o["err"][:, -1].max())
    print("feed-forward landing miss: " + ", ".join(f"{v * 1e3:.3f} mm at h = {DELTA / n * 1e3:.2f} ms" for n, v in miss.items()))
    for a, b in ((15, 30), (30, 60)):
        assert 1.8 <= miss[a] / miss[b] <= 2.2, (a, b, miss)


def test_first_order_on_a_turning_accelerating_torso():
    """The same on a torso with constant angular and linear acceleration, whose rows are exact samples of its motion: what is left at
    the landing is the step's truncation (the quaternion step included), with and without feedback.  A wrong sign in a torso term
    does not shrink with h: in the recursion's omega, alpha, a it would show without feedback, in foot_vel's omega x (R p) as a
    steady offset Kd / Kp times the velocity error under PD.  Measured 5.317 / 2.655 / 1.326 mm and 1.362 / 0.683 / 0.342 mm."""
    s = turning_logs(5, B=2)
    assert np.abs(s["actual"][:, -1, 0:3]).max() > 0.1 and np.abs(s["base_acc"]).min(axis=(0, 1)).max() > 0.0
    for what, gains in (("feed-forward", np.zeros((2, 2))), ("default gains", None)):
        miss = {n: float(track(s, substeps=n, gains=gains)["err"][:, -1].max()) for n in (15, 30, 60)}
        print(f"turning torso, {what}: " + ", ".join(f"{v * 1e3:.3f} mm at h = {DELTA / n * 1e3:.2f} ms" for n, v in miss.items()))
        for a, b in ((15, 30), (30, 60)):
            assert 1.8 <= miss[a] / miss[b] <= 2.2, (what, a, b, miss)


# ------------------------------------------------------------------------------------------------------------------- 3. recovery
def test_recovery_from_two_centimetres():
    s = parabola_logs(5, B=2, offset=0.02)                                        # a 12-tick-period trot: 7 stance, 5 swing ticks
    o = track(s)
    print(f"recovery, default gains and period: err per row {np.round(o['err'][0, :, 0] * 1e3, 3)} mm, worst at the landing "
          f"{o['err'][:, -1].max() * 1e3:.3f} mm")
    assert abs(o["err"][0, 0, 0] - 0.02) <= 1e-9
    assert o["err"][:, -1].max() <= 2e-3 and not np.any(o["flag"] & 2) and np.all(o["flag"] != 0xff)


# ------------------------------------------------------------------------------------------------------------------ 4. saturation
def test_saturated_actuators_clamp_and_lose_the_foot():
    s = parabola_logs(5, B=2, offset=0.08)                                        # (at 5 cm the command stays below a tenth of tau_max)
    weak = lite3_model.leg_inertia()
    weak["tau_max"] = 0.1 * weak["tau_max"]
    full, o = track(s), track(s, inertia=weak)
    up = s["contact_log"] == 0
    assert np.any(o["flag"][up] & 2) and not np.any(full["flag"] & 2)
    assert np.all(np.abs(o["tau"][up]) <= weak["tau_max"])                        # exactly: the clamp writes the limit itself
    assert np.any(np.abs(o["tau"][up]) == weak["tau_max"])
    print(f"saturation at 10 % tau_max: landing err {o['err'][:, -1].max() * 1e3:.2f} mm against {full['err'][:, -1].max() * 1e3:.2f} mm, "
          f"summed err {o['err'].sum():.4f} against {full['err'].sum():.4f} m")
    assert o["err"].sum() > full["err"].sum() and o["err"][:, -1].max() > full["err"][:, -1].max()


# ------------------------------------------------------------------------------------------------------------- 5. the stability bound
@functools.lru_cache(maxsize=None)
def _stand_to_trot(T=200):
    pb = gaits.make_phase_batch(1, ("trot",), 12, seed=6)
    lib = mpcqp.Library(ORACLE_SO)
    eng = mpcqp.Engine(lib, lib.default_config(N=10, delta=DELTA, max_iter=4000))
    o = gaits.rollout_phase_host(eng, pb["x"], pb["ref"], pb["feet"], pb["gait"], pb["stand"], pb["gain"], pb["tick"], pb["mu"], T)
    sw = gaits.phase_swing_host(o["actual"], o["desired"], o["feet_log"], pb["gait"], pb["tick"], pb["stand"], pb["gain"],
                                np.full(1, STEP_HEIGHT), DELTA)
    return o, sw["swing"]


def test_stability_bound_and_default_period(oracle_lib):
    rng = np.random.default_rng(41)
    n = 20000
    q = np.stack([rng.uniform(-0.5, 0.5, (n, 4)), rng.uniform(-1.5, -0.2, (n, 4)), rng.uniform(0.5, 2.3, (n, 4))], axis=-1)
    lam = float(lite3_model.swing_gain_lambda(q).max())
    h0 = max(h for h in (2e-3, 1e-3, 5e-4, 2.5e-4) if h <= 0.5 / lam)
    print(f"lambda = {lam:.2f} / s over {4 * n} legs of the joint box: h < {2.0 / lam * 1e3:.2f} ms, 0.5 / lambda = {0.5 / lam * 1e3:.2f} ms, h0 = {h0 * 1e3:g} ms")
    assert 100.0 < lam < 115.0 and h0 == lite3_model.SWING_H0 == 2e-3
    assert lite3_model.swing_substeps(DELTA) == 15 and lite3_model.swing_substeps(0.01) == 5 and lite3_model.swing_substeps(DELTA, 7) == 7
    o, swing = _stand_to_trot()
    a = [o[k] for k in ("actual", "forces", "feet_log", "contact_log")]
    good = lite3_model.swing_track_host(*a, swing, delta=DELTA)
    up = o["contact_log"] == 0
    print(f"200-tick stand-to-trot at h0: worst err {good['err'].max() * 1e3:.2f} mm, worst landing miss "
          f"{good['err'][(good['flag'] & 64) != 0].max() * 1e3:.2f} mm, {int(up.sum())} swing rows")
    # bounded: finite, far inside the leg's 0.41 m, and the second hundred ticks no worse than twice the first (measured 27.3 mm, at
    # landings: the target of a real swing moves from row to row, which is tracking error, not growth)
    assert up.sum() > 100 and np.all(good["flag"] != 0xff) and good["err"].max() < 0.1
    assert good["err"][:, 100:].max() <= 2.0 * good["err"][:, :100].max()
    # at h = 4 / lambda the damping term alone overshoots.  lambda scales with Kd: at Kd' = Kd (4 / delta) / lambda one whole tick is
    # 4 / lambda', so one control period per tick is that step.  A stance row re-initialises the leg, so the growth has one swing: a
    # millimetre off the parabola at lift-off ends more than a hundred times further off, where the step the rule gives for lambda'
    # (0.5 / lambda' = 3.75 ms -> 2 ms, 15 periods) brings two centimetres back
    kd = lite3_model.SWING_KD * (4.0 / DELTA) / lam
    gains = np.tile([[lite3_model.SWING_KP, kd]], (2, 1))
    wild = track(parabola_logs(5, B=2, offset=1e-3), gains=gains, substeps=1)
    calm = track(parabola_logs(5, B=2, offset=0.02), gains=gains, substeps=15)
    print(f"h = 4 / lambda (Kd = {kd:.2f}, one period per tick): err per row {np.round(wild['err'][0, :, 0] * 1e3, 1)} mm from 1 mm; at 2 ms "
          f"{np.round(calm['err'][0, :, 0] * 1e3, 2)} mm from 20 mm")
    assert wild["err"][:, -1].min() > 0.1 and np.all(wild["flag"] != 0xff) and calm["err"][:, -1].max() < 5e-3


# -------------------------------------------------------------------------------------------------------------------- 6. stance rows
@functools.lru_cache(maxsize=None)
def _loop():
    """The end-to-end case of the device test on the CPU checker: 16 robots, the eight gaits, two of them pushed."""
    pb, rows = rollout_batch()
    lib = mpcqp.Library(ORACLE_SO)
    eng = mpcqp.Engine(lib, lib.default_config(N=10, delta=DELTA, max_iter=4000))
    o = gaits.rollout_phase_host(eng, pb["x"], pb["ref"], pb["feet"], pb["gait"], pb["stand"], pb["gain"], pb["tick"], pb["mu"], ROLL_T,
                                 rows["body"], rows["push"], rows["push_ticks"])
    sw = gaits.phase_swing_host(o["actual"], o["desired"], o["feet_log"], pb["gait"], pb["tick"], pb["stand"], pb["gain"],
                                np.full(len(pb["x"]), STEP_HEIGHT), DELTA)
    return pb, rows, o, sw["swing"]


def test_stance_rows_are_joint_rates(oracle_lib):
    pb, rows, o, swing = _loop()
    out = lite3_model.swing_track_host(o["actual"], o["forces"], o["feet_log"], o["contact_log"], swing, None, rows["body"], delta=DELTA)
    q, qd, tau, _, _ = lite3_model.joint_rates_host(o["actual"], o["forces"], swing[:, :, :, 0], swing[:, :, :, 1])
    down = o["contact_log"] != 0
    for k, ref in (("q", q), ("qd", qd), ("tau", tau)):
        assert np.abs(out[k][down] - ref[down]).max() <= 1e-12, k
    assert np.all((out["flag"][down] & 1) == 0) and np.all((out["flag"][~down] & 1) == 1)
    lift = ~down[:, 1:] & down[:, :-1]                                         # a lift-off row starts on its trajectory
    assert lift.any() and out["err"][:, 1:][lift].max() <= 1e-9


# ------------------------------------------------------------------------------------------------------------------ 7. landing miss
def test_landing_miss(oracle_lib):
    # a perfect start on an unpushed, uniformly moving robot: the miss is below the feed-forward truncation of test 2 at the same h
    s = parabola_logs(5, B=2)
    ff = float(track(s, gains=np.zeros((2, 2)))["err"][:, -1].max())
    pd = track(s)
    assert np.all(pd["flag"][:, -1] == 64) and 0.0 < pd["err"][:, -1].max() < ff
    # the closed loop with pushes: every landing row carries bit 64 and its err is |foot(carried q) - pos| by hand
    pb, rows, o, swing = _loop()
    a = (o["actual"], o["forces"], o["feet_log"], o["contact_log"])
    out = lite3_model.swing_track_host(*a, swing, None, rows["body"], delta=DELTA)
    down = o["contact_log"] != 0
    landed = np.zeros_like(down); landed[:, 1:] = down[:, 1:] & ~down[:, :-1]
    assert landed.sum() >= 2 * len(pb["x"]) and np.array_equal((out["flag"] & 64) != 0, landed)
    checked = 0
    for b, t, l in list(zip(*np.nonzero(landed)))[::9]:                          # every ninth landing: all gaits, early and late rows
        st = lite3_model.swing_track_host(*[x[b:b + 1, :t] for x in a], swing[b:b + 1, :t], None, rows["body"][b:b + 1], delta=DELTA)["state"]
        R = mpcqp.plant.quat_to_matrix(mpcqp.plant.rotvec_to_quat(o["actual"][b, t, 0:3]))
        foot = o["actual"][b, t, 3:6] + R @ lite3_model.leg_fk_jac(l, st[0, l, 0:3])[0]
        miss = np.linalg.norm(foot - swing[b, t, l, 0])
        assert st[0, l, 6] == 1.0 and abs(miss - out["err"][b, t, l]) <= 1e-12 and miss > 0.0, (b, t, l)
        checked += 1
    assert checked >= 12
    # no (robot, tick, leg) of this case sits within 1e-9 of a threshold that decides a flag bit: the device test compares them all
    near = flag_margins(out)
    print(f"{int(near.sum())} of {near.size} (robot, tick, leg) within 1e-9 of a flag threshold; smallest margin {out['margin'].min():.3e}")
    assert near.sum() == 0 and np.isfinite(out["margin"]).all()
    # a poisoned input that never enters the state (a held foot, with base_acc given) still poisons the swing through its landing row
    s = parabola_logs(5, B=2)
    bad = dict(s, feet_log=s["feet_log"].copy()); bad["feet_log"][1, 3, 2, 0] = np.nan
    o1, o2 = track(s), track(bad)
    hit = np.zeros(o1["flag"].shape, bool); hit[1, 3:7, 2] = True
    assert np.array_equal(o2["flag"] == 0xff, hit) and np.isnan(o2["err"][hit]).all() and np.array_equal(o2["tau"][~hit], o1["tau"][~hit])
    pushed = rows["pushed"]
    worst = lambda m: float(out["err"][m][landed[m]].max())
    print(f"landing miss: {int(landed.sum())} landings, unpushed worst {worst(~pushed) * 1e3:.3f} mm, pushed worst {worst(pushed) * 1e3:.3f} mm")
    assert pushed.sum() == 2 and worst(pushed) > 0.0 and worst(~pushed) > 0.0


# -------------------------------------------------------------------------------------------------------------------- 8. split rows
def test_two_pieces_through_state_are_one_call(oracle_lib):
    pb, rows, o, swing = _loop()
    a = (o["actual"], o["forces"], o["feet_log"], o["contact_log"], swing)
    whole = lite3_model.swing_track_host(*a, body=rows["body"], delta=DELTA)
    for cut in (9, 14):
        first = lite3_model.swing_track_host(*[x[:, :cut] for x in a], body=rows["body"], delta=DELTA)
        second = lite3_model.swing_track_host(*[x[:, cut:] for x in a], body=rows["body"], state=first["state"], delta=DELTA)
        for k in lite3_model.SWING_OUT:
            assert np.array_equal(np.concatenate([first[k], second[k]], axis=1), whole[k], equal_nan=True), (cut, k)
        assert np.array_equal(second["state"], whole["state"], equal_nan=True)
    assert whole["state"][:, :, 6].any() and not whole["state"][:, :, 6].all()     # the cut-off row is mid-swing for some legs


# ------------------------------------------------------------------------------------------- 9. the growth factor of the serial state
def measure_growth():
    """The growth factor of the end-to-end case over the CPU checker's logs of it (the device test multiplies its one-row band by it)."""
    pb, rows, o, swing = _loop()
    return growth_factor(o, swing, rows["body"])


def test_growth_factor_is_the_recorded_one(oracle_lib):
    g = measure_growth()
    rec = float(np.load(GROWTH_NPZ)["growth"])
    print(f"growth of a 1e-10 perturbation of the initial state over {ROLL_T} rows: {g:.3f} (recorded {rec:.3f})")
    assert g < 1e3 and abs(g - rec) <= 1e-3 * rec


if __name__ == "__main__":                                                      # regenerate tests/golden/swing_track_growth.npz
    g = measure_growth()
    np.savez(GROWTH_NPZ, growth=np.float64(g), rows=np.int64(ROLL_T), eps=np.float64(1e-10))
    print("growth", g)
