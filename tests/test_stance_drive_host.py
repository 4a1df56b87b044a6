"""The stance drive on the host (lite3_model.stance_drive_host, gaits.rollout_drive_host; include/mpcqp_sim.h, mpcqp_stance_drive /
mpcqp_rollout_drive), no GPU: the rule case by case, and the closed loop of the eight named gaits on the CPU checker at the Lite3's
actuators, at tau_max halved and on slippery ground.  The loop's counts and heights are printed; profiles/r18_drive.txt and the
documents quote them.  The tests assert directions, not those values."""
import os
import re

import numpy as np
import pytest

import drive_cases as dc
import mpcqp
from conftest import REPO
from legsim_cases import DELTA
from mpcqp import gaits, lite3_model, synth

TAU_MAX = lite3_model.leg_inertia()["tau_max"]


def _same(a, b):
    return np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind == "f")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _stand(B=1, fz=None):
    """B robots in the nominal stance under the stand forces m g / 4."""
    x = np.zeros((B, 13))
    x[:, 5], x[:, 12] = synth.H_COM, synth.G_ACC
    feet = np.tile(np.concatenate([synth.NOMINAL_FEET[:, :2], np.full((4, 1), synth.FOOT_Z)], axis=1), (B, 1, 1))
    f = np.zeros((B, 4, 3))
    f[..., 2] = 8.885 * 9.81 / 4.0 if fz is None else fz
    return x, f, feet, np.ones((B, 4), np.uint8)


# ---------------------------------------------------------------------------------------------------------------------- 1. identity
def test_nominal_stance_is_left_alone():
    x, f, feet, contact = _stand()
    for ground in (None, np.array([0.5])):
        o = lite3_model.stance_drive_host(x, f, feet, contact, ground)
        assert np.array_equal(_bits(o["f"]), _bits(f.reshape(1, 12))) and not o["flag"].any()
        tau = lite3_model.joint_log_host(x[:, None, :12], f.reshape(1, 1, 12), feet[:, None])[1][:, 0]
        assert np.array_equal(_bits(o["tau"]), _bits(tau)) and np.abs(tau).max() < TAU_MAX.min()
    # a swing leg keeps its force bit for bit, whatever it is, and has no torque
    contact[0, 2] = 0
    f[0, 2] = [3.0, -np.inf, -5.0]
    o = lite3_model.stance_drive_host(x, f, feet, contact, np.array([0.1]))
    assert np.array_equal(_bits(o["f"]), _bits(f.reshape(1, 12))) and not o["flag"].any() and not o["tau"][0, 2].any()
    with pytest.raises(ValueError, match="drive must be"):
        lite3_model.stance_drive_host(x, f, feet, contact, drive="strong")


# ------------------------------------------------------------------------------------------------------------------------- 2. clamp
def test_clamp_on_the_joint_box():
    c = dc.clamp_draw(ground=False)
    assert np.abs(c["f"]).max() <= dc.F_MAX and np.linalg.norm(c["x"][0, :3]) < 1e-6
    o = dc.drive(c)
    st = c["contact"] != 0
    clamped = (o["flag"] & 2) != 0
    share = clamped[st].mean()
    print(f"clamp draw: scale {c['scale']:.1f} N, {int(st.sum())} stance legs, {int(clamped[st].sum())} clamped ({share:.0%}), "
          f"{int(((o['flag'] & 32) != 0).sum())} pulling, {int(((o['flag'] & 4) != 0).sum())} outside q limits")
    assert 0.3 <= share <= 0.7 and not clamped[~st].any() and not np.any(o["flag"] == 0xff) and not np.any(o["flag"] & 16)
    tau, tc = o["tau"], o["tau_cmd"]
    pulled = (o["flag"] & 32) != 0
    # (without a friction row bit 32 means a pull: commanded, or what the clamped torques amount to)
    assert pulled[st].sum() >= 5 and np.all(np.asarray(c["f"]).reshape(-1, 4, 3)[pulled & ~clamped][:, 2] <= 0.0)
    keep = st & ~pulled                                                          # a pulling leg's torque is that of no force
    assert np.all(np.abs(tau[keep]) <= TAU_MAX)
    inside = np.abs(tc) <= TAU_MAX
    assert np.array_equal(_bits(tau[keep][inside[keep]]), _bits(tc[keep][inside[keep]]))   # unclamped joints keep tau_cmd
    assert np.all(np.abs(tau[keep][~inside[keep]]) == np.broadcast_to(TAU_MAX, tau[keep].shape)[~inside[keep]])
    # legs that were not clamped and do not pull keep their force bit for bit
    fr, fo = c["f"].reshape(-1, 4, 3), o["f"].reshape(-1, 4, 3)
    free = ~clamped & ~pulled
    assert np.array_equal(_bits(fo[free]), _bits(fr[free]))
    # the applied force reproduces the applied torque
    back = lite3_model.joint_log_host(c["x"][:, None, :12], o["f"][:, None], c["feet"][:, None])[1][:, 0]
    err = np.abs(back - tau)[keep & clamped].max()
    print(f"(R J)^T (-f_out) against tau_app on the clamped legs: {err:.2e}")
    assert err <= dc.F64_BAND
    # ideal: the clamp is skipped
    ideal = dc.drive(c, drive="ideal")
    ip = (ideal["flag"] & 32) != 0
    assert not np.any(ideal["flag"] & 2) and np.array_equal(ip, st & (fr[..., 2] <= 0.0))
    assert np.array_equal(_bits(ideal["f"].reshape(-1, 4, 3)[~ip]), _bits(fr[~ip])) and not ideal["f"].reshape(-1, 4, 3)[ip].any()


def test_the_draw_keeps_clear_of_the_thresholds():
    """The condition of the device comparison: at most MARGIN_SHARE of the legs within FLAG_MARGIN of a deciding threshold, in both
    I/O dtypes, and the float32 operands decide every flag as the float64 ones do."""
    c = dc.clamp_draw()
    h64, h32 = dc.drive(c), dc.drive(dc.as_io(c, np.float32))
    for h in (h64, h32):
        near = dc.near_threshold(h)
        print(f"{int(near.sum())} of {near.size} legs near a threshold, smallest margin {h['margin'].min():.2e}")
        assert near.mean() <= dc.MARGIN_SHARE
    assert np.array_equal(h64["flag"], h32["flag"])
    st = c["contact"] != 0
    assert ((h64["flag"] & 32) != 0)[st].sum() >= 20 and ((h64["flag"] & 2) != 0)[st].sum() >= 20 and (~st).sum() >= 10


# ------------------------------------------------------------------------------------------------------------------------ 3. ground
def test_ground():
    x, f, feet, contact = _stand(6)
    f[0, :, 2] = [-3.0, 0.0, -0.0, -1e-300]; f[0, :, 0] = [1.0, 2.0, 0.0, 0.0]                  # cannot pull
    f[1, :, 0] = [20.0, -12.0, 0.0, 3.0]; f[1, :, 1] = [-15.0, 9.0, 8.0, 4.0]                  # outside / inside the cone
    f[2] = f[1]
    mu = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5])
    o = lite3_model.stance_drive_host(x, f, feet, contact, mu)
    fo = o["f"].reshape(6, 4, 3)
    # f_z <= 0: exact zeros and bit 32 -- except where the force was zero already, which is left alone, its sign of zero included
    assert not fo[0].any() and list(o["flag"][0] & 32) == [32, 32, 0, 32]
    assert np.array_equal(_bits(fo[0, 2]), _bits(f[0, 2])) and np.array_equal(_bits(fo[0, 0]), _bits(np.zeros(3)))
    assert not o["tau"][0].any()
    # outside the cone: |f_t| = mu f_z, direction and f_z kept
    fz = f[1, :, 2]
    ft = np.hypot(f[1, :, 0], f[1, :, 1])
    out = ft > 0.5 * fz
    assert list(out) == [True, True, False, False] and list(o["flag"][1] & 32) == [32, 32, 0, 0]
    ft2 = np.hypot(fo[1, :, 0], fo[1, :, 1])
    assert np.abs(ft2[out] - 0.5 * fz[out]).max() <= 1e-13 and np.array_equal(_bits(fo[1, :, 2]), _bits(fz))
    cross = fo[1, :, 0] * f[1, :, 1] - fo[1, :, 1] * f[1, :, 0]
    assert np.abs(cross[out]).max() <= 1e-12 and np.all((fo[1, :, :2] * f[1, :, :2]).sum(axis=-1)[out] > 0)
    # inside: untouched bits
    assert np.array_equal(_bits(fo[1][~out]), _bits(f[1][~out]))
    # the torque of a limited leg is that of the limited force
    back = lite3_model.joint_log_host(x[:, None, :12], o["f"][:, None], feet[:, None])[1][:, 0]
    assert np.abs(back - o["tau"])[1].max() <= 1e-12
    # ground = None skips only the cone
    n = lite3_model.stance_drive_host(x, f, feet, contact, None)
    fn = n["f"].reshape(6, 4, 3)
    assert np.array_equal(_bits(fn[1:]), _bits(f[1:])) and not n["flag"][1:].any()
    assert np.array_equal(_bits(fn[0]), _bits(fo[0])) and np.array_equal(n["flag"][0], o["flag"][0])
    # mu_g = 0: ice, only the normal force goes through
    ice = lite3_model.stance_drive_host(x, f, feet, contact, np.zeros(6))["f"].reshape(6, 4, 3)
    assert not ice[1, :, :2].any() and np.array_equal(ice[1, :, 2], fz)


# ------------------------------------------------------------------------------------------------------------------ 4. poisoned rows
def test_bad_rows_poison_their_own_robot_only():
    c = dc.clamp_draw()
    clean = dc.drive(c)
    bad = {k: (None if v is None else np.array(v, copy=True)) for k, v in c.items()}
    bad["x"][3, 4] = np.nan                       # the robot's state
    bad["ground"][5] = np.inf                     # its ground row
    bad["ground"][7] = -0.25                      # a negative friction coefficient
    stance9 = int(np.nonzero(c["contact"][9])[0][0])
    stance11 = int(np.nonzero(c["contact"][11])[0][0])
    bad["f"].reshape(-1, 4, 3)[9, stance9, 1] = np.nan       # one leg's force
    bad["feet"][11, stance11, 0] = np.inf                    # one leg's foot
    o = dc.drive(bad)
    fo, fc = o["f"].reshape(-1, 4, 3), clean["f"].reshape(-1, 4, 3)
    for b in (3, 5, 7):
        assert np.all(o["flag"][b] == 0xff) and np.isnan(fo[b]).all() and np.isnan(o["tau"][b]).all()
    for b, l in ((9, stance9), (11, stance11)):
        assert o["flag"][b, l] == 0xff and np.isnan(fo[b, l]).all() and np.isnan(o["tau"][b, l]).all()
        rest = [k for k in range(4) if k != l]
        assert _same(fo[b, rest], fc[b, rest]) and _same(o["tau"][b, rest], clean["tau"][b, rest]) and _same(o["flag"][b, rest], clean["flag"][b, rest])
    others = [b for b in range(33) if b not in (3, 5, 7, 9, 11)]
    for k in ("f", "tau", "flag"):
        assert _same(o[k][others], clean[k][others]), k


# ---------------------------------------------------------------------------------------------------------------- 5. out of reach
def test_an_out_of_reach_clamped_leg_keeps_its_force():
    x, f, feet, contact = _stand(2)
    feet[0, 1, 2] -= 0.5                           # 0.77 m below the hip: beyond l1 + l2 = 0.41 m
    f[:, :, 0], f[:, :, 2] = 100.0, 140.0
    o = lite3_model.stance_drive_host(x, f, feet, contact)
    assert o["reach"][0, 1] == 0 and o["flag"][0, 1] & 18 == 18
    assert np.array_equal(_bits(o["f"].reshape(2, 4, 3)[0, 1]), _bits(f[0, 1])) and np.all(np.abs(o["tau"][0, 1]) <= TAU_MAX)
    others = np.ones((2, 4), bool); others[0, 1] = False
    assert not np.any(o["flag"][others] & 16) and np.all(o["reach"][others] == 1)


# ----------------------------------------------------------------------------------------------------------------- 6. closed loop
@pytest.fixture(scope="module")
def loops(oracle_lib):
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config(N=10, delta=DELTA, max_iter=4000))
    pb = dc.loop_batch()
    return pb, {"legs": dc.run_loop(eng, pb, drive=None), "lite3": dc.run_loop(eng, pb, drive="limited"),
                "half": dc.run_loop(eng, pb, drive="limited", inertia=dc.weak_row(0.5)),
                "ground": dc.run_loop(eng, pb, drive="limited", ground=np.full(dc.LOOP_B, dc.GROUND_MU))}


def _stance_rows(o, bit):
    return (((o["flag"] & bit) != 0) & (o["flag"] != 0xff) & (o["contact_log"] != 0)).sum(axis=(1, 2))


def test_the_lite3s_actuators_do_not_limit_any_named_gait(loops):
    pb, r = loops
    legs, lite3 = r["legs"], r["lite3"]
    for k in legs:
        assert _same(legs[k], lite3[k]), k
    assert _same(lite3["cmd"], lite3["forces"]) and not _stance_rows(lite3, 2).any() and not _stance_rows(lite3, 32).any()
    st = lite3["contact_log"] != 0
    for b, name in enumerate(pb["names"]):
        print(f"{name:12s} largest stance torque {np.round(np.abs(lite3['tau'][b][st[b]]).max(axis=0), 1)} N m")
    assert np.all(np.abs(lite3["tau"][st]) <= TAU_MAX)
    with pytest.raises(ValueError, match="drive must be"):
        dc.run_loop(None, pb, drive="weak")


def test_halved_actuators_limit_bound_and_gallop(loops):
    pb, r = loops
    half, lite3 = r["half"], r["lite3"]
    rows = dict(zip(pb["names"], _stance_rows(half, 2)))
    low = {n: (lite3["actual"][b, :, 5].min(), half["actual"][b, :, 5].min()) for b, n in enumerate(pb["names"])}
    for n in pb["names"]:
        print(f"tau_max x 0.5: {n:12s} {int(rows[n]):3d} clamped stance leg-rows, lowest CoM {low[n][0]:.3f} -> {low[n][1]:.3f} m")
    assert rows["bound"] > 0 and rows["gallop"] > 0 and rows["trot"] == 0 and rows["walk"] == 0
    assert np.all(half["solved"] == dc.LOOP_T) and np.isfinite(half["x"]).all()
    assert low["gallop"][1] < low["gallop"][0]
    # the plant received what the legs could deliver: the clamped rows' forces differ from the commanded ones, the others' do not
    cl = ((half["flag"] & 2) != 0) & (half["contact_log"] != 0)
    fo, fc = half["forces"].reshape(dc.LOOP_B, dc.LOOP_T, 4, 3), half["cmd"].reshape(dc.LOOP_B, dc.LOOP_T, 4, 3)
    assert np.all((fo != fc).any(axis=-1)[cl]) and _same(fo[~cl & ((half["flag"] & 32) == 0)], fc[~cl & ((half["flag"] & 32) == 0)])
    assert np.all(np.abs(half["tau"][(half["contact_log"] != 0) & ((half["flag"] & 32) == 0)]) <= 0.5 * TAU_MAX)


def test_slippery_ground_limits_every_gait(loops):
    pb, r = loops
    o = r["ground"]
    rows = dict(zip(pb["names"], _stance_rows(o, 32)))
    st = o["contact_log"] != 0
    f = o["forces"].reshape(dc.LOOP_B, dc.LOOP_T, 4, 3)
    up = st & (f[..., 2] > 0.0)
    use = np.hypot(f[..., 0], f[..., 1])[up] / f[..., 2][up]
    for n in pb["names"]:
        print(f"ground {dc.GROUND_MU}: {n:12s} {int(rows[n]):3d} ground-limited stance leg-rows")
    print(f"largest friction use of the applied stance forces: {use.max():.15f}")
    assert all(rows[n] > 0 for n in pb["names"] if n != "stand")
    # "to rounding": a quotient, two products, a square root of a sum of squares and a quotient lie between mu_g and this figure
    assert use.max() <= dc.GROUND_MU * (1.0 + 8 * np.finfo(float).eps) and np.all(f[..., 2][st] >= 0.0)
    assert np.all(o["solved"] == dc.LOOP_T)
    fc = o["cmd"].reshape(f.shape)
    usec = np.hypot(fc[..., 0], fc[..., 1])[up] / np.maximum(fc[..., 2][up], 1e-300)
    assert usec.max() > 0.45                                                    # the controllers believe 0.5 to 1.0 and use it


# ------------------------------------------------------------------------------------------------------------------ 7. symbol set
def test_sim_header_declares_the_drive_product_only(oracle_lib):
    capi = mpcqp._capi
    hdr = open(os.path.join(REPO, "include", "mpcqp_sim.h")).read()
    syms = set(re.findall(r"^\s*int\s+(mpcqp_[a-z_]+)\s*\(", hdr, re.M))
    assert syms == set(capi.SIM_SYMBOLS) and capi.DRIVE_SYMBOLS == ("mpcqp_stance_drive", "mpcqp_rollout_drive")
    assert set(capi.DRIVE_SYMBOLS) <= set(capi.SIM_SYMBOLS)
    assert re.search(r"#define MPCQP_DRIVE_IDEAL 0\b", hdr) and re.search(r"#define MPCQP_DRIVE_LIMITED 1\b", hdr)
    assert (capi.DRIVE_IDEAL, capi.DRIVE_LIMITED) == (0, 1)
    plib = mpcqp.product_library()
    assert plib.has_sim and plib.has_legroll and plib.has_score and plib.has_drive and plib.version() == 0x00010301
    assert all(plib.calls[s][0] is not None for s in capi.DRIVE_SYMBOLS)
    assert not oracle_lib.has_drive and not oracle_lib.has_sim and not any(hasattr(oracle_lib.lib, s) for s in capi.DRIVE_SYMBOLS)
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    for call in (lambda: eng.stance_drive_ptr(1, 1, 1, 1, 1, 0, 1),
                 lambda: eng.rollout_drive_ptr(*([1, 1] + [1] * 9 + [0, 0, 0] + [10, 1, 0, 0, 0, 1, 0] + [0] * 15))):
        with pytest.raises(mpcqp.MpcQpError, match=r"does not export include/mpcqp_sim.h \(product library only\)"):
            call()
