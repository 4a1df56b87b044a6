"""Stance feet that slide, on the host (lite3_model.stance_slip_host / foot_mass, gaits.rollout_slip_host; include/mpcqp_slip.h,
mpcqp_stance_slip / mpcqp_rollout_slip), no GPU: the rule case by case on a robot in its nominal stance, the closed loop of the eight
named gaits on the CPU checker at high friction -- where it is rollout_drive_host bit for bit -- and on slippery ground, the margin share
of the draw the GPU comparison uses, and the binding's gate.  The loop's counts are printed; DESIGN.md quotes them.

The foot-move identity is asserted in its exact form, feet_log[t + 1].xy == feet_log[t].xy + disp[t]: the difference of two rounded
positions is not the displacement bit for bit, the sum is."""
import os
import re

import numpy as np
import pytest

import drive_cases as dc
import legsim_cases
import mpcqp
import slip_cases as sc
from conftest import REPO
from legsim_cases import DELTA
from mpcqp import gaits, lite3_model, score, synth

ME = 0.25
N_SUB = 10
H = DELTA / N_SUB
W4 = 8.885 * 9.81 / 4.0            # a quarter of the weight: the stand force of one leg


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _stand(fxy=(0.0, 0.0), fz=W4):
    """One robot in the nominal stance, every leg commanded (fxy, fz)."""
    x = np.zeros((1, 13))
    x[:, 5], x[:, 12] = synth.H_COM, synth.G_ACC
    feet = np.concatenate([synth.NOMINAL_FEET[:, :2], np.full((4, 1), synth.FOOT_Z)], axis=1)[None]
    f = np.zeros((1, 4, 3))
    f[..., 0], f[..., 1], f[..., 2] = fxy[0], fxy[1], fz
    return x, f, feet, np.ones((1, 4), np.uint8)


def _rule(x, f, feet, contact, mu, slip=None, me=ME, **kw):
    slip = np.zeros((1, 4, 2)) if slip is None else slip
    return lite3_model.stance_slip_host(x, f, feet, contact, np.array([mu]), np.array([me]), slip, delta=DELTA, **kw)


def _by_hand(fx, fy, fz, mu, s0, me=ME):
    """The rule of include/mpcqp_slip.h on Python floats, for a leg whose actuators do not clamp (f1 = f)."""
    fn = max(fz, 0.0)
    hm = H / me
    cap, vx, vy = (mu * fn) * hm, -fx * hm, -fy * hm
    sx, sy, dx, dy = s0[0], s0[1], 0.0, 0.0
    for _ in range(N_SUB):
        tx, ty = sx + vx, sy + vy
        nrm = (tx * tx + ty * ty) ** 0.5
        if nrm <= cap:
            sx, sy = 0.0, 0.0
        else:
            keep = 1.0 - cap / nrm
            sx, sy = tx * keep, ty * keep
        dx, dy = dx + H * sx, dy + H * sy
    sliding = s0[0] != 0.0 or s0[1] != 0.0 or sx != 0.0 or sy != 0.0
    if fz <= 0.0:
        f2 = (0.0, 0.0, 0.0)
    elif sliding:
        f2 = (fx + (me / DELTA) * (sx - s0[0]), fy + (me / DELTA) * (sy - s0[1]), fz)
    else:
        f2 = (fx, fy, fz)
    return (sx, sy), (dx, dy), f2, sliding


# ------------------------------------------------------------------------------------------------------ 1. the rule, case by case
def test_a_foot_at_rest_inside_the_cone_never_moves():
    x, f, feet, contact = _stand((5.0, -3.0))                                   # |f_xy| = 5.83 < 0.5 f_z = 10.9
    f[0, 1, 0] = -0.0                                                           # a -0 is kept too
    o = _rule(x, f, feet, contact, 0.5)
    assert np.array_equal(_bits(o["f"]), _bits(f.reshape(1, 12))) and not o["flag"].any()
    assert not o["slip"].any() and not o["disp"].any()
    tau = lite3_model.joint_log_host(x[:, None, :12], f.reshape(1, 1, 12), feet[:, None])[1][:, 0]
    assert np.array_equal(_bits(o["tau"]), _bits(tau))
    # and it is the drive's answer, key by key
    d = lite3_model.stance_drive_host(x, f, feet, contact, np.array([0.5]))
    for k in ("f", "tau", "flag", "tau_cmd", "q", "reach"):
        assert np.array_equal(o[k], d[k]), k


def test_a_foot_just_outside_the_cone_slides_against_the_force():
    mu = 0.3
    fx, fy = 0.6 * mu * W4 * 1.02, 0.8 * mu * W4 * 1.02                          # 2 % outside the cone
    x, f, feet, contact = _stand((fx, fy))
    o = _rule(x, f, feet, contact, mu)
    s, d, f2, sliding = _by_hand(fx, fy, W4, mu, (0.0, 0.0))
    assert sliding and np.all(o["flag"] == (32 | 128))
    for l in range(4):
        assert tuple(o["slip"][0, l]) == s and tuple(o["disp"][0, l]) == d and tuple(o["f"].reshape(4, 3)[l]) == f2
    # along -f1_xy: antiparallel to the commanded tangential force, and the ground returned |f2_xy| = mu f_z to rounding
    s, d = np.array(s), np.array(d)
    assert s @ np.array([fx, fy]) < 0.0 and abs(s[0] * fy - s[1] * fx) <= 1e-15 * np.hypot(fx, fy) * np.linalg.norm(s)
    assert d @ np.array([fx, fy]) < 0.0
    assert abs(np.hypot(f2[0], f2[1]) - mu * W4) <= 1e-12 * mu * W4
    # just inside: at rest, no bit
    x, f, feet, contact = _stand((fx / 1.05, fy / 1.05))
    o = _rule(x, f, feet, contact, mu)
    assert not o["flag"].any() and not o["slip"].any() and np.array_equal(_bits(o["f"]), _bits(f.reshape(1, 12)))


def test_a_moving_foot_with_no_drive_stops_and_sticks_exactly():
    mu, s0 = 0.3, (0.09, -0.12)                                                 # 0.15 m/s; stops within |s0| m_e / (mu f_n) = 5.7 ms
    x, f, feet, contact = _stand()
    slip = np.zeros((1, 4, 2))
    slip[0, 2] = s0
    o = _rule(x, f, feet, contact, mu, slip)
    t_stop = np.hypot(*s0) * ME / (mu * W4)
    assert t_stop < DELTA
    s, d, f2, sliding = _by_hand(0.0, 0.0, W4, mu, s0)
    assert s == (0.0, 0.0) and sliding
    assert o["slip"][0, 2, 0] == 0.0 and o["slip"][0, 2, 1] == 0.0 and tuple(o["disp"][0, 2]) == d
    assert o["flag"][0, 2] == (32 | 128) and not o["flag"][0, [0, 1, 3]].any()
    # it slid along s0, no further than it would at constant deceleration plus one substep of travel
    dist = np.hypot(*d)
    assert d[0] * s0[0] + d[1] * s0[1] > 0.0 and dist <= 0.5 * np.hypot(*s0) * t_stop + np.hypot(*s0) * H
    # momentum: m_e (s_end - s0) = delta (f2_xy - f1_xy), to a few ulps of the larger side
    fo = o["f"].reshape(4, 3)[2]
    for a in range(2):
        lhs, rhs = ME * (o["slip"][0, 2, a] - s0[a]), DELTA * (fo[a] - f[0, 2, a])
        assert abs(lhs - rhs) <= 4 * np.spacing(max(abs(lhs), abs(rhs)))
    # the next tick: at rest, nothing left
    o2 = _rule(x, f, feet, contact, mu, o["slip"])
    assert not o2["flag"].any() and not o2["disp"].any()


def test_momentum_holds_on_a_driven_sliding_foot():
    mu, s0 = 0.2, (-0.3, 0.4)
    x, f, feet, contact = _stand((7.0, 2.0))
    slip = np.tile(np.array(s0), (1, 4, 1))
    o = _rule(x, f, feet, contact, mu, slip, me=0.4)
    s, d, f2, sliding = _by_hand(7.0, 2.0, W4, mu, s0, me=0.4)
    fo = o["f"].reshape(4, 3)
    for l in range(4):
        assert tuple(o["slip"][0, l]) == s and tuple(o["disp"][0, l]) == d and tuple(fo[l]) == f2 and fo[l, 2] == W4
        for a in range(2):
            lhs, rhs = 0.4 * (o["slip"][0, l, a] - s0[a]), DELTA * (fo[l, a] - f[0, l, a])
            assert abs(lhs - rhs) <= 4 * np.spacing(max(abs(lhs), abs(rhs)))
    assert np.all(o["flag"] == (32 | 128))


def test_a_pull_mu_zero_and_a_swing_leg():
    # a pull: no force, and the foot coasts under drv with cap = 0
    x, f, feet, contact = _stand((4.0, 0.0), fz=-10.0)
    o = _rule(x, f, feet, contact, 0.8)
    s, d, f2, sliding = _by_hand(4.0, 0.0, -10.0, 0.8, (0.0, 0.0))
    assert not o["f"].any() and np.all(o["flag"] == (32 | 128)) and f2 == (0.0, 0.0, 0.0)
    assert tuple(o["slip"][0, 0]) == s and abs(s[0] + N_SUB * 4.0 * H / ME) <= 1e-15 and tuple(o["disp"][0, 0]) == d and d[0] < 0.0
    # mu_g = 0: nothing is returned; the foot takes the whole tangential force as acceleration
    x, f, feet, contact = _stand((1.0, -2.0))
    o = _rule(x, f, feet, contact, 0.0)
    fo = o["f"].reshape(4, 3)
    assert np.all(o["flag"] == (32 | 128)) and np.all(fo[:, 2] == W4) and np.abs(fo[:, :2]).max() <= 1e-13
    assert np.all(o["slip"][0, :, 0] < 0.0) and np.all(o["slip"][0, :, 1] > 0.0)
    # mu_g = 0 under a force with no tangential part: at rest, untouched
    x, f, feet, contact = _stand()
    o = _rule(x, f, feet, contact, 0.0)
    assert not o["flag"].any() and np.array_equal(_bits(o["f"]), _bits(f.reshape(1, 12)))
    # a swing leg: force kept bit for bit whatever it and its slip entry are, s = d = 0
    contact[0, 1] = 0
    f[0, 1] = [3.0, -np.inf, -5.0]
    slip = np.zeros((1, 4, 2))
    slip[0, 1] = [0.5, np.nan]
    o = _rule(x, f, feet, contact, 0.1, slip)
    assert np.array_equal(_bits(o["f"]), _bits(f.reshape(1, 12))) and not o["flag"].any() and not o["tau"][0, 1].any()
    assert not o["slip"].any() and not o["disp"].any()
    with pytest.raises(ValueError, match="drive must be"):
        _rule(x, f, feet, contact, 0.1, drive="strong")
    with pytest.raises(ValueError, match="substeps must be"):
        _rule(x, f, feet, contact, 0.1, substeps=1001)


def test_every_poison_kind_stays_with_its_robot_or_leg():
    c = sc.slip_draw()
    good = sc.slip(c)
    assert not np.any(good["flag"] == 0xff)
    B = c["x"].shape[0]
    robots = {"x": 3, "ground nan": 5, "ground negative": 7, "foot_mass nan": 9, "foot_mass zero": 11, "foot_mass negative": 13,
              "foot_mass inf": 15}
    bad = {k: np.array(v, copy=True) for k, v in c.items() if k != "scale"}
    bad["x"][3, 1] = np.nan
    bad["ground"][5], bad["ground"][7] = np.nan, -0.5
    bad["foot_mass"][9], bad["foot_mass"][11], bad["foot_mass"][13], bad["foot_mass"][15] = np.nan, 0.0, -0.2, np.inf
    legs = {}
    for b, what in ((17, "slip"), (19, "f"), (21, "feet")):
        l = int(np.nonzero(c["contact"][b])[0][0])
        legs[(b, l)] = what
        if what == "slip":
            bad["slip"][b, l, 1] = np.inf
        elif what == "f":
            bad["f"][b, 3 * l + 2] = np.nan
        else:
            bad["feet"][b, l, 0] = np.nan
    o = sc.slip(bad)
    others = np.ones((B, 4), bool)
    for b in robots.values():
        others[b] = False
        assert np.all(o["flag"][b] == 0xff), b
        for k in ("tau", "slip", "disp"):
            assert np.isnan(o[k][b]).all(), (b, k)
        assert np.isnan(o["f"][b]).all()
    for (b, l), what in legs.items():
        others[b, l] = False
        assert o["flag"][b, l] == 0xff and np.isnan(o["tau"][b, l]).all() and np.isnan(o["slip"][b, l]).all() and np.isnan(o["disp"][b, l]).all(), what
        assert np.isnan(o["f"][b, 3 * l:3 * l + 3]).all()
    for k in ("tau", "flag", "slip", "disp"):
        assert np.array_equal(o[k][others], good[k][others]), k
    assert np.array_equal(o["f"].reshape(B, 4, 3)[others], good["f"].reshape(B, 4, 3)[others])


def test_actuator_rates_are_those_of_the_moving_foot():
    """With a table the envelope is read at the joint rates of a foot moving at s0; at s0 = 0 they are the drive's."""
    from mpcqp import actuators
    c = sc.slip_draw()
    B = c["x"].shape[0]
    rows = np.tile(np.concatenate([lite3_model.leg_inertia()["tau_max"], [4.0, 4.0, 3.0], [9.0, 9.0, 7.0]]), (B, 1))
    rest = dict(c, slip=np.zeros_like(c["slip"]))
    o0, d0 = sc.slip(rest, actuators=rows), dc.drive(c, actuators=rows)
    assert np.array_equal(o0["rate"], d0["rate"]) and np.array_equal(o0["tau_cmd"], d0["tau_cmd"], equal_nan=True)
    assert np.array_equal(o0["flag"] & 2, d0["flag"] & 2)
    o1 = sc.slip(c, actuators=rows)
    moving = c["slip"].any(axis=-1) & (c["contact"] != 0)
    assert np.all((o1["rate"] != o0["rate"]).any(axis=-1)[moving & (o1["reach"] != 0)]) and np.array_equal(o1["rate"][~moving], o0["rate"][~moving])
    fv = np.concatenate([c["slip"], np.zeros((B, 4, 1))], axis=-1)
    rate = lite3_model.joint_rates_host(c["x"][:, None, :12], c["f"].reshape(B, 1, 12), c["feet"][:, None], fv[:, None])[1][:, 0]
    assert np.array_equal(o1["rate"], rate)


def test_foot_mass_of_the_lite3():
    me = lite3_model.foot_mass()
    print(f"foot_mass() = {me:.6f} kg")
    assert abs(me - 0.258) <= 1e-3
    q, _ = lite3_model.leg_ik_closed(synth.NOMINAL_FEET[None])
    M = lite3_model.leg_dynamics_host(q)[1][0]
    for l in range(4):
        J = lite3_model.leg_fk_jac(l, q[0, l])[1]
        eig = np.linalg.eigvalsh((J @ np.linalg.solve(M[l], J.T))[:2, :2])
        assert abs(eig[0] - 3.32) <= 0.01 and abs(eig[1] - 4.44) <= 0.01, (l, eig)
    heavy = lite3_model.leg_inertia()
    heavy["mass"] = heavy["mass"] * 2.0
    heavy["inertia"] = heavy["inertia"] * 2.0
    assert abs(lite3_model.foot_mass(heavy) - 2.0 * me) <= 1e-12


# ----------------------------------------------------------------------------------------------------------------- 2., 3. the loop
@pytest.fixture(scope="module")
def loops(oracle_lib):
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config(N=10, delta=DELTA, max_iter=4000))
    pb = dc.loop_batch()
    grip, ice = np.full(dc.LOOP_B, 1e3), np.full(dc.LOOP_B, sc.ICE)
    return pb, {"drive grip": dc.run_loop(eng, pb, drive="limited", ground=grip), "slip grip": sc.run_slip(eng, pb, grip),
                "drive ice": dc.run_loop(eng, pb, drive="limited", ground=ice), "slip ice": sc.run_slip(eng, pb, ice)}


def test_high_friction_is_rollout_drive_bit_for_bit(loops):
    pb, r = loops
    d, s = r["drive grip"], r["slip grip"]
    assert set(s) == set(d) | {"slip", "slip_log", "disp"}
    for k in d:
        assert np.array_equal(d[k], s[k], equal_nan=np.asarray(d[k]).dtype.kind == "f"), k
    assert not s["slip_log"].any() and not s["disp"].any() and not s["slip"].any()
    assert not ((s["flag"] & 128) != 0)[s["flag"] != 0xff].any() and np.all(s["solved"] == dc.LOOP_T)


def test_slippery_ground_moves_the_feet_and_fells_a_robot(loops):
    pb, r = loops
    d, s = r["drive ice"], r["slip ice"]
    live = s["flag"] != 0xff
    sliding = ((s["flag"] & 128) != 0) & live & (s["contact_log"] != 0)
    rows = sliding.sum(axis=(1, 2))
    dist = np.linalg.norm(s["disp"], axis=-1).sum(axis=(1, 2))
    sd, ss = score.score_host(d), score.score_host(s)
    fall = score.FIELDS.index("fall_row")
    for b, n in enumerate(pb["names"]):
        print(f"ground {sc.ICE}: {n:12s} {int(rows[b]):3d} sliding leg-rows, slid {dist[b]:7.3f} m, fall row {int(ss[b, fall]):3d} "
              f"(drive only: {int(sd[b, fall])}), solved {int(s['solved'][b])}")
    assert all(rows[b] > 0 for b, n in enumerate(pb["names"]) if n != "stand")
    assert not ((s["flag"] & 128) != 0)[live & (s["contact_log"] == 0)].any()
    assert sc.foot_move_holds(s["feet_log"], s["contact_log"], s["disp"], pb["gait"], pb["tick"])
    assert np.abs(s["disp"]).max() > 1e-3
    assert np.all(s["solved"] == dc.LOOP_T)
    assert np.all(sd[:, fall] == -1) and np.any(ss[:, fall] >= 0)
    # a replay of every row through the rule alone gives the applied forces and the displacements, and the slip state follows it: a
    # row's s0 is the previous row's s_end where the leg was down and did not touch down (a lifting leg carries its s_end into its
    # first swing row, where the rule ignores it), 0 after a swing row and at a touchdown
    B, T = dc.LOOP_B, dc.LOOP_T
    rows = lambda a: a.reshape((B * T,) + a.shape[2:])
    o = lite3_model.stance_slip_host(rows(s["actual"]), rows(s["cmd"]), rows(s["feet_log"]), rows(s["contact_log"]), np.full(B * T, sc.ICE),
                                     lite3_model.foot_mass(), rows(s["slip_log"]), delta=DELTA)
    assert np.array_equal(o["f"], rows(s["forces"])) and np.array_equal(o["disp"].reshape(B, T, 4, 2), s["disp"])
    end = o["slip"].reshape(B, T, 4, 2)
    st = s["contact_log"] != 0
    assert not end[~st].any() and not s["slip_log"][:, 0].any()
    for t in range(1, T):
        td = gaits.touchdown_mask(pb["gait"], pb["tick"] + t)
        assert not td[st[:, t - 1]].any()
        assert np.array_equal(s["slip_log"][:, t][~td], end[:, t - 1][~td]) and not s["slip_log"][:, t][td].any()


# -------------------------------------------------------------------------------------------------- 4. the GPU draw's margin share
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_draw_keeps_clear_of_the_thresholds(dtype):
    c = sc.as_io(sc.slip_draw(), dtype)
    o = sc.slip(c)
    st = c["contact"] != 0
    near = dc.near_threshold(o)
    moving = c["slip"].any(axis=-1)
    fl = o["flag"]
    print(f"{np.dtype(dtype).name}: {int(near.sum())} of {int(st.sum())} stance legs within {legsim_cases.FLAG_MARGIN:g} of a threshold; "
          f"{int(moving.sum())} moving, {int(((fl & 128) != 0).sum())} sliding, {int(((fl & 2) != 0).sum())} clamped, "
          f"{int((moving & ((fl & 128) != 0) & ~o['slip'].any(axis=-1)).sum())} stopped")
    assert near.sum() <= dc.MARGIN_SHARE * st.sum()
    assert abs(moving.sum() / st.sum() - 1.0 / 3.0) < 0.1 and not moving[~st].any() and np.linalg.norm(c["slip"], axis=-1).max() <= sc.S_MAX
    assert c["foot_mass"].min() >= sc.MASS_LO and c["foot_mass"].max() <= sc.MASS_HI
    # not vacuous: clamped legs, sliding legs that started at rest, moving feet that stuck, feet at rest that stayed
    assert ((fl & 2) != 0)[st].sum() >= 20 and (((fl & 128) != 0) & ~moving).sum() >= 5
    assert (moving & ~o["slip"].any(axis=-1)).sum() >= 3 and (st & ((fl & 128) == 0)).sum() >= 10


# ------------------------------------------------------------------------------------------------------------------- 5. the gate
def test_slip_header_is_product_only(oracle_lib):
    capi = mpcqp._capi
    hdr = open(os.path.join(REPO, "include", "mpcqp_slip.h")).read()
    syms = set(re.findall(r"^\s*int\s+(mpcqp_[a-z_]+)\s*\(", hdr, re.M))
    assert syms == set(capi.SLIP_SYMBOLS) and capi.SLIP_SYMBOLS == ("mpcqp_stance_slip", "mpcqp_rollout_slip")
    assert re.search(r"#define MPCQP_DRIVE_SLIDING 128\b", hdr) and capi.DRIVE_SLIDING == 128 == lite3_model.DRIVE_SLIDING
    assert list(capi.SLIP_ABI) == ["mpcqp_slip.h"] and "mpcqp_slip.h" not in capi.ABI
    plib = mpcqp.product_library()
    assert plib.has_slip and plib.has_actuators and plib.version() == 0x00010301
    assert all(plib.calls[s][0] is not None for s in capi.SLIP_SYMBOLS)
    assert not oracle_lib.has_slip and not any(hasattr(oracle_lib.lib, s) for s in capi.SLIP_SYMBOLS)
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    for call in (lambda: eng.stance_slip_ptr(1, 1, 1, 1, 1, 1, 1, 1, 1),
                 lambda: eng.rollout_slip_ptr(*([1, 1] + [1] * 9 + [0, 0, 0] + [10, 1, 0, 0, 0, 1, 1, 1, 1] + [0] * 17))):
        with pytest.raises(mpcqp.MpcQpError, match=r"does not export include/mpcqp_slip.h \(product library only\)"):
            call()


def test_slip_abi_table_matches_the_header():
    """The rows of SLIP_ABI against the prototypes of include/mpcqp_slip.h, as tests/test_capi.py holds the other tables."""
    import ctypes
    from test_capi import _C_INTEGER, _C_RETURN, _is_pointer_type, _prototypes
    protos = _prototypes("mpcqp_slip.h")
    table = {name: (restype, argtypes) for name, restype, argtypes in mpcqp._capi.SLIP_ABI["mpcqp_slip.h"]}
    assert set(table) == set(protos) and len(protos) == 2
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is _C_RETURN[ret] and len(argtypes) == len(params), (name, len(argtypes), len(params))
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            ctype = decl.rsplit(" ", 1)[0]
            if "*" in ctype or ctype == "mpcqp_handle":
                assert _is_pointer_type(t), (name, i, decl, t)
            else:
                assert t is _C_INTEGER[ctype], (name, i, decl, t)
    assert ctypes.c_int is _C_RETURN["int"]
