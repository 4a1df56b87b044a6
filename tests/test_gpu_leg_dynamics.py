"""Leg dynamics on the device (include/mpcqp_joints.h, mpcqp_leg_dynamics / mpcqp_leg_effort) against the host counterparts
lite3_model.leg_dynamics_host / leg_effort_host: rows with known accelerations, massless legs against mpcqp_joint_rates bit for bit,
a real roll-out on the eight named gaits, the NULL-output combinations, the argument and inertia-row checks and the poisoned rows.

Bands are those of tests/test_gpu_joint_rates.py, for the same reason -- identical fp64 arithmetic on identical inputs: 1e-9 against
max(1, |host|) for fp64 I/O, 2 float32 spacings against the host value rounded once for fp32 I/O."""
import itertools
import re

import numpy as np
import pytest

import mpcqp
from dynamics_cases import known_effort_logs
from mpcqp import gaits, lite3_model, synth

B, T = 32, 4            # 128 rows
OUT = ("qdd", "tau_dyn", "tau", "power", "limit")
FLOAT_OUT = OUT[:4]
DELTA, STEP_HEIGHT = 0.03, 0.06


def _t(a, dt):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _ulps32(dev, host64):
    """fp32 device values against the fp64 host values rounded once, in float32 spacings (floor 2^-20); NaN must match NaN."""
    ref = np.asarray(host64, np.float64).astype(np.float32)
    dev = np.asarray(dev)
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(dev))
    sp = np.spacing(np.maximum(np.abs(ref[~nan]), np.float32(2.0 ** -20)))
    err = np.abs(dev[~nan].astype(np.float64) - ref[~nan].astype(np.float64)) / sp
    return float(err.max()) if err.size else 0.0


def _error(dev, host, io):
    """(error, band): f64 |dev - host| / max(1, |host|) against 1e-9, f32 float32 spacings against 2; the NaN pattern must match."""
    if io == "f32":
        return _ulps32(dev, host), 2.0
    nan = np.isnan(host)
    assert np.array_equal(nan, np.isnan(dev))
    err = np.abs(dev[~nan] - host[~nan]) / np.maximum(1.0, np.abs(host[~nan]))
    return (float(err.max()) if err.size else 0.0), 1e-9


def _logs(io):
    """The rows with known accelerations, with one leg's foot out of reach and one robot-tick's feet far away."""
    s = known_effort_logs(B, T)
    s.pop("min_det")
    s["feet"][3, 1, 2, 2] -= 0.5
    s["feet"][7, 2] += [0.0, 0.0, 2.0]
    s["body"] = synth.make_plant_rows(B, seed=3)["body"]
    if io == "f32":
        s = {k: _r32(v) for k, v in s.items()}
    return s


IN = ("actual", "forces", "feet", "foot_vel", "foot_acc", "base_acc", "body")


# ------------------------------------------------------------------------------------------------- 1. leg_dynamics against the host
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_leg_dynamics_against_the_host(io):
    import torch
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(41)
    n = B * T // 4 + 1                                                          # 33 rows, 132 legs: not a multiple of anything
    q = np.stack([rng.uniform(-0.5, 0.5, (n, 4)), rng.uniform(-1.5, -0.2, (n, 4)), rng.uniform(0.5, 2.3, (n, 4))], axis=-1)
    ops = {"qd": rng.uniform(-3.0, 3.0, (n, 4, 3)), "qdd": rng.uniform(-40.0, 40.0, (n, 4, 3)),
           "rot": Rotation.from_rotvec(rng.normal(0.0, 0.15, (n, 3))).as_matrix(),
           "base": np.concatenate([rng.normal(0.0, 1.0, (n, 3)), rng.normal(0.0, 3.0, (n, 3)), rng.normal(0.0, 2.0, (n, 3))], axis=-1)}
    if io == "f32":
        q, ops = _r32(q), {k: _r32(v) for k, v in ops.items()}
    sol = mpcqp.MPCBatch(io_dtype=io)
    dt = sol.tdtype
    variants = [()] + [(k,) for k in ops] + [tuple(ops)]                         # all given, each one left out, all left out
    for drop in variants:
        use = {k: (None if k in drop else v) for k, v in ops.items()}
        out = sol.leg_dynamics(_t(q, dt), **{k: _t(v, dt) for k, v in use.items()})
        torch.cuda.synchronize()
        host = dict(zip(("tau", "mass", "bias"), lite3_model.leg_dynamics_host(q, **use)))
        for k in ("tau", "mass", "bias"):
            err, band = _error(out[k].cpu().numpy(), host[k], io)
            print(f"leg_dynamics {io} without {drop or 'nothing'} {k}: err {err:.3e} band {band:.1e} (max |{k}| {np.abs(host[k]).max():.3f})")
            assert err <= band, (drop, k, err)
    only = sol.leg_dynamics(_t(q, dt), want=("mass",))
    torch.cuda.synchronize()
    assert only["tau"] is None and only["bias"] is None and torch.equal(only["mass"], out["mass"])


# -------------------------------------------------------------------------------------------------- 2. leg_effort against the host
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_leg_effort_against_the_host(io):
    import torch
    s = _logs(io)
    sol = mpcqp.MPCBatch(io_dtype=io)
    dt = sol.tdtype
    d = {k: _t(s[k], dt) for k in IN}
    for what, drop in (("all operands", ()), ("base_acc = None", ("base_acc",)), ("only the required", IN[3:])):
        dev = sol.leg_effort(*[None if k in drop else d[k] for k in IN])
        torch.cuda.synchronize()
        host = lite3_model.leg_effort_host(*[None if k in drop else s[k] for k in IN])
        got = {k: dev[k].cpu().numpy() for k in OUT}
        assert np.array_equal(got["limit"], host["limit"]), what
        assert got["limit"][3, 1, 2] & 8 and np.all(got["limit"][7, 2] & 8) and (got["limit"] & 8).sum() == 8 * 5
        assert not got["qdd"][3, 1, 2].any() and not got["qdd"][7, 2].any() and np.abs(got["tau_dyn"][7, 2]).max(axis=-1).min() > 0.0
        for k in FLOAT_OUT:
            err, band = _error(got[k], host[k], io)
            print(f"leg_effort {io} {what} {k}: err {err:.3e} band {band:.1e} (max |{k}| {np.abs(host[k]).max():.2f})")
            assert err <= band, (what, k, err)
        if not drop and io == "f64":
            ok = host["reach"] == 1
            print(f"leg_effort f64: recovered qdd against the rows' own: {np.abs(got['qdd'] - s['qdd'])[ok].max():.3e} rad/s^2")
            assert np.abs(got["qdd"] - s["qdd"])[ok].max() <= 7.1e-5            # the band of tests/test_leg_dynamics_host.py


# --------------------------------------------------------------------------------------------- 3. massless legs reproduce the parent
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_massless_legs_are_joint_rates(io):
    """With an inertia row of all-zero masses and inertias tau and power are mpcqp_joint_rates' under torch.equal and tau_dyn is all
    zero: both kernels inline the same leg_joints<true, true>, and csrc/mpcqp_legdyn.h says what it takes for the compiler to fuse its
    multiply-adds the same way in both (with the inertial row as one 1064-byte kernel argument 307 of 1536 fp64 torques were off
    by up to 4 units in the last place)."""
    import torch
    s = _logs(io)
    sol = mpcqp.MPCBatch(io_dtype=io)
    d = {k: _t(s[k], sol.tdtype) for k in IN}
    none = lite3_model.leg_inertia()
    for k in ("mass", "com", "inertia"):
        none[k] = np.zeros_like(none[k])
    jr = sol.joint_rates(d["actual"], d["forces"], d["feet"], d["foot_vel"])
    light = {}
    for drop in ((), ("base_acc",)):
        out = light[drop] = sol.leg_effort(*[None if k in drop else d[k] for k in IN], inertia=none)
        torch.cuda.synchronize()
        assert torch.equal(out["tau"], jr["tau"]) and torch.equal(out["power"], jr["power"])
        assert not bool(out["tau_dyn"].any()) and not bool(torch.isnan(out["qdd"]).any())
    full = sol.leg_effort(*[d[k] for k in IN])
    torch.cuda.synchronize()
    assert not torch.equal(full["tau"], jr["tau"]) and torch.equal(full["qdd"], light[()]["qdd"])    # (qdd is kinematics: no mass in it)


# ------------------------------------------------------------------------------------------------------- 4. end to end on the device
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_effort_of_a_real_rollout(io):
    """rollout_phase on the device (16 robots on the eight named gaits, period 12, unpushed, per-robot bodies), phase_swing on its logs,
    leg_effort on feet_des with the swing velocities and accelerations and base_acc = None, against the host on the device's logs."""
    import torch
    Br, Tr = 16, 25
    pb = gaits.make_phase_batch(Br, tuple(gaits.GAITS), 12, seed=6)
    body = synth.make_plant_rows(Br, seed=6)["body"]
    if io == "f32":
        pb = {k: (_r32(v) if k in ("x", "ref", "feet", "stand", "gain", "mu") else v) for k, v in pb.items()}
        body = _r32(body)
    sol = mpcqp.MPCBatch(N=10, delta=DELTA, io_dtype=io, precision="mixed")
    dt = sol.tdtype
    tick = _t(pb["tick"], torch.int32)
    tick0 = tick.clone()
    gait, stand, gain, bd = _t(pb["gait"], torch.int32), _t(pb["stand"], dt), _t(pb["gain"], dt), _t(body, dt)
    logs = sol.rollout_phase(_t(pb["x"], dt), _t(pb["ref"], dt), _t(pb["feet"], dt), gait, stand, gain, tick, _t(pb["mu"], dt), Tr, body=bd)
    sw = sol.phase_swing(logs, gait, tick0, stand, gain, _t(np.full(Br, STEP_HEIGHT), dt))
    vel, acc = sw["swing"][:, :, :, 1].contiguous(), sw["swing"][:, :, :, 2].contiguous()
    out = sol.leg_effort(logs["actual"], logs["forces"], sw["feet_des"], vel, acc, None, bd)
    torch.cuda.synchronize()
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    host = lite3_model.leg_effort_host(f64(logs["actual"]), f64(logs["forces"]), f64(sw["feet_des"]), f64(vel), f64(acc), None, body)
    got = {k: out[k].cpu().numpy() for k in OUT}
    assert np.array_equal(got["limit"], host["limit"])
    for k in FLOAT_OUT:
        err, band = _error(got[k], host[k], io)
        print(f"roll-out {io} {k}: err {err:.3e} band {band:.1e} (max |{k}| {np.abs(host[k]).max():.2f})")
        assert err <= band, (k, err)
    up = logs["contact_log"].cpu().numpy() == 0
    assert up.sum() > 100 and np.all(np.abs(got["tau_dyn"][up]).max(axis=-1) > 0.0)      # every swing leg's dynamic torque
    assert np.array_equal(got["tau"][up], got["tau_dyn"][up])                            # ... is its whole torque: its ground torque is a zero
    flagged = (got["limit"] != 0).any(axis=-1)
    print(f"roll-out {io}: swing legs peak |tau_dyn| {np.abs(got['tau_dyn'][up]).max(axis=0)} N m, stance legs peak |tau| "
          f"{np.abs(got['tau'][~up]).max(axis=0)} N m, robot-ticks with a limit bit {flagged.sum()} of {flagged.size}")


# --------------------------------------------------------------------------------------------------- 5. NULL and argument handling
@pytest.mark.gpu
def test_null_outputs_arguments_and_poisoned_rows():
    import torch
    s = _logs("f64")
    sol = mpcqp.MPCBatch(io_dtype="f64")
    eng = sol.engine
    dt = sol.tdtype
    d = {k: _t(s[k], dt) for k in IN}
    out = sol.leg_effort(*[d[k] for k in IN])
    torch.cuda.synchronize()
    ins = tuple(d[k].data_ptr() for k in IN)
    # every non-empty subset of the five outputs: what is asked for is what the full call gives, what is not is not written
    for keep in itertools.product((False, True), repeat=5):
        bufs = [torch.full_like(out[k], 7) for k in OUT]
        ptrs = [b.data_ptr() if on else 0 for b, on in zip(bufs, keep)]
        if not any(keep):
            with pytest.raises(mpcqp.MpcQpError, match=r"-1.*no output"):
                eng.leg_effort_ptr(B, T, *ins, *ptrs)
            continue
        eng.leg_effort_ptr(B, T, *ins, *ptrs)
        torch.cuda.synchronize()
        for b, on, k in zip(bufs, keep, OUT):
            assert torch.equal(b, out[k]) if on else bool((b == 7).all()), (keep, k)
    o = out["tau"].data_ptr()
    for i in range(3):                                                          # actual, forces, feet are required
        args = list(ins); args[i] = 0
        with pytest.raises(mpcqp.MpcQpError, match=r"-1.*mpcqp_leg_effort: null buffer"):
            eng.leg_effort_ptr(B, T, *args, 0, 0, o, 0, 0)
    for bad in ((B, -1), (-1, T), (2 ** 20, 2 ** 10), (2 ** 31, 1)):
        with pytest.raises(mpcqp.MpcQpError, match=r"-1.*size"):
            eng.leg_effort_ptr(*bad, *ins, 0, 0, o, 0, 0)
    eng.leg_effort_ptr(B, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, o, 0, 0)                # no ticks, no robots: no-ops
    eng.leg_effort_ptr(0, T, 0, 0, 0, 0, 0, 0, 0, 0, 0, o, 0, 0)
    qp = d["foot_vel"].data_ptr()                                               # (any [B T,4,3] buffer serves as q here)
    with pytest.raises(mpcqp.MpcQpError, match=r"-1.*no output"):
        eng.leg_dynamics_ptr(B * T, qp, 0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(mpcqp.MpcQpError, match=r"-1.*null q"):
        eng.leg_dynamics_ptr(B * T, 0, 0, 0, 0, 0, o, 0, 0)
    for bad in (-1, 2 ** 29):
        with pytest.raises(mpcqp.MpcQpError, match=r"-1.*batch size"):
            eng.leg_dynamics_ptr(bad, qp, 0, 0, 0, 0, o, 0, 0)
    eng.leg_dynamics_ptr(0, 0, 0, 0, 0, 0, o, 0, 0)
    with pytest.raises(ValueError, match="foot_acc"):
        sol.leg_effort(d["actual"], d["forces"], d["feet"], d["foot_vel"], d["foot_acc"].view(B, T, 12))
    with pytest.raises(ValueError, match="base"):
        sol.leg_dynamics(d["foot_vel"].view(B * T, 4, 3), base=d["base_acc"].view(B * T, 6))
    # every invalid field of the inertia row, by its name, from both calls
    good = lite3_model.leg_inertia()
    cases = []
    for k in ("mass", "com", "inertia", "q_min", "q_max", "qd_max", "tau_max"):
        r = {f: np.array(v, dtype=float, copy=True) if f != "gravity" else v for f, v in good.items()}
        r[k].flat[-1] = np.nan
        cases.append((r, f"{k} is not finite"))
    for k, v, msg in (("mass", -0.1, "mass is negative"), ("q_min", 3.0, "q_min > q_max"), ("qd_max", -1.0, "qd_max is negative"),
                      ("tau_max", -1.0, "tau_max is negative")):
        r = {f: np.array(x, dtype=float, copy=True) if f != "gravity" else x for f, x in good.items()}
        r[k].flat[1] = v
        cases.append((r, msg))
    for g in (0.0, 9.81, np.inf, np.nan):
        cases.append((dict(good, gravity=g), "gravity is not negative and finite"))
    for r, msg in cases:
        row = mpcqp._capi.MpcQpLegInertia.from_dict(r)
        with pytest.raises(mpcqp.MpcQpError, match=rf"-1: mpcqp_leg_effort: invalid leg inertia row: {re.escape(msg)}"):
            eng.leg_effort_ptr(B, T, *ins, 0, 0, o, 0, 0, inertia=row)
        with pytest.raises(mpcqp.MpcQpError, match=rf"-1: mpcqp_leg_dynamics: invalid leg inertia row: {re.escape(msg)}"):
            eng.leg_dynamics_ptr(B * T, qp, 0, 0, 0, 0, o, 0, 0, inertia=row)
    short = mpcqp._capi.MpcQpLegInertia.from_dict(good); short.size = 8
    with pytest.raises(mpcqp.MpcQpError, match=r"inertia struct size mismatch"):
        eng.leg_effort_ptr(B, T, *ins, 0, 0, o, 0, 0, inertia=short)
    # poisoned rows.  With base_acc given a leg reads its own row of actual and base_acc and its own force, foot, velocity and
    # acceleration: a NaN foot poisons its leg, a NaN omega or base_acc row the four legs of its row.
    foot = s["feet"].copy(); foot[2, 1, 3, 0] = np.nan
    act = s["actual"].copy(); act[5, 2, 7] = np.nan
    bacc = s["base_acc"].copy(); bacc[9, 1, 4] = np.nan
    o2 = sol.leg_effort(_t(act, dt), d["forces"], _t(foot, dt), d["foot_vel"], d["foot_acc"], _t(bacc, dt), d["body"])
    torch.cuda.synchronize()
    hit = np.zeros((B, T, 4), bool); hit[2, 1, 3] = True; hit[5, 2] = True; hit[9, 1] = True
    m = torch.as_tensor(hit).cuda()
    for k in FLOAT_OUT:
        assert bool(torch.isnan(o2[k][m]).all()) and torch.equal(o2[k][~m], out[k][~m]), k
    assert bool((o2["limit"][m] == 0xff).all()) and torch.equal(o2["limit"][~m], out["limit"][~m])
    # with base_acc = None the row's right-hand side reads the robot's body row: an invalid one poisons every tick of that robot
    body = s["body"].copy(); body[4, 2] = np.nan
    clean = sol.leg_effort(d["actual"], d["forces"], d["feet"], d["foot_vel"], d["foot_acc"], None, d["body"])
    o3 = sol.leg_effort(d["actual"], d["forces"], d["feet"], d["foot_vel"], d["foot_acc"], None, _t(body, dt))
    o4 = sol.leg_effort(d["actual"], d["forces"], d["feet"], d["foot_vel"], d["foot_acc"], d["base_acc"], _t(body, dt))
    torch.cuda.synchronize()
    hit = np.zeros((B, T, 4), bool); hit[4] = True
    m = torch.as_tensor(hit).cuda()
    for k in FLOAT_OUT:
        assert bool(torch.isnan(o3[k][m]).all()) and torch.equal(o3[k][~m], clean[k][~m]), k
        assert torch.equal(o4[k], out[k]), k                                      # (body is not read when base_acc is given)
    assert bool((o3["limit"][m] == 0xff).all()) and torch.equal(o3["limit"][~m], clean["limit"][~m])


# ------------------------------------------------------------------------------------------------------------- 6. the extension gate
def test_the_checker_library_names_the_missing_header(oracle_lib):
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    for call in (lambda: eng.leg_dynamics_ptr(1, 0, 0, 0, 0, 0, 0, 0, 0), lambda: eng.leg_effort_ptr(1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)):
        with pytest.raises(mpcqp.MpcQpError, match=rf"{re.escape(oracle_lib.path)} does not export include/mpcqp_joints.h \(product library only\)"):
            call()
    with pytest.raises(mpcqp.MpcQpError, match=r"mpcqp_default_leg_inertia: .* does not export include/mpcqp_joints.h \(product library only\)"):
        oracle_lib.default_leg_inertia()
