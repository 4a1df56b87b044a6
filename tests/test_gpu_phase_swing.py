"""Swing-foot trajectories of the roll-out on a gait clock on the device (include/mpcqp_plan.h, mpcqp_phase_swing) against the host
counterpart mpcqp.gaits.phase_swing_host: synthetic logs on every named gait and on hostile gait rows, with poisoned rows; the logs
of one real roll-out, whose swing feet then go through mpcqp_joint_rates; the argument checks; determinism."""
import numpy as np
import pytest

import mpcqp
from mpcqp import gaits, lite3_model, synth

NAMES = tuple(gaits.GAITS)
DELTA = 0.03
STEP_HEIGHT = 0.06          # (tests/test_phase_swing_host.py: every swing foot of an unpushed robot stays in reach on the CPU checker's loop)


def _t(a, dt):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


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
    """(error, band): f64 |dev - host| / max(1, |host|) against 1e-12, f32 float32 spacings against 2; the NaN pattern must match."""
    if io == "f32":
        return _ulps32(dev, host), 2.0
    nan = np.isnan(host)
    assert np.array_equal(nan, np.isnan(dev))
    err = np.abs(dev[~nan] - host[~nan]) / np.maximum(1.0, np.abs(host[~nan]))
    return (float(err.max()) if err.size else 0.0), 1e-12


def _solver(io):
    return mpcqp.MPCBatch(N=10, delta=DELTA, io_dtype=io, precision="mixed")


FLOATS = ("actual", "desired", "feet_log", "stand", "gain", "step_height")


def _device_swing(sol, p, gain=True, des=True):
    import torch
    dt = sol.tdtype
    d = {k: _t(p[k], dt) for k in FLOATS}
    out = sol.phase_swing(d, _t(p["gait"], torch.int32), _t(p["tick0"], torch.int32), d["stand"], d["gain"] if gain else None,
                          d["step_height"], want_des=des)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def _host_swing(p, gain=True):
    return gaits.phase_swing_host(p["actual"], p["desired"], p["feet_log"], p["gait"], p["tick0"], p["stand"], p["gain"] if gain else None,
                                  p["step_height"], DELTA)


# ----------------------------------------------------------------------------------------------------------- 1. synthetic logs
B_SYN, T_SYN = 64, 26
POISON = {"stand": (5, 2, 1), "gain": (9,), "step_height": (13,), "feet_log": (17, 3, 2, 0), "actual": (21, 4, 10)}


def _synthetic_logs():
    """52 robots on the eight named gaits (periods 12 and 9, start ticks 0 .. 30) and 12 on hostile gait rows and ticks (the table of
    tests/test_gpu_gaits.py: P <= 0, P = 1, offsets and stances out of range, ticks at both ends of int32), over T = 26 log rows of
    random torso states, references and held feet."""
    big = 2 ** 31 - 1
    hostile = np.array([[0, 5, -1, 7, 0, 3, 0, 1, 9], [-7, 1, 2, 3, 4, -5, 0, 1, 2], [1, 0, 0, 0, 0, 1, 0, 1, 0],   # P <= 0, P = 1
                        [10, -1, -10, -13, 25, 11, -3, 10, 0], [70000, 65536, -65536, 1, 2, 70000, 65535, 1, 2],
                        [7, big, -big - 1, big - 3, 0, 3, 3, 3, 3], [6, 0, 0, 2, 3, 6, 0, 3, 3], [12, 0, 6, 6, 0, 12, 12, 0, 0],
                        [9, 1, 2, 3, 4, 4, 4, 4, 4], [9, 1, 2, 3, 4, 4, 4, 4, 4], [65535, 65534, 0, 1, 2, 30000, 30000, 7, 7],
                        [8, 0, 4, 4, 0, 5, 5, 5, 5]])
    htick = np.array([3, 0, 11, 4, 12345, big, 1, 5, -4, big - 3, big - 2, -big - 1])
    B, T, H = B_SYN, T_SYN, len(hostile)
    rng = np.random.default_rng(20251018)
    named = gaits.gait_rows([NAMES[b % 8] for b in range(B - H)], np.where(np.arange(B - H) < 32, 12, 9))
    gait = np.concatenate([named.astype(np.int64), hostile]).astype(np.int32)
    tick0 = np.concatenate([rng.integers(0, 31, B - H), htick]).astype(np.int32)
    tick0[3] = -7                                                                # a negative start tick on a named gait
    actual = np.concatenate([rng.normal(0.0, 0.1, (B, T, 3)), rng.normal(0.0, 0.3, (B, T, 2)), rng.normal(synth.H_COM, 0.01, (B, T, 1)),
                             rng.normal(0.0, 0.5, (B, T, 3)), rng.normal(0.0, 0.3, (B, T, 3))], axis=2)
    desired = rng.normal(0.0, 0.3, (B, T, 12))
    stand = np.concatenate([synth.NOMINAL_FEET[None, :, :2] + rng.normal(0.0, 0.01, (B, 4, 2)), rng.normal(0.02, 0.01, (B, 4, 1))], axis=2)
    feet_log = actual[:, :, None, 3:6] * [1.0, 1.0, 0.0] + stand[:, None] + rng.normal(0.0, 0.02, (B, T, 4, 3))
    return {"actual": actual, "desired": desired, "feet_log": feet_log, "gait": gait, "tick0": tick0, "stand": stand,
            "gain": rng.uniform(0.0, 0.1, B), "step_height": rng.uniform(0.03, 0.1, B)}


def _poisoned(p):
    bad = {k: (v.copy() if k in POISON else v) for k, v in p.items()}
    for k, at in POISON.items():
        bad[k][at] = np.inf if k == "gain" else np.nan
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_synthetic_logs_match_the_host(io):
    p = _synthetic_logs()
    if io == "f32":
        p = {k: (_r32(v) if k in FLOATS else v) for k, v in p.items()}
    sol = _solver(io)
    dev, host = _device_swing(sol, p), _host_swing(p)
    nog, hnog = _device_swing(sol, p, gain=False, des=False), _host_swing(p, gain=False)
    _, _, st = gaits.clamp_gait(p["gait"])
    tick = np.minimum(np.maximum(p["tick0"].astype(np.int64)[:, None] + np.arange(T_SYN)[None, :], 0), 2 ** 31 - 1)
    down = gaits.phase(p["gait"], tick) < st[:, None, :]
    assert down.any() and not down.all()
    assert np.array_equal(gaits.phase(p["gait"], tick)[3, :8], np.repeat(gaits.phase(p["gait"], tick)[3, :1], 8, axis=0))   # the clock held at 0
    for what, d, h in (("gain", dev, host), ("no gain", nog, hnog)):
        err, band = _error(d["swing"], h["swing"], io)
        print(f"synthetic {io} {what}: swing err {err:.3e} band {band:.3e}; max |vel| {np.abs(h['swing'][:, :, :, 1]).max():.2f}, "
              f"max |acc| {np.abs(h['swing'][:, :, :, 2]).max():.1f}")
        assert err <= band, (what, err)
        assert not np.isnan(d["swing"]).any()
    assert nog["feet_des"] is None and np.array_equal(dev["feet_des"], dev["swing"][:, :, :, 0])
    assert not np.array_equal(dev["swing"], nog["swing"])
    # stance legs and legs without touchdowns: the log row itself, at rest
    fl = p["feet_log"].astype(dev["swing"].dtype)
    P, _, _ = gaits.clamp_gait(p["gait"])
    still = down | ~((st > 0) & (st < P[:, None]))[:, None, :]
    assert np.array_equal(dev["swing"][:, :, :, 0][still], fl[still]) and np.array_equal(dev["swing"][:, :, :, 3][still], fl[still])
    assert not dev["swing"][:, :, :, 1:3][still].any() and (~still).sum() > B_SYN * T_SYN // 2
    assert np.abs(dev["swing"][:, :, :, 1][~still]).max() > 0.1
    # poisoned rows: the same NaN pattern as the host, nobody else changes
    bad = _poisoned(p)
    dbad, hbad = _device_swing(sol, bad), _host_swing(bad)
    err, band = _error(dbad["swing"], hbad["swing"], io)
    assert err <= band
    nan = np.isnan(dbad["swing"])
    want = np.zeros((B_SYN, T_SYN, 4), bool)
    want[5] = want[9] = want[13] = True                    # stand, gain, step_height: the robot
    want[17, 3, 2] = True                                  # a foot: its leg
    want[21, 4] = True                                     # a state entry: the row
    assert np.array_equal(nan, np.broadcast_to(want[..., None, None], nan.shape)) and np.array_equal(np.isnan(dbad["feet_des"]), nan[:, :, :, 0])
    assert np.array_equal(dbad["swing"][~want], dev["swing"][~want]) and np.array_equal(dbad["feet_des"][~want], dev["feet_des"][~want])


@pytest.mark.gpu
def test_two_calls_give_the_same_bits():
    p = _synthetic_logs()
    sol = _solver("f64")
    a, b = _device_swing(sol, p), _device_swing(_solver("f64"), p)
    assert np.array_equal(a["swing"], b["swing"]) and np.array_equal(a["feet_des"], b["feet_des"])


# ------------------------------------------------------------------------------------------------------------ 2. one real roll-out
B_RUN, T_RUN = 24, 25


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_swing_of_a_real_rollout_and_its_joint_rates(io):
    """rollout_phase on the device (eight gaits, period 12, pushes on half of the robots), phase_swing on its logs against the host on
    the same logs, then joint_rates on feet_des and the swing velocities: every swing foot of an unpushed robot is in reach."""
    import torch
    B, T = B_RUN, T_RUN
    pb = gaits.make_phase_batch(B, NAMES, 12, seed=6)
    rows = synth.make_plant_rows(B, seed=6, push_start=(3, 15))                    # (this seed pushes half of them)
    assert rows["pushed"].sum() == B // 2
    if io == "f32":
        pb = {k: (_r32(v) if k in ("x", "ref", "feet", "stand", "gain", "mu") else v) for k, v in pb.items()}
        rows = {k: (_r32(v) if k in ("body", "push") else v) for k, v in rows.items()}
    sol = _solver(io)
    dt = sol.tdtype
    tick = _t(pb["tick"], torch.int32)
    tick0 = tick.clone()                                                         # the roll-out advances `tick` in place
    gait, stand, gain = _t(pb["gait"], torch.int32), _t(pb["stand"], dt), _t(pb["gain"], dt)
    logs = sol.rollout_phase(_t(pb["x"], dt), _t(pb["ref"], dt), _t(pb["feet"], dt), gait, stand, gain, tick, _t(pb["mu"], dt), T,
                             body=_t(rows["body"], dt), push=_t(rows["push"], dt), push_ticks=_t(rows["push_ticks"], torch.int32))
    hh = _t(np.full(B, STEP_HEIGHT), dt)
    sw = sol.phase_swing(logs, gait, tick0, stand, gain, hh)
    vel = sw["swing"][:, :, :, 1].contiguous()
    jr = sol.joint_rates(logs["actual"], logs["forces"], sw["feet_des"], vel)
    torch.cuda.synchronize()
    print(f"roll-out {io}: solved ticks per robot {int(logs['solved'].min())} .. {int(logs['solved'].max())} of {T}")
    assert bool((tick == T).all()) and not bool(tick0.any())
    lg = {k: logs[k].cpu().numpy().astype(np.float64) for k in ("actual", "desired", "feet_log", "forces")}
    host = gaits.phase_swing_host(lg["actual"], lg["desired"], lg["feet_log"], pb["gait"], pb["tick"], pb["stand"], pb["gain"],
                                  np.full(B, float(hh[0])), DELTA)
    got = sw["swing"].cpu().numpy()
    err, band = _error(got, host["swing"], io)
    print(f"roll-out {io}: swing err {err:.3e} band {band:.3e}")
    assert err <= band
    cl = logs["contact_log"].cpu().numpy()
    up = cl == 0
    assert up.any() and np.array_equal(got[:, :, :, 0][~up], logs["feet_log"].cpu().numpy()[~up]) and not got[:, :, :, 1:3][~up].any()
    assert np.array_equal(sw["feet_des"].cpu().numpy(), got[:, :, :, 0]) and np.abs(got[:, :, :, 1][up]).max() > 0.1
    reach, qd, power = (jr[k].cpu().numpy() for k in ("reach", "qd", "power"))
    calm = ~rows["pushed"]
    assert up[calm].sum() > 100 and np.all(reach[calm][up[calm]] == 1)
    _, qdh, _, ph, rh = lite3_model.joint_rates_host(lg["actual"], lg["forces"], host["feet_des"], host["swing"][:, :, :, 1])
    assert np.all(rh[calm] == 1)
    print(f"roll-out {io}: swing-leg max |qd| {np.abs(qd[up]).max():.2f} rad/s, mean joint power per robot "
          f"{power.astype(np.float64).sum(axis=2).mean():.2f} W (host {ph.sum(axis=2).mean():.2f} W)")
    assert np.abs(qd[up]).max() > 1.0


# ------------------------------------------------------------------------------------------------------------ 3. argument checks
@pytest.mark.gpu
def test_argument_checks():
    import torch
    sol = _solver("f64")
    eng = sol.engine
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    a = buf.data_ptr()
    # phase_swing_ptr(B, T, actual, desired, feet_log, gait, tick0, stand, gain, step_height, swing, feet_des)
    good = [a, a, a, a, a, a, 0, a, a, 0]
    for i in (0, 1, 2, 3, 4, 5, 7, 8):                                          # every required buffer (gain and feet_des are optional)
        args = list(good); args[i] = 0
        with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_phase_swing: null buffer"):
            eng.phase_swing_ptr(1, 1, *args)
    for B, T in ((-1, 1), (1, -1), (2 ** 31, 1), (2 ** 20, 2 ** 12)):
        with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_phase_swing: size out of range"):
            eng.phase_swing_ptr(B, T, *good)
    eng.phase_swing_ptr(0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)                       # B = 0 and T = 0: no-ops, nothing is read or written
    eng.phase_swing_ptr(5, 0, *good)
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0
    p = {k: v[:4, :3] if k in ("actual", "desired", "feet_log") else v[:4] for k, v in _synthetic_logs().items()}
    d = {k: _t(p[k], sol.tdtype) for k in FLOATS}
    with pytest.raises(ValueError, match="tick0"):
        sol.phase_swing(d, _t(p["gait"], torch.int32), _t(p["tick0"], torch.int64), d["stand"], d["gain"], d["step_height"])
    with pytest.raises(ValueError, match="feet_log"):
        sol.phase_swing(dict(d, feet_log=d["feet_log"].view(4, 3, 12)), _t(p["gait"], torch.int32), _t(p["tick0"], torch.int32), d["stand"],
                        d["gain"], d["step_height"])
    empty = {k: d[k][:, :0].contiguous() for k in ("actual", "desired", "feet_log")}
    out = sol.phase_swing(empty, _t(p["gait"], torch.int32), _t(p["tick0"], torch.int32), d["stand"], None, d["step_height"])
    assert tuple(out["swing"].shape) == (4, 0, 4, 4, 3) and tuple(out["feet_des"].shape) == (4, 0, 4, 3)
