"""Per-leg periodic gaits with reactive footholds on the device (include/mpcqp_plan.h: mpcqp_phase_expand, mpcqp_solve_batch_phase;
include/mpcqp_sim.h: mpcqp_rollout_phase) against the host counterpart mpcqp.gaits: the expansion element by element, the one-call
solve against expand + solve, the roll-out against the CPU checker's closed loop, every logged robot-tick and every landing replayed
from the logs alone, the stand gait against mpcqp_rollout_plant, determinism, batch independence and the argument checks."""
import functools

import numpy as np
import pytest

import mpcqp
from conftest import ORACLE_SO
from mpcqp import gaits
from mpcqp.plant import push_wrench, srb_step

G32 = float(np.float32(-9.81))
NAMES = tuple(gaits.GAITS)          # trot, flying_trot, pace, bound, pronk, gallop, walk, stand: three of them have flight phases


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


def _solver(io, warm=False, N=10):
    return mpcqp.MPCBatch(N=N, delta=0.03, io_dtype=io, precision="mixed", warm_start=warm, warm_shift=warm)


FLOATS = ("x", "ref", "feet", "stand", "gain", "mu", "body", "push")


def _rounded(pb, io):
    return {k: (_r32(v) if io == "f32" and k in FLOATS else v) for k, v in pb.items()}


def _device_rollout(sol, pb, T, rows=None, gain=True):
    """rollout_phase on the device from a host batch (gaits.make_phase_batch layout, plus synth.make_plant_rows rows)."""
    import torch
    dt = sol.tdtype
    rows = rows or {}
    st = {k: _t(pb[k], dt) for k in ("x", "ref", "feet")}
    st["tick"] = _t(pb["tick"], torch.int32)
    opt = lambda k, d=dt: None if rows.get(k) is None else _t(rows[k], d)
    out = sol.rollout_phase(st["x"], st["ref"], st["feet"], _t(pb["gait"], torch.int32), _t(pb["stand"], dt),
                            _t(pb["gain"], dt) if gain else None, st["tick"], _t(pb["mu"], dt), T, body=opt("body"), push=opt("push"),
                            push_ticks=opt("push_ticks", torch.int32))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update({k: v.cpu().numpy() for k, v in st.items()})
    return res


# ------------------------------------------------------------------------------------------------------------- 1. the expansion
def _expand_inputs(N):
    """512 robots on make_perleg_batch timing, then hostile gait rows on copies of the first robots' state."""
    B0 = 512
    b = mpcqp.synth.make_perleg_batch(B0, N=N)
    rng = np.random.default_rng(20251018 + N)
    tm = b["timing"]
    gait = np.concatenate([tm["period"][:, None], tm["offset"], tm["stance"]], axis=1).astype(np.int64)
    tick = np.asarray(b["t0"], np.int64)
    big = 2 ** 31 - 1
    hostile = np.array([[0, 5, -1, 7, 0, 3, 0, 1, 9], [-7, 1, 2, 3, 4, -5, 0, 1, 2], [1, 0, 0, 0, 0, 1, 0, 1, 0],   # P <= 0, P = 1
                        [10, -1, -10, -13, 25, 11, -3, 10, 0], [70000, 65536, -65536, 1, 2, 70000, 65535, 1, 2],
                        [7, big, -big - 1, big - 3, 0, 3, 3, 3, 3], [6, 0, 0, 2, 3, 6, 0, 3, 3], [12, 0, 6, 6, 0, 12, 12, 0, 0],
                        [9, 1, 2, 3, 4, 4, 4, 4, 4], [9, 1, 2, 3, 4, 4, 4, 4, 4], [65535, 65534, 0, 1, 2, 30000, 30000, 7, 7],
                        [8, 0, 4, 4, 0, 5, 5, 5, 5]])
    htick = np.array([3, 0, 11, 4, 12345, big, 1, 5, -4, big - 3, big - 2, -big - 1])
    gait = np.concatenate([gait, hostile]); tick = np.concatenate([tick, htick])
    B, H = len(gait), len(hostile)
    x0 = np.concatenate([b["x0"], b["x0"][:H]])
    yaw = x0[:, 2]
    vb = rng.uniform(-0.3, 0.5, (B, 2))
    v_ref = np.stack([np.cos(yaw) * vb[:, 0] - np.sin(yaw) * vb[:, 1], np.sin(yaw) * vb[:, 0] + np.cos(yaw) * vb[:, 1], np.zeros(B)], axis=1)
    ref = np.concatenate([rng.normal(0.0, 0.05, (B, 2)), yaw[:, None] + rng.normal(0.0, 0.1, (B, 1)), x0[:, 3:5] + rng.normal(0.0, 0.02, (B, 2)),
                          np.full((B, 1), mpcqp.synth.H_COM), v_ref, rng.normal(0.0, 0.5, (B, 1))], axis=1)
    feet = np.concatenate([b["r"][:, 0], b["r"][:H, 0]]) + x0[:, None, 3:6]
    stand = np.concatenate([mpcqp.synth.NOMINAL_FEET[None, :, :2] + rng.normal(0.0, 0.01, (B, 4, 2)), rng.normal(0.02, 0.01, (B, 4, 1))], axis=2)
    return {"x": x0, "ref": ref, "feet": feet, "gait": gait.astype(np.int32), "tick": tick.astype(np.int32), "stand": stand,
            "gain": rng.uniform(0.0, 0.1, B)}


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("N", [10, 24])
def test_expand_matches_host(N, io):
    import torch
    p = _rounded(_expand_inputs(N), io)
    sol = _solver(io, N=N)
    dt = sol.tdtype
    d = {k: _t(p[k], torch.int32 if k in ("gait", "tick") else dt) for k in p}
    out = sol.phase_expand(d["x"], d["ref"], d["feet"], d["gait"], d["tick"], d["stand"], d["gain"])
    nog = sol.phase_expand(d["x"], d["ref"], d["feet"], d["gait"], d["tick"], d["stand"], None)
    torch.cuda.synchronize()
    for dev, gain in ((out, p["gain"]), (nog, None)):
        host = gaits.phase_expand_host(p["x"], p["ref"], p["feet"], p["gait"], p["tick"], p["stand"], gain, N, 0.03)
        assert np.array_equal(dev["contact"].cpu().numpy(), host["contact"])
        for k in ("r", "xdes"):
            got = dev[k].cpu().numpy()
            if io == "f64":
                err, band = np.abs(got - host[k]).max(), 1e-12 * max(1.0, np.abs(host[k]).max())
            else:
                err, band = _ulps32(got, host[k]), 2
            print(f"expand N={N} {io} gain={'yes' if gain is not None else 'no'} {k}: err {err:.3e} band {band:.3e}")
            assert err <= band, (k, err)
    ct = out["contact"].cpu().numpy()
    assert ct[:512].min() == 0 and ct[:512].max() == 1 and not torch.equal(out["r"], nog["r"])


# ------------------------------------------------------------------------------------------- 2. the one-call solve is expand + solve
@pytest.mark.gpu
@pytest.mark.parametrize("N", [10, 24])
def test_solve_batch_phase_is_expand_plus_solve(N):
    import torch
    B = 256
    p = _expand_inputs(N)
    p = {k: v[:B] for k, v in p.items()}
    mu = np.exp(np.random.default_rng(5).uniform(np.log(0.3), np.log(1.5), B))
    sol = _solver("f64", N=N)
    dt = sol.tdtype
    d = {k: _t(p[k], torch.int32 if k in ("gait", "tick") else dt) for k in p}
    mu_d = _t(mu, dt)
    one = {k: v.clone() for k, v in sol.solve_batch_phase(d["x"], d["ref"], d["feet"], d["gait"], d["tick"], d["stand"], d["gain"], mu_d,
                                                         want_X=True).items()}
    e = sol.phase_expand(d["x"], d["ref"], d["feet"], d["gait"], d["tick"], d["stand"], d["gain"])
    two = sol.solve_batch(d["x"], e["r"], e["contact"], e["xdes"], mu_d, want_X=True)
    torch.cuda.synchronize()
    for k in ("u", "X", "status", "iters", "res"):
        assert torch.equal(one[k], two[k]), k
    st = one["status"].cpu().numpy()
    assert ((st == 1) | (st == 2)).mean() > 0.5 and float(one["u"].abs().max()) > 1.0


# ----------------------------------------------------------------------------------------- 3. the roll-out against the host checker
T_HOST, B_HOST = 30, 24


@functools.lru_cache(maxsize=None)
def _host_case():
    """B = 24 robots on all eight named gaits (period 10), heterogeneous bodies, pushes on half of them, gain 0 for the first half."""
    pb = gaits.make_phase_batch(B_HOST, NAMES, 10, seed=7)
    rows = mpcqp.synth.make_plant_rows(B_HOST, seed=7, push_start=(3, 15))
    lib = mpcqp.Library(ORACLE_SO)
    eng = mpcqp.Engine(lib, lib.default_config(N=10, delta=0.03, max_iter=4000))
    ref = gaits.rollout_phase_host(eng, pb["x"], pb["ref"], pb["feet"], pb["gait"], pb["stand"], pb["gain"], pb["tick"], pb["mu"], T_HOST,
                                   rows["body"], rows["push"], rows["push_ticks"])
    return pb, rows, ref


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True])
def test_rollout_phase_matches_host_checker(warm):
    T = T_HOST
    pb, rows, ref = _host_case()
    out = _device_rollout(_solver("f64", warm), pb, T, rows)
    assert rows["pushed"].any() and (pb["gain"] == 0).sum() == B_HOST // 2 and (pb["gain"] > 0).any()
    assert np.all(out["solved"] == T) and np.all(ref["solved"] == T) and np.all(out["tick"] == T)
    assert np.array_equal(out["contact_log"], ref["contact_log"]) and (ref["contact_log"].sum(axis=2) == 0).any()   # flight ticks
    sc = max(1.0, np.abs(ref["forces"]).max())
    fb = 1e-5 * (1.0 + np.abs(pb["stand"][:, :, :2]).max() + pb["gain"].max())
    figures = {"forces": (np.abs(out["forces"] - ref["forces"]).max(), 1e-4 * sc), "actual": (np.abs(out["actual"] - ref["actual"]).max(), 1e-5),
               "desired": (np.abs(out["desired"] - ref["desired"]).max(), 1e-12), "ref": (np.abs(out["ref"] - ref["ref"]).max(), 1e-12),
               "x": (np.abs(out["x"] - ref["x"]).max(), 1e-5), "feet": (np.abs(out["feet"] - ref["feet"]).max(), fb),
               "feet_log": (np.abs(out["feet_log"] - ref["feet_log"]).max(), fb)}
    for k, (err, band) in figures.items():
        print(f"rollout_phase vs host, warm={warm}: {k} err {err:.3e} band {band:.3e}")
    for k, (err, band) in figures.items():
        assert err <= band, (k, err, band)


# --------------------------------------------------------------------------------------------------- 4. replay from the logs alone
def _tiled_case(B, period, seed, names=NAMES):
    pb = gaits.make_phase_batch(B, names, period, seed=seed)
    pb["gait"] = np.concatenate([gaits.gait_rows([NAMES[b % 8] for b in range(B // 2)], period),
                                 gaits.gait_rows([NAMES[b % 8] for b in range(B - B // 2)], period + 3)])
    rows = mpcqp.synth.make_plant_rows(B, seed=seed, push_start=(3, 18))
    return pb, rows


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_replay_every_robot_tick_and_every_landing_from_the_logs(io):
    T, B = 24, 1024
    pb, rows = _tiled_case(B, 9, 9)
    pb, rows = _rounded(pb, io), _rounded(rows, io)
    out = _device_rollout(_solver(io, warm=True), pb, T, rows)
    g = G32 if io == "f32" else -9.81
    cl, fl, act = out["contact_log"], out["feet_log"], out["actual"].astype(np.float64)
    assert np.array_equal(cl, gaits.phase_contact(pb["gait"], pb["tick"], T)) and np.array_equal(fl[:, 0], pb["feet"].astype(fl.dtype))
    worst_x = worst_f = 0.0
    landings = 0
    for t in range(T - 1):
        tick = pb["tick"] + t
        x = np.concatenate([act[:, t], np.full((B, 1), g)], axis=1)
        nxt = srb_step(x, out["forces"][:, t].astype(np.float64), fl[:, t].astype(np.float64), cl[:, t], rows["body"],
                       push_wrench(rows["push"], rows["push_ticks"], tick), 0.03, 10)
        landed = (cl[:, t + 1] == 1) & (cl[:, t] == 0)
        p = gaits.touchdown_foothold(act[:, t + 1, 3:6], gaits.measured_yaw(act[:, t + 1, 0:3]), act[:, t + 1, 9:12], pb["ref"][:, 6:9],
                                     pb["stand"], pb["gain"], pb["gait"], 0.03)
        assert np.array_equal(fl[:, t + 1][~landed], fl[:, t][~landed]), t         # every other foot: bit for bit
        landings += int(landed.sum())
        if io == "f64":
            worst_x = max(worst_x, np.abs(nxt[:, :12] - out["actual"][:, t + 1]).max())
            worst_f = max(worst_f, np.abs(fl[:, t + 1][landed] - p[landed]).max()) if landed.any() else worst_f
        else:
            worst_x = max(worst_x, _ulps32(out["actual"][:, t + 1], nxt[:, :12]))
            worst_f = max(worst_f, _ulps32(fl[:, t + 1][landed], p[landed]))
    print(f"replay {io}: plant step worst {worst_x:.3e}, landing worst {worst_f:.3e}, {landings} landings")
    band = 1e-12 if io == "f64" else 2
    assert landings > 2 * B and worst_x <= band and worst_f <= band, (worst_x, worst_f)
    # the feet state after the last tick is the last log row plus the landings of tick T
    last = gaits.touchdown_mask(pb["gait"], pb["tick"] + T)
    assert np.array_equal(out["feet"][~last], fl[:, T - 1][~last])


# --------------------------------------------------------------------------------------------- 5. stand is the existing roll-out
@pytest.mark.gpu
def test_stand_gait_is_rollout_plant_on_an_all_stance_plan():
    import torch
    T, B = 20, 256
    pb = gaits.make_phase_batch(B, "stand", 7, seed=4, v_ref=(0.0, 0.0, 0.0), theta_dot=0.0)
    pb["feet"][:, :, :2] += np.random.default_rng(4).normal(0.0, 0.02, (B, 4, 2))    # not the stand rows: those must not be read
    rows = mpcqp.synth.make_plant_rows(B, seed=4, push_start=(2, 12))
    out = _device_rollout(_solver("f64", warm=True), pb, T, rows)
    sol = _solver("f64", warm=True)
    dt = sol.tdtype
    x, rf, tk = _t(pb["x"], dt), _t(pb["ref"], dt), _t(pb["tick"], torch.int32)
    meta = np.tile(np.array([1, 4, 2, 0], np.int32), (B, 1))
    old = sol.rollout_plant(x, rf, _t(pb["feet"][:, None], dt), _t(np.ones((B, 1, 4), np.uint8), torch.uint8), _t(meta, torch.int32), tk,
                            _t(pb["mu"], dt), T, body=_t(rows["body"], dt), push=_t(rows["push"], dt),
                            push_ticks=_t(rows["push_ticks"], torch.int32))
    torch.cuda.synchronize()
    for k in ("actual", "desired", "forces", "solved"):
        assert np.array_equal(out[k], old[k].cpu().numpy()), k
    assert np.array_equal(out["x"], x.cpu().numpy()) and np.array_equal(out["ref"], rf.cpu().numpy()) and np.array_equal(out["tick"], tk.cpu().numpy())
    assert out["contact_log"].all() and np.array_equal(out["feet"], pb["feet"]) and np.array_equal(out["feet_log"], np.repeat(pb["feet"][:, None], T, axis=1))
    assert np.abs(out["forces"]).max() > 10.0 and rows["pushed"].any()


# ------------------------------------------------------------------------------------------- 6. determinism and batch independence
@pytest.mark.gpu
def test_determinism_batch_independence_and_a_nonfinite_row():
    T, B = 20, 256
    pb, rows = _tiled_case(B, 9, 5)
    pb, rows = _rounded(pb, "f32"), _rounded(rows, "f32")
    keys = ("actual", "desired", "forces", "feet_log", "contact_log", "solved", "x", "ref", "feet", "tick")
    a = _device_rollout(_solver("f32", warm=True), pb, T, rows)
    b = _device_rollout(_solver("f32", warm=True), pb, T, rows)
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    sub = slice(100, 164)
    cut = lambda d: {k: (v[sub] if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    s = _device_rollout(_solver("f32", warm=True), cut(pb), T, cut(rows))
    for k in keys:
        assert np.array_equal(s[k], a[k][sub], equal_nan=True), k
    bad = dict(pb, stand=pb["stand"].copy())
    bad["stand"][37, 2, 1] = np.nan
    c = _device_rollout(_solver("f32", warm=True), bad, T, rows)
    assert c["solved"][37] == 0 and not np.any(c["forces"][37])                   # NONFINITE from the first tick: zero forces
    keep = np.arange(B) != 37
    for k in keys:
        assert np.array_equal(c[k][keep], a[k][keep], equal_nan=True), k
    # ... and through the one-call solve the status itself
    import torch
    sol = _solver("f32")
    dt = sol.tdtype
    o = sol.solve_batch_phase(_t(bad["x"], dt), _t(bad["ref"], dt), _t(bad["feet"], dt), _t(bad["gait"], torch.int32), _t(bad["tick"], torch.int32),
                              _t(bad["stand"], dt), _t(bad["gain"], dt), _t(bad["mu"], dt))
    torch.cuda.synchronize()
    st = o["status"].cpu().numpy()
    assert st[37] == mpcqp._capi.STATUS_NONFINITE and np.all(st[keep] != mpcqp._capi.STATUS_NONFINITE)


# ------------------------------------------------------------------------------------------------------------ 7. argument checks
@pytest.mark.gpu
def test_argument_checks():
    import torch
    sol = _solver("f64")
    eng = sol.engine
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    a = buf.data_ptr()
    # rollout_phase_ptr(B, T, x, ref, feet, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, 6 logs)
    good = [a, a, a, a, a, 0, a, a]
    for bad in (-1, 1001):
        with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_rollout_phase: substeps out of range \[0, 1000\]"):
            eng.rollout_phase_ptr(1, 1, *good, 0, 0, 0, bad, 0, 0, 0, 0, 0, 0)
    with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_rollout_phase: push without push_ticks"):
        eng.rollout_phase_ptr(1, 1, *good, 0, a, 0, 10, 0, 0, 0, 0, 0, 0)
    for i in (0, 1, 2, 3, 4, 6, 7):                                             # every required buffer (gain, at 5, is optional)
        args = list(good); args[i] = 0
        with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_rollout_phase: null buffer"):
            eng.rollout_phase_ptr(1, 1, *args, 0, 0, 0, 10, 0, 0, 0, 0, 0, 0)
    for B, T in ((-1, 1), (1, -1), (2 ** 31, 1), (2 ** 20, 2 ** 12)):
        with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_rollout_phase: size out of range"):
            eng.rollout_phase_ptr(B, T, *good, 0, 0, 0, 10, 0, 0, 0, 0, 0, 0)
    eng.rollout_phase_ptr(0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 10, 0, 0, 0, 0, 0, 0)      # B = 0 and T = 0: no-ops, nothing is read or written
    eng.rollout_phase_ptr(5, 0, *good, 0, 0, 0, 10, a, a, a, a, a, a)                       # (the checks come first, as in the sibling calls)
    with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_phase_expand: null buffer"):
        eng.phase_expand_ptr(1, a, a, a, a, a, 0, 0, a, a, a)
    with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_phase_expand: batch size out of range"):
        eng.phase_expand_ptr(-1, a, a, a, a, a, a, 0, a, a, a)
    with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_solve_batch_phase: null buffer"):
        eng.solve_batch_phase_ptr(1, a, a, a, 0, a, a, 0, a, a, 0, a, a, 0)
    eng.phase_expand_ptr(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    eng.solve_batch_phase_ptr(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0
    # the Python surface: T = 0 returns empty logs and leaves the state alone; a model table of another size is refused by name
    pb = gaits.make_phase_batch(8, ("trot",), 10)
    out = _device_rollout(sol, pb, 0)
    assert out["actual"].shape == (8, 0, 12) and out["feet_log"].shape == (8, 0, 4, 3) and not out["solved"].any()
    assert np.array_equal(out["x"], pb["x"]) and np.array_equal(out["feet"], pb["feet"]) and not out["tick"].any()
    sol.set_models(mpcqp.synth.make_model_rows(4))
    with pytest.raises(mpcqp.MpcQpError, match=r"mpcqp_rollout_phase: batch size 8, but the model table has 4 rows"):
        _device_rollout(sol, pb, 2)
