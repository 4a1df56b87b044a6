"""Device rigid-body plant (include/mpcqp_sim.h): mpcqp_plant_step against the host checker plant.srb_step, mpcqp_rollout_plant
against plant.rollout_plant_host on the CPU checker, every logged robot-tick replayed through the checker, and what the closed loop
does on a plant that is not its model: mass mismatch, pushes, invalid rows."""
import numpy as np
import pytest

import mpcqp
from conftest import ORACLE_SO
from mpcqp.plant import model_body, push_wrench, rollout_plant_host, srb_step, stance_feet

G32 = float(np.float32(-9.81))


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


def _oracle():
    lib = mpcqp.Library(ORACLE_SO)
    return mpcqp.Engine(lib, lib.default_config(N=10, delta=0.03, max_iter=4000))


def _solver(io, warm=False):
    return mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed", warm_start=warm, warm_shift=warm)


def _plant_inputs(B, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 13))
    ax = rng.normal(size=(B, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    x[:, 0:3] = ax * rng.uniform(0.0, 2.5, (B, 1)) * (rng.uniform(size=(B, 1)) < 0.9)   # a tenth at theta = 0 exactly
    x[:, 3:6] = rng.normal(0.0, 0.3, (B, 3)) + [0.0, 0.0, 0.285]
    x[:, 6:9] = rng.normal(0.0, 2.0, (B, 3)); x[:, 9:12] = rng.normal(0.0, 0.5, (B, 3)); x[:, 12] = -9.81
    f = rng.normal(0.0, 10.0, (B, 12)) + np.tile([0.0, 0.0, 25.0], 4)
    feet = x[:, None, 3:6] + mpcqp.synth.NOMINAL_FEET[None] + rng.normal(0.0, 0.02, (B, 4, 3))
    contact = ((np.arange(B)[:, None] >> np.arange(4)[None]) & 1).astype(np.uint8)        # all 16 patterns
    rows = mpcqp.synth.make_plant_rows(B, seed=seed, push_frac=1.0)
    return {"x": x, "f": f, "feet": feet, "contact": contact, "body": rows["body"], "wrench": rows["push"]}


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("substeps", [1, 10, 37])
def test_plant_step_matches_host_checker(io, substeps):
    import torch
    B = 4096
    p = _plant_inputs(B, seed=substeps)
    sol = _solver(io)
    if io == "f32":
        p = {k: (_r32(v) if v.dtype == np.float64 else v) for k, v in p.items()}
    dev_in = {k: _t(v, torch.uint8 if k == "contact" else sol.tdtype) for k, v in p.items()}
    out = sol.plant_step(dev_in["x"], dev_in["f"], dev_in["feet"], dev_in["contact"], dev_in["body"], dev_in["wrench"], substeps)
    none = sol.plant_step(dev_in["x"], dev_in["f"], dev_in["feet"], dev_in["contact"], None, None, substeps)
    model = _t(model_body(sol.cfg.m, list(sol.cfg.Ibody_inv), B), sol.tdtype)
    explicit = sol.plant_step(dev_in["x"], dev_in["f"], dev_in["feet"], dev_in["contact"], model, None, substeps)
    torch.cuda.synchronize()
    host = srb_step(p["x"], p["f"], p["feet"], p["contact"], p["body"], p["wrench"], 0.03, substeps)
    dev = out.cpu().numpy()
    if io == "f64":
        assert np.abs(dev - host).max() <= 1e-12 * max(1.0, np.abs(host).max())
    else:
        assert _ulps32(dev, host) <= 2
    if io == "f64":
        assert torch.equal(none, explicit)                        # body = NULL is the model's row
    else:                                                         # (an fp32 row is the model rounded: NULL keeps it in fp64)
        host_model = srb_step(p["x"], p["f"], p["feet"], p["contact"], model_body(sol.cfg.m, list(sol.cfg.Ibody_inv), B), None, 0.03, substeps)
        assert _ulps32(none.cpu().numpy(), host_model) <= 2


def _rollout_inputs(B, seed, **rows_kw):
    rb = mpcqp.synth.make_rollout_batch(B, seed=seed)
    rows = mpcqp.synth.make_plant_rows(B, seed=seed, **rows_kw)
    return rb, rows


def _device_rollout(sol, rb, T, body=None, push=None, push_ticks=None, tick=None, substeps=10):
    import torch
    dt = sol.tdtype
    x, rf = _t(rb["x"], dt), _t(rb["ref"], dt)
    tk = _t(rb["tick"] if tick is None else tick, torch.int32)
    opt = lambda a, d=dt: None if a is None else _t(a, d)
    out = sol.rollout_plant(x, rf, _t(rb["plan_pos"], dt), _t(rb["plan_feet_id"], torch.uint8), _t(rb["plan_meta"], torch.int32), tk,
                            _t(rb["mu"], dt), T, body=opt(body), push=opt(push), push_ticks=opt(push_ticks, torch.int32),
                            substeps=substeps)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(x=x.cpu().numpy(), ref=rf.cpu().numpy(), tick=tk.cpu().numpy())
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True])
def test_rollout_plant_matches_host_checker(warm):
    T, B = 30, 24
    rb, rows = _rollout_inputs(B, 7, push_start=(3, 15))
    ref = rollout_plant_host(_oracle(), rb["x"], rb["ref"], rb["plan_pos"], rb["plan_feet_id"], rb["plan_meta"], rb["tick"], rb["mu"], T,
                             rows["body"], rows["push"], rows["push_ticks"])
    out = _device_rollout(_solver("f64", warm), rb, T, rows["body"], rows["push"], rows["push_ticks"])
    assert np.all(out["solved"] == T) and np.all(ref["solved"] == T) and np.all(out["tick"] == T)
    sc = max(1.0, np.abs(ref["forces"]).max())
    assert np.abs(out["forces"] - ref["forces"]).max() <= 1e-4 * sc
    assert np.abs(out["actual"] - ref["actual"]).max() <= 1e-5
    assert np.abs(out["desired"] - ref["desired"]).max() <= 1e-12
    assert np.abs(out["ref"] - ref["ref"]).max() <= 1e-12 and np.abs(out["x"] - ref["x"]).max() <= 1e-5


def _tiled(B0, rep, seed, **rows_kw):
    rb, rows = _rollout_inputs(B0, seed, **rows_kw)
    tile = lambda a: np.concatenate([a] * rep, axis=0)
    return {k: tile(v) if isinstance(v, np.ndarray) else v for k, v in rb.items()}, {k: tile(v) for k, v in rows.items()}


def _replay(rb, rows, out, T, io):
    """srb_step(actual[t], forces[t], ...) == actual[t + 1] for every robot and tick."""
    r = _r32 if io == "f32" else (lambda a: np.asarray(a, np.float64))
    g = G32 if io == "f32" else -9.81
    pos, body, push = r(rb["plan_pos"]), r(rows["body"]), r(rows["push"])
    worst = 0.0
    for t in range(T - 1):
        tick = rb["tick"] + t
        feet, ct = stance_feet(pos, rb["plan_feet_id"], rb["plan_meta"], tick)
        x = np.concatenate([out["actual"][:, t].astype(np.float64), np.full((len(tick), 1), g)], axis=1)
        nxt = srb_step(x, out["forces"][:, t].astype(np.float64), feet, ct, body, push_wrench(push, rows["push_ticks"], tick), 0.03, 10)
        if io == "f64":
            worst = max(worst, np.abs(nxt[:, :12] - out["actual"][:, t + 1]).max())
        else:
            worst = max(worst, _ulps32(out["actual"][:, t + 1], nxt[:, :12]))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_log_replay_every_robot_tick(io):
    """B = 4096 heterogeneous robots with pushes: every logged tick is one plant step of the logged state under the logged forces."""
    T = 30
    rb, rows = _tiled(64, 64, 9, push_start=(3, 20))
    rows = mpcqp.synth.make_plant_rows(4096, seed=9, push_start=(3, 20))
    out = _device_rollout(_solver(io, warm=True), rb, T, rows["body"], rows["push"], rows["push_ticks"])
    worst = _replay(rb, rows, out, T, io)
    assert worst <= (1e-12 if io == "f64" else 2), worst


@pytest.mark.gpu
def test_nominal_plant_tracks_and_is_not_the_model():
    """B = 2048, T = 60, f32, warm-started, body = None, no push: the closed loop on the plant tracks within the kinematic roll-out's
    bounds, and its first tick differs from the model's own prediction X[:,1] by a small amount."""
    import torch
    T = 60
    rb, _ = _tiled(32, 64, 9)
    sol = _solver("f32", warm=True)
    out = _device_rollout(sol, rb, T)
    a = out["actual"]
    print(f"nominal plant: solved {(out['solved'] == T).mean():.4f}, height err max {np.abs(a[:, :, 5] - 0.285).max():.4f}, "
          f"tilt max {np.abs(a[:, :, 0:2]).max():.4f}, mean vx dev {np.abs(a[:, 20:, 9].mean(axis=1) - 0.18).max():.4f}")
    assert (out["solved"] == T).mean() >= 0.999
    # measured on the MI355X: height error 26.1 mm, tilt 0.018 rad, mean v_x within 0.013 of 0.18
    assert np.abs(a[:, :, 5] - 0.285).max() < 0.03 and np.abs(a[:, :, 0:2]).max() < 0.03
    assert np.abs(a[:, 20:, 9].mean(axis=1) - 0.18).max() < 0.03
    kin = _solver("f32", warm=True)
    dt = kin.tdtype
    x, rf, tk = _t(rb["x"], dt), _t(rb["ref"], dt), _t(rb["tick"], torch.int32)
    k = kin.rollout(x, rf, _t(rb["plan_pos"], dt), _t(rb["plan_feet_id"], torch.uint8), _t(rb["plan_meta"], torch.int32), tk, _t(rb["mu"], dt), 2)
    torch.cuda.synchronize()
    d = np.abs(k["actual"][:, 1].cpu().numpy().astype(np.float64) - a[:, 1]).max()
    print(f"first tick: plant vs X[:,1] max diff {d:.3e}")
    assert 1e-3 < d < 1e-2                                         # measured 5.2e-3


@pytest.mark.gpu
def test_determinism_and_batch_independence():
    T = 30
    rb, rows = _tiled(64, 64, 5, push_start=(3, 20))
    sol = _solver("f32", warm=True)
    out = _device_rollout(sol, rb, T, rows["body"], rows["push"], rows["push_ticks"])
    assert np.array_equal(out["actual"][:64], out["actual"][64:128]) and np.array_equal(out["forces"][:64], out["forces"][4032:])
    one = {k: (v[5:6] if isinstance(v, np.ndarray) else v) for k, v in rb.items()}
    alone = _device_rollout(_solver("f32", warm=True), one, T, rows["body"][5:6], rows["push"][5:6], rows["push_ticks"][5:6])
    assert np.array_equal(alone["actual"][0], out["actual"][5]) and np.array_equal(alone["forces"][0], out["forces"][5])


@pytest.mark.gpu
def test_pushes_act_in_each_robots_own_window():
    """Robots start at different ticks; a pushed robot equals its unpushed twin exactly up to its window and not after it.  Moderate
    lateral pushes mostly recover; a push large enough to topple does."""
    T, B0 = 60, 256
    rb, rows = _rollout_inputs(B0, 13, push_frac=1.0, push_force=(20.0, 60.0), push_torque=(0.0, 0.0), push_start=(10, 20), push_len=(2, 4))
    tick0 = np.random.default_rng(1).integers(0, 6, B0).astype(np.int32)
    twin = {k: (np.concatenate([v, v]) if isinstance(v, np.ndarray) else v) for k, v in rb.items()}
    body = np.concatenate([rows["body"], rows["body"]])
    push = np.concatenate([rows["push"], np.zeros_like(rows["push"])])
    pt = np.concatenate([rows["push_ticks"], rows["push_ticks"]])
    out = _device_rollout(_solver("f64", warm=True), twin, T, body, push, pt, tick=np.concatenate([tick0, tick0]))
    a = out["actual"]
    for b in range(B0):
        k = rows["push_ticks"][b, 0] - tick0[b] + 1          # first log row after the first pushed tick
        assert np.array_equal(a[b, :k], a[B0 + b, :k]), b
        assert np.abs(a[b, k] - a[B0 + b, k]).max() > 0, b
    end = rows["push_ticks"][:, 1] - tick0 + 20
    late = a[np.arange(B0), np.minimum(end, T - 1)]
    back = (np.abs(late[:, 5] - 0.285) < 0.03) & (np.abs(late[:, 0:2]).max(axis=1) < 0.1)
    print(f"moderate pushes: {int(back.sum())}/{B0} back within the nominal bounds 20 ticks after the window")
    assert 185 <= back.sum() <= 210                                # measured 197 of 256
    big_rows = {"body": rows["body"][:8], "push": np.tile([0.0, 600.0, 0.0, 0.0, 0.0, 0.0], (8, 1)), "push_ticks": np.tile([5, 10], (8, 1)).astype(np.int32)}
    small = {k: (v[:8] if isinstance(v, np.ndarray) else v) for k, v in rb.items()}
    big = _device_rollout(_solver("f64", warm=True), small, 40, big_rows["body"], big_rows["push"], big_rows["push_ticks"])
    ab = big["actual"]
    toppled = ~np.isfinite(ab).all(axis=(1, 2)) | (np.nan_to_num(np.abs(ab[:, :, 0:2]), nan=9.0).max(axis=(1, 2)) > 0.5) | \
        (np.nan_to_num(np.abs(ab[:, :, 3:5] - rb["x"][:8, None, 3:5]), nan=9.0).max(axis=(1, 2)) > 0.5)
    print(f"large push: {int(toppled.sum())}/8 toppled or thrown off")
    assert toppled.all()


@pytest.mark.gpu
def test_mass_mismatch_height_error_grows_with_mismatch():
    T = 60
    scales = np.array([0.8, 0.9, 1.0, 1.1, 1.25])
    rb, _ = _tiled(16, len(scales), 3)
    body = model_body(8.885, [1.0 / 0.24, 1.0, 1.0], 16 * len(scales))
    body[:, 0] *= np.repeat(scales, 16)
    out = _device_rollout(_solver("f64", warm=True), rb, T, body)
    h = (out["actual"][:, 40:, 5] - 0.285).mean(axis=1).reshape(len(scales), 16).mean(axis=1)
    print("mass sweep", dict(zip(scales.tolist(), np.round(h * 1e3, 3).tolist())), "mm")
    assert np.all(np.diff(h) < 0)                                  # heavier sags more, lighter rides high
    assert abs(h[0]) > abs(h[1]) and abs(h[4]) > abs(h[3])


@pytest.mark.gpu
def test_argument_and_row_checks():
    import torch
    sol = _solver("f64")
    eng = sol.engine
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    a = buf.data_ptr()
    for bad in (-1, 1001):
        with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_plant_step: substeps out of range"):
            eng.plant_step_ptr(1, a, a, a, a, 0, 0, bad, a)
        with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_rollout_plant: substeps out of range"):
            eng.rollout_plant_ptr(1, 1, 1, a, a, a, a, a, a, a, 0, 0, 0, bad, 0, 0, 0, 0)
    with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_rollout_plant: push without push_ticks"):
        eng.rollout_plant_ptr(1, 1, 1, a, a, a, a, a, a, a, 0, a, 0, 10, 0, 0, 0, 0)
    with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_plant_step: null buffer"):
        eng.plant_step_ptr(1, a, 0, a, a, 0, 0, 10, a)
    eng.plant_step_ptr(0, 0, 0, 0, 0, 0, 0, 10, 0)
    # an invalid body row: that robot NaN from tick 1, its solves NONFINITE from then on; the others bit-identical
    T, B = 6, 8
    rb, rows = _rollout_inputs(B, 21)
    good = _device_rollout(_solver("f64"), rb, T, rows["body"])
    body = rows["body"].copy(); body[3, 4] = 5.0                   # Ixx Iyy - Ixy^2 < 0
    bad = _device_rollout(_solver("f64"), rb, T, body)
    assert np.all(np.isnan(bad["actual"][3, 1:])) and bad["solved"][3] == 1
    keep = np.arange(B) != 3
    for k in ("actual", "forces", "desired"):
        assert np.array_equal(bad[k][keep], good[k][keep]), k
    assert np.array_equal(bad["solved"][keep], good["solved"][keep])
    assert not np.any(bad["forces"][3, 1:])                       # NONFINITE solves: zero forces
