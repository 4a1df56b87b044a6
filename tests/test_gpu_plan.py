"""Device footstep plans and swing-foot trajectories (include/mpcqp_plan.h) against the reference's goldens and the host checkers
(footstep_planner.plan_tables, foot_trajectory_generator.swing_tables), in fp64 and fp32 I/O."""
import numpy as np
import pytest

import mpcqp
from mpcqp.foot_trajectory_generator import swing_tables
from mpcqp.footstep_planner import plan_tables
from plan_cases import CASES, case_inputs, inputs, mask

IO = ("f64", "f32")
TABLES = ("plan_pos", "plan_feet_id", "plan_meta", "plan_ang", "plan_hip")


def _t(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda().contiguous()


def _solver(io, delta, **kw):
    return mpcqp.MPCBatch(N=10, delta=delta, io_dtype=io, precision="mixed", **kw)


def _plan(sol, feet0, cmd, gait, S, **kw):
    import torch
    out = sol.plan_footsteps(_t(feet0, sol.tdtype), _t(cmd, sol.tdtype), _t(gait, torch.int32), S, **kw)
    torch.cuda.synchronize()
    return out


def _np(d):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in d.items()}


def _swing(sol, plan, tick, K, h):
    import torch
    out = sol.swing_trajectories(plan, _t(tick, torch.int32), K, _t(h, sol.tdtype))
    torch.cuda.synchronize()
    return out["traj"].cpu().numpy(), out["feet_des"].cpu().numpy()


def _r32(a):
    """What an fp32 caller hands the device, as fp64 values."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _ulps32(dev, host64, ulps=2):
    """fp32 device values against the fp64 host values rounded once: within `ulps` float32 spacings (spacing taken at >= 2^-20, so
    that values that cancel to near zero are held to an absolute 1e-13, not to the spacing of a denormal).  NaN must match NaN."""
    ref = np.asarray(host64, np.float64).astype(np.float32)
    dev = np.asarray(dev)
    assert dev.dtype == np.float32
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(dev))
    sp = np.spacing(np.maximum(np.abs(ref[~nan]), np.float32(2.0 ** -20)))
    err = np.abs(dev[~nan].astype(np.float64) - ref[~nan].astype(np.float64)) / sp
    return float(err.max()) if err.size else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("io", IO)
@pytest.mark.parametrize("gait,tag", CASES)
def test_device_plans_and_swing_match_golden(golden, io, gait, tag):
    L, G = golden["ref_log"], golden["planner_golden"]
    key = gait + tag
    feet0, cmd, g, dt, h = case_inputs(L, gait, tag)
    S = len(G[key + "_plan_pos"])
    sol = _solver(io, dt)
    plan = _plan(sol, feet0, cmd, g, S)
    p = _np(plan)
    assert np.array_equal(p["plan_feet_id"][0], G[key + "_plan_feet_id"])
    assert p["plan_meta"][0].tolist() == [S, int(g[0, 1]), int(g[0, 2]), 0]
    T = len(G[key + "_swing_traj"])
    traj, des = _swing(sol, plan, np.zeros(1), T, h)
    if io == "f64":
        assert np.abs(p["plan_pos"][0] - G[key + "_plan_pos"]).max() <= 1e-12
        assert np.abs(p["plan_ang"][0] - G[key + "_plan_ang"]).max() <= 1e-12
        assert np.abs(traj[0] - G[key + "_swing_traj"]).max() <= 1e-9
    else:
        # fp32 I/O: the fp64 recurrence on the fp32 inputs, rounded once; and the golden at fp32 input resolution
        ref = plan_tables(_r32(feet0), _r32(cmd), g, S, dt)
        assert _ulps32(p["plan_pos"][0], ref["plan_pos"][0]) <= 2 and _ulps32(p["plan_ang"][0], ref["plan_ang"][0]) <= 2
        assert np.abs(p["plan_pos"][0] - G[key + "_plan_pos"]).max() <= 1e-6 and np.abs(p["plan_ang"][0] - G[key + "_plan_ang"]).max() <= 1e-6
        # the generator on the fp32 plan, carried in fp64 and rounded once
        ref, _ = swing_tables({k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in p.items() if v is not None},
                              np.zeros(1), T, h.astype(np.float32).astype(np.float64), dt)
        assert _ulps32(traj, ref) <= 2
        g6 = G[key + "_swing_traj"]
        for q in range(3):   # pos / vel / acc against the fp64 golden, at the fp32 plan's resolution
            assert np.abs(traj[0, :, :, q] - g6[:, :, q]).max() <= 1e-5 * max(1.0, np.abs(g6[:, :, q]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("io", IO)
def test_device_feet_des_replays_closed_loop_log(golden, io):
    """The log's 1000 x 4 FEET POS des rows (src/main.py:152-167) from one batched call."""
    L, G = golden["ref_log"], golden["planner_golden"]
    feet0, cmd, g, dt, h = inputs(L)
    sol = _solver(io, dt)
    plan = _plan(sol, feet0, cmd, g, int(g[0, 0]))
    _, des = _swing(sol, plan, np.zeros(1), 1000, h)
    if io == "f64":
        assert np.abs(des[0] - G["replay_feet_des"]).max() <= 1e-12
    else:
        p = {k: v.cpu().numpy().astype(np.float64) if v.dtype.is_floating_point else v.cpu().numpy() for k, v in plan.items() if v is not None}
        _, ref = swing_tables(p, np.zeros(1), 1000, h.astype(np.float32).astype(np.float64), dt)
        assert _ulps32(des, ref) <= 2
        assert np.abs(des[0] - G["replay_feet_des"]).max() <= 1e-6


@pytest.fixture(scope="module")
def hetero():
    """4096 heterogeneous robots and their host tables at S = 9 (< most total_steps) and S = 60 (> every total_steps), from the fp64
    inputs and from the inputs an fp32 caller passes."""
    p = mpcqp.synth.make_plan_inputs(4096, seed=20250902)
    cast = {"f64": lambda a: a, "f32": _r32}
    return p, {(S, io): plan_tables(cast[io](p["feet0"]), cast[io](p["cmd"]), p["gait"], S, 0.03) for S in (9, 60) for io in IO}


@pytest.mark.gpu
@pytest.mark.parametrize("io", IO)
@pytest.mark.parametrize("S", [9, 60])
def test_device_tables_match_host_on_heterogeneous_batch(hetero, io, S):
    p, host = hetero
    host = host[S, io]
    sol = _solver(io, 0.03)
    dev = _np(_plan(sol, p["feet0"], p["cmd"], p["gait"], S, want_hip=True))
    assert np.array_equal(dev["plan_meta"], host["plan_meta"]) and np.array_equal(dev["plan_feet_id"], host["plan_feet_id"])
    for k in ("plan_pos", "plan_ang", "plan_hip"):
        if io == "f64":
            assert np.array_equal(np.isnan(dev[k]), np.isnan(host[k])), k
            assert np.nanmax(np.abs(dev[k] - host[k])) <= 1e-12, k
        else:
            assert _ulps32(dev[k], host[k]) <= 2, k
    # swing trajectories of 256 of them from scattered ticks, against the host generator on the device's own tables
    n, K = 256, 60
    tick = np.random.default_rng(S).integers(0, 300, n).astype(np.int32)
    import torch
    sub = {k: _t(dev[k][:n], {np.float64: torch.float64, np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32}[dev[k].dtype.type])
           for k in ("plan_pos", "plan_feet_id", "plan_meta", "plan_ang")}
    traj, des = _swing(sol, sub, tick, K, p["step_height"][:n])
    h_io = p["step_height"][:n].astype(np.float32 if io == "f32" else np.float64).astype(np.float64)
    ref_t, ref_d = swing_tables({k: dev[k][:n].astype(np.float64) if dev[k].dtype == np.float32 else dev[k][:n] for k in sub}, tick, K, h_io, 0.03)
    if io == "f64":
        assert np.abs(traj - ref_t).max() <= 1e-9 and np.abs(des - ref_d).max() <= 1e-12
    else:
        assert _ulps32(traj, ref_t) <= 2 and _ulps32(des, ref_d) <= 2


@pytest.mark.gpu
def test_rollout_on_device_tables_matches_host_tables():
    """mpcqp_rollout on device-made plan tables == on host-made tables of the same inputs (bitwise where the plans are)."""
    import torch
    T, B, S = 30, 24, 50
    rb = mpcqp.synth.make_rollout_batch(B, seed=7)
    pats = mpcqp.synth.gait_patterns(("trot", "gallop", "amble"))
    feet0 = rb["plan_pos"][:, 0]
    cmd = np.tile([0.0, 0.18, 0.0, 0.0, mpcqp.synth.H_COM], (B, 1))
    gait = np.array([[50, 4, 2, mask(pats[i])] for i in rb["gait_ids"]], np.int32)
    sol = _solver("f64", 0.03)
    dev = _plan(sol, feet0, cmd, gait, S, want_ang=False)
    host = plan_tables(feet0, cmd, gait, S, 0.03)
    logs = []
    for tables in ((dev["plan_pos"], dev["plan_feet_id"], dev["plan_meta"]),
                   (_t(host["plan_pos"], torch.float64), _t(host["plan_feet_id"], torch.uint8), _t(host["plan_meta"], torch.int32))):
        x, rf, tick = _t(rb["x"], torch.float64), _t(rb["ref"], torch.float64), _t(rb["tick"], torch.int32)
        out = sol.rollout(x, rf, *tables, tick, _t(rb["mu"], torch.float64), T)
        torch.cuda.synchronize()
        assert np.all(out["solved"].cpu().numpy() == T)
        logs.append({k: out[k].cpu().numpy() for k in ("forces", "actual", "desired")})
    same = all(np.array_equal(dev[k].cpu().numpy(), host[k]) for k in ("plan_pos", "plan_feet_id", "plan_meta"))
    a, b = logs
    if same:
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    else:
        assert np.abs(a["forces"] - b["forces"]).max() <= 1e-4 * max(1.0, np.abs(b["forces"]).max())
        assert np.abs(a["actual"] - b["actual"]).max() <= 1e-5


@pytest.mark.gpu
def test_plan_calls_validate_sizes_and_buffers():
    import torch
    sol = _solver("f64", 0.03)
    eng = sol.engine
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    a = buf.data_ptr()
    bad_plan = [dict(B=-1, S=5), dict(B=1, S=0), dict(B=1 << 31, S=1), dict(B=1 << 20, S=1 << 12)]
    for kw in bad_plan:
        with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_plan_footsteps: size out of range"):
            eng.plan_footsteps_ptr(kw["B"], kw["S"], a, a, a, a, a, a)
    for i in range(6):   # each required buffer NULL in turn
        args = [a] * 6
        args[i] = 0
        with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_plan_footsteps: null buffer"):
            eng.plan_footsteps_ptr(1, 5, *args)
    for B, K, S in ((-1, 5, 5), (1, -1, 5), (1, 5, 0), (1 << 20, 1 << 12, 5)):
        with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_swing_trajectories: size out of range"):
            eng.swing_trajectories_ptr(B, K, S, a, a, a, a, a, a, a)
    for i in range(7):
        args = [a] * 7
        args[i] = 0
        with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_swing_trajectories: null buffer"):
            eng.swing_trajectories_ptr(1, 5, 5, *args)
    eng.plan_footsteps_ptr(0, 5, 0, 0, 0, 0, 0, 0)                    # empty batch: nothing to do, no pointer needed
    eng.swing_trajectories_ptr(3, 0, 5, 0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="operand mismatch"):
        sol.plan_footsteps(buf[:12].view(1, 4, 3), buf[:4].view(1, 4), torch.zeros((1, 4), dtype=torch.int32, device="cuda"), 5)
    with pytest.raises(ValueError, match="operand mismatch"):
        sol.plan_footsteps(buf[:12].view(1, 4, 3).float(), buf[:5].view(1, 5), torch.zeros((1, 4), dtype=torch.int32, device="cuda"), 5)


@pytest.mark.gpu
@pytest.mark.parametrize("io", IO)
def test_two_streams_give_bitwise_equal_results(io):
    """Two handles (a handle serves one stream at a time, include/mpcqp.h) on two non-default streams, enqueued back to back."""
    import torch
    p = mpcqp.synth.make_plan_inputs(1000, seed=4)
    sols = [_solver(io, 0.03) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    ins = [(_t(p["feet0"], s.tdtype), _t(p["cmd"], s.tdtype), _t(p["gait"], torch.int32), _t(p["step_height"], s.tdtype)) for s in sols]
    tick = _t(np.arange(1000) % 97, torch.int32)
    torch.cuda.synchronize()
    outs = []
    for s, st, (f, c, g, h) in zip(sols, streams, ins):
        plan = s.plan_footsteps(f, c, g, 40, want_hip=True, stream=st)
        outs.append((plan, s.swing_trajectories(plan, tick, 50, h, stream=st)))
    torch.cuda.synchronize()
    (p0, s0), (p1, s1) = outs
    for k in TABLES:
        assert torch.equal(p0[k], p1[k]) or (k == "plan_hip" and torch.equal(p0[k].nan_to_num(7.0), p1[k].nan_to_num(7.0))), k
    assert torch.equal(s0["traj"], s1["traj"]) and torch.equal(s0["feet_des"], s1["feet_des"])
