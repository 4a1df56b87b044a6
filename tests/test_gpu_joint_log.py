"""Joint-space log of a roll-out on the device (include/mpcqp_joints.h, mpcqp_joint_log) against its host counterpart
lite3_model.joint_log_host: a synthetic case with known joint angles, and the chain plan_footsteps -> rollout_plant ->
swing_trajectories(K = T) -> joint_log at the smallest shape that has swing legs."""
import numpy as np
import pytest

import mpcqp
from mpcqp import lite3_model, synth
from plan_cases import mask


def _t(a, dt):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _synthetic(B=65, T=3, seed=65):
    """Logs with known joint angles: random small rotation vectors (one row with |theta| < 1e-6, in the series range of the
    rotation-vector conversion, and one near 1.0 rad), feet = CoM + R FK(q) of in-box q, random forces."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    q = np.stack([rng.uniform(-0.5, 0.5, (B, T, 4)), rng.uniform(-1.5, -0.2, (B, T, 4)), rng.uniform(0.5, 2.3, (B, T, 4))], axis=-1)
    actual = np.zeros((B, T, 12))
    actual[..., 0:3] = rng.normal(0.0, 0.15, (B, T, 3))
    actual[0, 0, 0:3] = [3e-7, -2e-7, 5e-7]
    actual[0, 1, 0:3] = 0.0
    actual[1, 0, 0:3] = np.array([0.6, -0.5, 0.62]) * (1.0 / np.linalg.norm([0.6, -0.5, 0.62]))
    actual[..., 3:6] = rng.normal(0.0, 0.5, (B, T, 3)) + [0.0, 0.0, 0.285]
    actual[..., 6:12] = rng.normal(0.0, 0.3, (B, T, 6))
    forces = rng.normal(0.0, 30.0, (B, T, 12))
    R = Rotation.from_rotvec(actual[..., :3].reshape(-1, 3)).as_matrix().reshape(B, T, 3, 3)
    p = np.array([[[lite3_model.leg_fk_jac(l, q[b, t, l])[0] for l in range(4)] for t in range(T)] for b in range(B)])
    feet = actual[:, :, None, 3:6] + np.einsum("btij,btlj->btli", R, p)
    return {"q": q, "actual": actual, "forces": forces, "feet": feet}


@pytest.mark.gpu
def test_synthetic_logs_against_the_host():
    import torch
    B, T = 65, 3
    s = _synthetic(B, T)
    qh, tauh, rh = lite3_model.joint_log_host(s["actual"], s["forces"], s["feet"])
    assert np.abs(qh - s["q"]).max() <= 1e-10 and np.all(rh == 1)          # the host finds the angles the feet were made from
    sol = mpcqp.MPCBatch(io_dtype="f64")
    a, f, ft = (_t(s[k], sol.tdtype) for k in ("actual", "forces", "feet"))
    out = sol.joint_log(a, f, ft)
    torch.cuda.synchronize()
    eq, et = np.abs(out["q"].cpu().numpy() - qh).max(), np.abs(out["tau"].cpu().numpy() - tauh).max()
    print(f"synthetic f64: q {eq:.3e} rad, tau {et:.3e} N m (|tau| <= {np.abs(tauh).max():.1f})")
    assert eq <= 1e-10 and et <= 1e-10
    assert np.array_equal(out["reach"].cpu().numpy(), rh)
    # each output may be NULL on its own: the others are what they were; all three NULL is an argument error
    eng = sol.engine
    for skip in range(3):
        bufs = [torch.full_like(out["q"], 7.0), torch.full_like(out["tau"], 7.0), torch.full_like(out["reach"], 7)]
        ptrs = [0 if i == skip else b.data_ptr() for i, b in enumerate(bufs)]
        eng.joint_log_ptr(B, T, a.data_ptr(), f.data_ptr(), ft.data_ptr(), *ptrs)
        torch.cuda.synchronize()
        for i, (b, k) in enumerate(zip(bufs, ("q", "tau", "reach"))):
            assert bool((b == 7).all()) if i == skip else torch.equal(b, out[k])
    with pytest.raises(mpcqp.MpcQpError, match=r"-1.*no output"):
        eng.joint_log_ptr(B, T, a.data_ptr(), f.data_ptr(), ft.data_ptr(), 0, 0, 0)
    with pytest.raises(mpcqp.MpcQpError, match=r"-1.*null buffer"):
        eng.joint_log_ptr(B, T, a.data_ptr(), 0, ft.data_ptr(), out["q"].data_ptr(), 0, 0)
    with pytest.raises(mpcqp.MpcQpError, match=r"-1.*size"):
        eng.joint_log_ptr(B, -1, a.data_ptr(), f.data_ptr(), ft.data_ptr(), out["q"].data_ptr(), 0, 0)
    eng.joint_log_ptr(B, 0, 0, 0, 0, out["q"].data_ptr(), 0, 0)            # no ticks: a no-op
    with pytest.raises(ValueError, match="feet"):
        sol.joint_log(a, f, ft.view(B, T, 12))
    # out of reach: the torque of the clamped q; a non-finite row is NaN in q and tau, 0 in reach, and stays in its own row
    far = s["feet"].copy(); far[3, 1, 2, 2] -= 0.5
    bad = s["actual"].copy(); bad[5, 2, 4] = np.nan
    o2 = sol.joint_log(_t(bad, sol.tdtype), f, _t(far, sol.tdtype))
    torch.cuda.synchronize()
    q2, tau2, r2 = (o2[k].cpu().numpy() for k in ("q", "tau", "reach"))
    q2h, tau2h, r2h = lite3_model.joint_log_host(bad, s["forces"], far)
    assert r2[3, 1, 2] == 0 and r2.sum() == r2.size - 5 and np.array_equal(r2, r2h)
    assert np.isnan(q2[5, 2]).all() and np.isnan(tau2[5, 2]).all() and np.isnan(q2).sum() == 12 == np.isnan(tau2).sum()
    assert np.isfinite(q2[3, 1, 2]).all() and q2[3, 1, 2, 2] == 0.0        # the stretched leg
    keep = ~np.isnan(q2h)
    assert np.abs(q2 - q2h)[keep].max() <= 1e-10 and np.abs(tau2 - tau2h)[keep].max() <= 1e-10
    untouched = np.ones((B, T, 4), bool); untouched[3, 1, 2] = False; untouched[5, 2] = False
    m = torch.as_tensor(untouched).cuda()
    assert torch.equal(o2["q"][m], out["q"][m]) and torch.equal(o2["tau"][m], out["tau"][m])


def _trot_chain(io, B=64, T=8):
    """plan_footsteps (default trot, ss = 4, ds = 2: ticks 6 and 7 are the first swing) -> rollout_plant -> swing_trajectories."""
    import torch
    sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed")
    rng = np.random.default_rng(64)
    com = np.array([0.0, 0.0, synth.H_COM]) + rng.normal(0.0, 0.005, (B, 3)) * [1.0, 1.0, 0.5]
    feet0 = synth.NOMINAL_FEET[None] + np.stack([com[:, 0], com[:, 1], np.full(B, synth.H_COM)], axis=1)[:, None]
    cmd = np.tile([0.0, 0.18, 0.0, 0.0, synth.H_COM], (B, 1))
    gait = np.tile(np.array([20, 4, 2, mask(synth.GAITS["trot"])], np.int32), (B, 1))
    x = np.zeros((B, 13)); x[:, 3:6] = com; x[:, 6:12] = rng.normal(0.0, 0.02, (B, 6)); x[:, 12] = synth.G_ACC
    ref = np.zeros((B, 10)); ref[:, 3:5] = com[:, :2]; ref[:, 5] = synth.H_COM; ref[:, 6] = 0.18
    dt = sol.tdtype
    tick = _t(np.zeros(B), torch.int32)
    plan = sol.plan_footsteps(_t(feet0, dt), _t(cmd, dt), _t(gait, torch.int32), 4)
    sw = sol.swing_trajectories(plan, tick, T, _t(np.full(B, 0.08), dt))      # (before the roll-out advances `tick`)
    out = sol.rollout_plant(_t(x, dt), _t(ref, dt), plan["plan_pos"], plan["plan_feet_id"], plan["plan_meta"], tick, _t(np.full(B, 0.7), dt), T)
    jl = sol.joint_log(out["actual"], out["forces"], sw["feet_des"])
    torch.cuda.synchronize()
    assert bool((out["solved"] == T).all())
    return {k: v.cpu().numpy() for k, v in dict(actual=out["actual"], forces=out["forces"], feet=sw["feet_des"], **jl).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_trot_rollout_to_joint_torques(io):
    """f64: 1e-9 against the host on the same logs.  f32: host and device share the fp64 arithmetic on the same fp32 logs, so what
    is left is the rounding of the outputs -- 5e-7 rad for |q| <= 2.3, and the same relative band at the magnitude of the torques,
    5e-7 * max(1, max |tau| / 2.3) N m."""
    B, T = 64, 8
    r = _trot_chain(io, B, T)
    q, tau, reach = r["q"].astype(np.float64), r["tau"].astype(np.float64), r["reach"]
    assert np.all(reach == 1)
    forces = r["forces"].reshape(B, T, 4, 3)
    swing = np.all(forces == 0.0, axis=3)
    assert swing.any() and not swing.all() and not swing[:, :6].any()        # all stance in step 0, two legs up afterwards
    assert np.all(tau[swing] == 0.0)
    assert np.all(tau[~swing][:, 2] != 0.0) and np.abs(tau[~swing][:, 2]).max() > 1.0    # a stance knee carries load
    qh, tauh, rh = lite3_model.joint_log_host(r["actual"].astype(np.float64), r["forces"].astype(np.float64), r["feet"].astype(np.float64))
    eq, et = np.abs(q - qh).max(), np.abs(tau - tauh).max()
    print(f"trot {io}: q {eq:.3e} rad, tau {et:.3e} N m (max |tau| {np.abs(tauh).max():.2f}, min stance knee |tau| {np.abs(tau[~swing][:, 2]).min():.2f})")
    assert np.all(rh == 1)
    if io == "f64":
        assert eq <= 1e-9 and et <= 1e-9
    else:
        assert eq <= 5e-7 and et <= 5e-7 * max(1.0, np.abs(tauh).max() / 2.3)
