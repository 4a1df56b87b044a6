"""Closed-form leg inverse kinematics on the device (include/mpcqp_joints.h, mpcqp_leg_ik) against its host counterpart
lite3_model.leg_ik_closed and against the device's own forward map mpcqp_leg_jacobians.  B = 257: the last block is partial and
4 * 257 legs are no multiple of the wave."""
import ctypes

import numpy as np
import pytest

import mpcqp
from mpcqp import lite3_model

B = 257


def _t(a, dt):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def legs():
    """In-box joint vectors [B,4,3], their feet in the torso frame, and a random torso pose per robot."""
    rng = np.random.default_rng(257)
    q = np.stack([rng.uniform(-0.5, 0.5, (B, 4)), rng.uniform(-1.5, -0.2, (B, 4)), rng.uniform(0.5, 2.3, (B, 4))], axis=2)
    assert np.all(0.20 * np.cos(q[..., 1]) + 0.21 * np.cos(q[..., 1] + q[..., 2]) > 0.0)      # all on the closed form's branch
    foot = np.array([[lite3_model.leg_fk_jac(l, q[b, l])[0] for l in range(4)] for b in range(B)])
    R = np.linalg.qr(rng.normal(size=(B, 3, 3)))[0]
    R[:, :, 0] *= np.sign(np.linalg.det(R))[:, None]
    origin = rng.normal(0.0, 1.0, (B, 3))
    return {"q": q, "foot": foot, "R": R, "origin": origin}


def _sol(io):
    return mpcqp.MPCBatch(io_dtype=io)


def _run(sol, foot, rot=None, origin=None, **kw):
    import torch
    opt = lambda a: None if a is None else _t(a, sol.tdtype)
    q, reach = sol.leg_ik(_t(foot, sol.tdtype), opt(rot), opt(origin), **kw)
    torch.cuda.synchronize()
    return q, reach


@pytest.mark.gpu
def test_f64_matches_host_and_inverts_the_device_forward_map(legs):
    import torch
    sol = _sol("f64")
    q, reach = _run(sol, legs["foot"])
    qh, rh = lite3_model.leg_ik_closed(legs["foot"])
    err = np.abs(q.cpu().numpy() - qh).max()
    print(f"f64 device - host: {err:.3e} rad; host - drawn q: {np.abs(qh - legs['q']).max():.3e}")
    assert err <= 1e-12
    assert np.array_equal(reach.cpu().numpy(), rh) and np.all(rh == 1)
    _, foot = sol.leg_jacobians(q)
    torch.cuda.synchronize()
    back = np.abs(foot.cpu().numpy() - legs["foot"]).max()
    print(f"f64 FK(IK(foot)) - foot on the device: {back:.3e} m")
    assert back <= 1e-12
    q2, reach2 = _run(sol, legs["foot"])                  # bitwise deterministic
    assert torch.equal(q, q2) and torch.equal(reach, reach2)
    qn, none = _run(sol, legs["foot"], want_reach=False)  # reach may be NULL
    assert none is None and torch.equal(qn, q)


@pytest.mark.gpu
def test_f32_buffers_carry_the_fp64_result_rounded(legs):
    """5e-7 rad: the output rounding of |q| <= 2.3 (1.2e-7) plus the fp32 rounding of the inputs, which host and device share; the
    fp64 arithmetic is common to both."""
    sol = _sol("f32")
    foot = _r32(legs["foot"])
    q, reach = _run(sol, foot)
    qh, rh = lite3_model.leg_ik_closed(foot)
    err = np.abs(q.cpu().numpy().astype(np.float64) - qh).max()
    print(f"f32 device - host: {err:.3e} rad")
    assert err <= 5e-7 and np.array_equal(reach.cpu().numpy(), rh)
    # ... and with a torso pose: the host sees the same fp32-rounded rot / origin / foot
    R, o = _r32(legs["R"]), _r32(legs["origin"])
    fw = _r32(o[:, None] + np.einsum("bij,blj->bli", R, foot))
    q, reach = _run(sol, fw, R, o)
    qh, rh = lite3_model.leg_ik_closed(np.einsum("bji,blj->bli", R, fw - o[:, None]))
    ok = rh == 1                                          # (fp32 rounding of a world position can push a leg across a boundary)
    err = np.abs(q.cpu().numpy().astype(np.float64) - qh)[ok].max()
    print(f"f32 device - host with rot / origin: {err:.3e} rad on {ok.mean():.3f} of the legs")
    assert ok.mean() > 0.99 and err <= 5e-7


@pytest.mark.gpu
def test_rot_and_origin_against_their_null_forms(legs):
    sol = _sol("f64")
    base, _ = _run(sol, legs["foot"])
    base = base.cpu().numpy()
    R, o = legs["R"], legs["origin"]
    rotated = np.einsum("bij,blj->bli", R, legs["foot"])
    for foot, rot, origin in ((rotated, R, None), (legs["foot"] + o[:, None], None, o), (rotated + o[:, None], R, o)):
        q, reach = _run(sol, foot, rot, origin)
        assert np.abs(q.cpu().numpy() - base).max() <= 1e-12 and bool(reach.all())


def _mixed_rows():
    """Reachable legs, the unreachable kinds (stretched, folded, inside the HipX cylinder) and their host answers; no point lies
    within 1e-9 of a boundary."""
    rng = np.random.default_rng(5)
    foot = np.empty((B, 4, 3))
    hip = lite3_model._HIPX + lite3_model._HIPY
    kind = np.arange(B) % 4
    for b in range(B):
        dz = {0: -rng.uniform(0.12, 0.38), 1: -rng.uniform(0.45, 0.9), 2: -rng.uniform(0.001, 0.008), 3: None}[int(kind[b])]
        for l in range(4):
            if dz is None:      # inside the cylinder p_y^2 + p_z^2 < d^2
                foot[b, l] = lite3_model._HIPX[l] + [rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)]
            else:
                foot[b, l] = hip[l] + [rng.uniform(-0.2, 0.2) * abs(dz), 0.0, dz]
    return foot, kind


@pytest.mark.gpu
def test_reach_flags_and_a_nan_row():
    import torch
    sol = _sol("f64")
    foot, kind = _mixed_rows()
    qh, rh = lite3_model.leg_ik_closed(foot)
    assert np.all(rh[kind == 0] == 1) and np.all(rh[kind != 0] == 0) and np.isfinite(qh).all()
    q, reach = _run(sol, foot)
    assert np.array_equal(reach.cpu().numpy(), rh)
    assert np.abs(q.cpu().numpy() - qh).max() <= 1e-12
    dirty = foot.copy()
    dirty[100, 2, 1] = np.nan; dirty[200, 0, 0] = np.inf
    qd, rd = _run(sol, dirty)
    hit = np.zeros((B, 4), bool); hit[100, 2] = True; hit[200, 0] = True
    hit_t = torch.as_tensor(hit).cuda()
    assert bool(torch.isnan(qd[hit_t]).all()) and bool((rd[hit_t] == 0).all())
    assert torch.equal(qd[~hit_t], q[~hit_t]) and torch.equal(rd[~hit_t], reach[~hit_t])      # neighbours: bitwise untouched
    # a non-finite torso pose takes the robot's four legs, and nothing else
    R = np.tile(np.eye(3), (B, 1, 1)); R[7, 1, 1] = np.nan
    o = np.zeros((B, 3)); o[9, 2] = -np.inf
    qp, rp = _run(sol, foot, R, o)
    rows = torch.zeros(B, dtype=torch.bool, device="cuda"); rows[7] = True; rows[9] = True
    assert bool(torch.isnan(qp[rows]).all()) and bool((rp[rows] == 0).all())
    assert torch.equal(qp[~rows], q[~rows]) and torch.equal(rp[~rows], reach[~rows])


@pytest.mark.gpu
def test_argument_checks():
    import torch
    sol = _sol("f64")
    eng = sol.engine
    buf = torch.zeros(B * 12, dtype=torch.float64, device="cuda")
    out = torch.zeros(B * 12, dtype=torch.float64, device="cuda")
    with pytest.raises(mpcqp.MpcQpError, match=r"-1.*null foot"):
        eng.leg_ik_ptr(B, 0, 0, 0, out.data_ptr())
    with pytest.raises(mpcqp.MpcQpError, match=r"-1.*null q"):
        eng.leg_ik_ptr(B, buf.data_ptr(), 0, 0, 0)
    with pytest.raises(mpcqp.MpcQpError, match=r"-1.*batch size"):
        eng.leg_ik_ptr(-1, buf.data_ptr(), 0, 0, out.data_ptr())
    eng.leg_ik_ptr(0, 0, 0, 0, 0)                        # the empty batch is a no-op, as for mpcqp_leg_jacobians
    q0, r0 = sol.leg_ik(buf[:0].view(0, 4, 3))
    assert tuple(q0.shape) == (0, 4, 3) and tuple(r0.shape) == (0, 4)

    def geometry(**fields):
        g = mpcqp._capi.MpcQpLegGeometry()
        assert mpcqp.product_library().lib.mpcqp_default_leg_geometry(ctypes.byref(g)) == 0
        for name, vals in fields.items():
            for i, v in enumerate(vals):
                getattr(g, name)[i] = v
        return g

    for fields, word in ((dict(knee=(0.01, 0.0, -0.2)), "knee"), (dict(axis_y=(0.0, -1.0, 0.1)), "axis_y"),
                         (dict(axis_x=(0.0, 0.0, 1.0)), "axis_x"), (dict(foot=(0.0, 0.0, 0.21)), "foot")):
        with pytest.raises(mpcqp.MpcQpError, match=rf"-1.*{word}"):
            eng.leg_ik_ptr(B, buf.data_ptr(), 0, 0, out.data_ptr(), geometry=geometry(**fields))
    g = geometry(); g.hip_y[2][2] = 0.01
    with pytest.raises(mpcqp.MpcQpError, match=r"-1.*hip_y"):
        eng.leg_ik_ptr(B, buf.data_ptr(), 0, 0, out.data_ptr(), geometry=g)
    bad = mpcqp._capi.MpcQpLegGeometry()                 # size field left at zero
    with pytest.raises(mpcqp.MpcQpError, match=r"-1.*size"):
        eng.leg_ik_ptr(B, buf.data_ptr(), 0, 0, out.data_ptr(), geometry=bad)
    torch.cuda.synchronize()
    assert not bool(out.any())                           # nothing was launched
    with pytest.raises(ValueError, match="foot"):
        sol.leg_ik(buf[:12].view(1, 4, 3).float())
    with pytest.raises(ValueError, match="rot"):
        sol.leg_ik(buf[:12].view(1, 4, 3), rot=buf[:3].view(1, 3))


@pytest.mark.gpu
def test_a_geometry_of_the_callers_own():
    """Longer links, mirrored joint axes given unnormalised: the inverse reads the link lengths and the axis signs from the geometry
    and inverts the device's forward map for it."""
    import torch
    sol = _sol("f64")
    g = mpcqp._capi.MpcQpLegGeometry()
    mpcqp.product_library().lib.mpcqp_default_leg_geometry(ctypes.byref(g))
    g.knee[2] = -0.35; g.foot[2] = -0.3; g.axis_y[1] = 2.0; g.axis_x[0] = 1.0
    rng = np.random.default_rng(8)
    q = np.stack([rng.uniform(-0.5, 0.5, (B, 4)), rng.uniform(-1.5, -0.2, (B, 4)), rng.uniform(0.5, 2.3, (B, 4))], axis=2)
    assert np.all(0.35 * np.cos(q[..., 1]) + 0.3 * np.cos(q[..., 1] + q[..., 2]) > 0.0)      # on the branch (axis_y = +e_y: HipY < 0)
    tq = _t(q, sol.tdtype)
    _, foot = sol.leg_jacobians(tq, geometry=g)
    back, reach = sol.leg_ik(foot, geometry=g)
    torch.cuda.synchronize()
    assert bool(reach.all()) and float((back - tq).abs().max()) <= 1e-12
