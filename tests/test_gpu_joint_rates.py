"""Joint rates and joint power on the device (include/mpcqp_joints.h, mpcqp_joint_rates) against the host counterpart
lite3_model.joint_rates_host on logs with known angles and rates, against mpcqp_joint_log on the same operands bit for bit, and the
NULL-output combinations."""
import itertools

import numpy as np
import pytest

import mpcqp
from mpcqp import lite3_model
from rates_cases import known_rate_logs

B, T = 32, 4            # 128 rows
OUT = ("q", "qd", "tau", "power", "reach")


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


def _logs(io):
    """The known-rate logs (row (0, 0) has |theta| < 1e-6) with one leg's foot out of reach and one robot-tick's feet far away."""
    s = known_rate_logs(B, T)
    s["feet"][3, 1, 2, 2] -= 0.5
    s["feet"][7, 2] += [0.0, 0.0, 2.0]
    if io == "f32":
        s = {k: _r32(v) for k, v in s.items()}
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_against_the_host_and_against_joint_log(io):
    """f64: 1e-9, the device band of the joint log -- the rates go through the same J, whose conditioning is bounded on the box.
    f32: host and device share the fp64 arithmetic on the same fp32 logs; what is left is the rounding of the outputs, 2 spacings."""
    import torch
    s = _logs(io)
    assert np.linalg.norm(s["actual"][0, 0, :3]) < 1e-6
    sol = mpcqp.MPCBatch(io_dtype=io)
    dt = sol.tdtype
    a, f, ft, fv = (_t(s[k], dt) for k in ("actual", "forces", "feet", "foot_vel"))
    for vel, hvel in ((fv, s["foot_vel"]), (None, None)):
        out = sol.joint_rates(a, f, ft, vel)
        jl = sol.joint_log(a, f, ft)
        torch.cuda.synchronize()
        for k in ("q", "tau", "reach"):
            assert torch.equal(out[k], jl[k]), k                                # mpcqp_joint_log's, bit for bit
        host = dict(zip(OUT, lite3_model.joint_rates_host(s["actual"], s["forces"], s["feet"], hvel)))
        got = {k: out[k].cpu().numpy() for k in OUT}
        assert np.array_equal(got["reach"], host["reach"]) and got["reach"].sum() == got["reach"].size - 5
        assert not got["qd"][3, 1, 2].any() and not got["qd"][7, 2].any() and not got["power"][7, 2].any() and got["power"][3, 1, 2] == 0.0
        for k in ("q", "qd", "tau", "power"):
            err = np.abs(got[k] - host[k]).max() if io == "f64" else _ulps32(got[k], host[k])
            band = 1e-9 if io == "f64" else 2.0
            print(f"joint_rates {io} foot_vel={'yes' if vel is not None else 'None'} {k}: err {err:.3e} band {band:.1e} "
                  f"(max |{k}| {np.abs(host[k]).max():.2f})")
            assert err <= band, (k, err)
        if vel is not None and io == "f64":
            ok = got["reach"] == 1
            assert np.abs(got["qd"] - s["qd"])[ok].max() <= 1e-9                # the rates the logs were made from
        else:
            assert np.abs(got["power"]).max() > 10.0 and np.abs(got["qd"]).max() > 1.0


@pytest.mark.gpu
def test_null_outputs_and_argument_checks():
    import torch
    s = _logs("f64")
    sol = mpcqp.MPCBatch(io_dtype="f64")
    eng = sol.engine
    a, f, ft, fv = (_t(s[k], sol.tdtype) for k in ("actual", "forces", "feet", "foot_vel"))
    out = sol.joint_rates(a, f, ft, fv)
    torch.cuda.synchronize()
    ins = (a.data_ptr(), f.data_ptr(), ft.data_ptr(), fv.data_ptr())
    # every non-empty subset of the five outputs: what is asked for is what the full call gives, what is not is not written
    for keep in itertools.product((False, True), repeat=5):
        bufs = [torch.full_like(out[k], 7) for k in OUT]
        ptrs = [b.data_ptr() if on else 0 for b, on in zip(bufs, keep)]
        if not any(keep):
            with pytest.raises(mpcqp.MpcQpError, match=r"-1.*no output"):
                eng.joint_rates_ptr(B, T, *ins, *ptrs)
            continue
        eng.joint_rates_ptr(B, T, *ins, *ptrs)
        torch.cuda.synchronize()
        for b, on, k in zip(bufs, keep, OUT):
            assert torch.equal(b, out[k]) if on else bool((b == 7).all()), (keep, k)
    q = out["q"].data_ptr()
    with pytest.raises(mpcqp.MpcQpError, match=r"-1.*null buffer"):
        eng.joint_rates_ptr(B, T, ins[0], 0, ins[2], ins[3], q, 0, 0, 0, 0)
    for bad in ((B, -1), (-1, T), (2 ** 20, 2 ** 10)):
        with pytest.raises(mpcqp.MpcQpError, match=r"-1.*size"):
            eng.joint_rates_ptr(*bad, *ins, q, 0, 0, 0, 0)
    eng.joint_rates_ptr(B, 0, 0, 0, 0, 0, q, 0, 0, 0, 0)                         # no ticks: a no-op
    eng.joint_rates_ptr(0, T, 0, 0, 0, 0, q, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="foot_vel"):
        sol.joint_rates(a, f, ft, fv.view(B, T, 12))
    # a non-finite body twist or foot velocity: that leg's rates and power, not its angles and torques
    bad = s["actual"].copy(); bad[5, 2, 7] = np.nan
    odd = s["foot_vel"].copy(); odd[9, 1, 3, 0] = np.inf
    o2 = sol.joint_rates(_t(bad, sol.tdtype), f, ft, _t(odd, sol.tdtype))
    torch.cuda.synchronize()
    hit = np.zeros((B, T, 4), bool); hit[5, 2] = True; hit[9, 1, 3] = True
    m = torch.as_tensor(hit).cuda()
    assert bool(torch.isnan(o2["qd"][m]).all()) and bool(torch.isnan(o2["power"][m]).all())
    for k in OUT:
        assert torch.equal(o2[k][~m], out[k][~m]), k
    for k in ("q", "tau", "reach"):
        assert torch.equal(o2[k], out[k]), k
