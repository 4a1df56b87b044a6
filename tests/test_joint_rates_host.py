"""Joint rates and joint power on the host (lite3_model.joint_rates_host, the counterpart of mpcqp_joint_rates in
include/mpcqp_joints.h): recovery of known rates, the power of a stance leg against the work of its ground force, out-of-reach and
non-finite legs.  No GPU: the device is held to this module in tests/test_gpu_joint_rates.py."""
import numpy as np

from mpcqp import lite3_model
from rates_cases import known_rate_logs


def test_known_rates_are_recovered():
    """The band of the joint-log host tests, 1e-10 scaled by max(1, |qd|): fp64 rounding times the conditioning of J, which is that of
    the inverse kinematics on this box (1 / (l sin Knee) <~ 25)."""
    s = known_rate_logs()
    q, qd, tau, power, reach = lite3_model.joint_rates_host(s["actual"], s["forces"], s["feet"], s["foot_vel"])
    q0, tau0, reach0 = lite3_model.joint_log_host(s["actual"], s["forces"], s["feet"])
    assert np.array_equal(q, q0) and np.array_equal(tau, tau0) and np.array_equal(reach, reach0) and np.all(reach == 1)
    eq, ed = np.abs(q - s["q"]).max(), (np.abs(qd - s["qd"]) / np.maximum(1.0, np.abs(s["qd"]))).max()
    print(f"known rates: q {eq:.3e} rad, qd {ed:.3e} (relative to max(1, |qd|)), max |qd| {np.abs(s['qd']).max():.2f} rad/s")
    assert eq <= 1e-10 and ed <= 1e-10
    want = (tau * s["qd"]).sum(axis=-1)
    assert (np.abs(power - want) / np.maximum(1.0, np.abs(want))).max() <= 1e-10 and np.abs(power).max() > 10.0


def test_stance_leg_power_is_the_work_rate_of_its_ground_force():
    s = known_rate_logs(seed=129)
    q, qd, tau, power, reach = lite3_model.joint_rates_host(s["actual"], s["forces"], s["feet"])
    B, T = s["actual"].shape[:2]
    f = s["forces"].reshape(B, T, 4, 3)
    vfoot = s["actual"][:, :, None, 9:12] + np.cross(s["actual"][:, :, None, 6:9], s["feet"] - s["actual"][:, :, None, 3:6])
    want = (f * vfoot).sum(axis=-1)
    err = (np.abs(power - want) / np.maximum(1.0, np.abs(want))).max()
    print(f"stance power against f . (v + omega x r): {err:.3e} relative, max |power| {np.abs(want).max():.1f} W")
    assert err <= 1e-10 and np.all(reach == 1)
    # a body at rest over feet at rest: no joint moves, whatever the forces
    still = s["actual"].copy(); still[..., 6:12] = 0.0
    qd0, p0 = lite3_model.joint_rates_host(still, s["forces"], s["feet"])[1::2]
    assert not qd0.any() and not p0.any()


def test_out_of_reach_and_non_finite_legs():
    s = known_rate_logs(B=4, T=2, seed=130)
    far = s["feet"].copy(); far[3, 1, 2, 2] -= 0.5
    bad = s["actual"].copy(); bad[1, 0, 4] = np.nan                        # a CoM entry: the whole row's legs
    odd = s["foot_vel"].copy(); odd[2, 1, 0, 1] = np.inf                   # one leg's velocity: its rates alone
    q, qd, tau, power, reach = lite3_model.joint_rates_host(bad, s["forces"], far, odd)
    ref = lite3_model.joint_rates_host(s["actual"], s["forces"], s["feet"], s["foot_vel"])
    assert reach[3, 1, 2] == 0 and not qd[3, 1, 2].any() and power[3, 1, 2] == 0.0 and np.isfinite(q[3, 1, 2]).all()
    assert np.isnan(q[1, 0]).all() and np.isnan(qd[1, 0]).all() and np.isnan(tau[1, 0]).all() and np.isnan(power[1, 0]).all()
    assert not reach[1, 0].any()
    assert np.isnan(qd[2, 1, 0]).all() and np.isnan(power[2, 1, 0]) and reach[2, 1, 0] == 1
    assert np.array_equal(q[2, 1, 0], ref[0][2, 1, 0]) and np.array_equal(tau[2, 1, 0], ref[2][2, 1, 0])
    keep = np.ones((4, 2, 4), bool); keep[3, 1, 2] = keep[1, 0] = keep[2, 1, 0] = False
    for got, want in zip((q, qd, tau, power, reach), ref):
        assert np.array_equal(got[keep], want[keep])
