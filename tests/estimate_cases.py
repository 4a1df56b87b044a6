"""Cases shared by tests/test_estimate_host.py and tests/test_gpu_estimate.py (include/mpcqp_estimate.h, mpcqp_imu_log and
mpcqp_estimate_track):

  real       the 16-robot x 25-tick legroll_cases.host_loop("actual") logs (pushed robots included): the IMU rows from the pushed plant's
             right-hand side, the encoders from the roll-out's q / qd logs, init = the first actual row.
  exact      33 robots, 25 rows, feet fixed in the world, encoders from joint_rates_host with the feet at rest.  Robots 0..16: no
             rotation, a constant CoM acceleration of up to 0.5 m/s^2; robots 17..32: a constant yaw rate of up to 0.3 rad/s with a
             constant CoM velocity of up to 0.1 m/s.  The acceleration of the first kind is vertical: a horizontal one tilts the
             specific force against gravity, and the orientation filter then turns towards that apparent vertical by design, so only
             a vertical one leaves the tilt correction an exact zero.  Its start velocity is chosen so that the CoM comes back to its
             start height after the 25 rows and every foot stays in reach (asserted: reach == 1 on every row).
  synthetic  random finite operands, B in {1, 63, 64, 65, 257}, T in {1, 2, 25}, trust strictly between 0 and 1 on half of the legs,
             height given for every other call.

and the growth factor the bands are multiplied by where a state is carried over the rows: the worst change of an output of the real
case, relative to max(1, |output|), under perturbations of 1e-10 of the start state and of every operand, divided by 1e-10.  It is
measured on the host and recorded in tests/golden/estimate_growth.npz (`python tests/estimate_cases.py` regenerates it).
The band itself is the project's (tests/test_gpu_rollout_legs.py, _error): fp64 I/O |dev - host| / max(1, |host|) <= 1e-9, fp32 I/O two
float32 spacings against the host value rounded once, the host fed the float32 operands."""
import functools
import os

import numpy as np

from conftest import ORACLE_SO                                                  # noqa: F401  (first: it puts the repository on the path)
import mpcqp                                                                    # noqa: F401
from legsim_cases import DELTA
from mpcqp import estimator, gaits, lite3_model

GROWTH_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "estimate_growth.npz")
OPERANDS = ("imu", "q", "qd", "contact_log", "init", "trust", "height")         # estimate_track's, in the host's argument names
EXACT_B, EXACT_T, EXACT_SPLIT = 33, 25, 17
EDGE_B, EDGE_T = (1, 63, 64, 65, 257), (1, 2, 25)
BAND64, BAND32 = 1e-9, 2.0


def r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def as_io(case, io):
    """The case as the I/O dtype holds its floating-point operands."""
    if io == "f64":
        return case
    return {k: (r32(v) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for k, v in case.items()}


def operands(case):
    return {k: case.get(k) for k in OPERANDS}


def error(dev, host, io):
    """(error, band) of the project's band; the NaN pattern must match."""
    host = np.asarray(host, np.float64)
    if io == "f32":
        ref = host.astype(np.float32)
        dev = np.asarray(dev)
        nan = np.isnan(ref)
        assert np.array_equal(nan, np.isnan(dev))
        sp = np.spacing(np.maximum(np.abs(ref[~nan]), np.float32(2.0 ** -20)))
        err = np.abs(dev[~nan].astype(np.float64) - ref[~nan].astype(np.float64)) / sp
        return (float(err.max()) if err.size else 0.0), BAND32
    dev = np.asarray(dev, np.float64)
    nan = np.isnan(host)
    assert np.array_equal(nan, np.isnan(dev))
    err = np.abs(dev[~nan] - host[~nan]) / np.maximum(1.0, np.abs(host[~nan]))
    return (float(err.max()) if err.size else 0.0), BAND64


def growth():
    return float(np.load(GROWTH_NPZ)["growth"])


@functools.lru_cache(maxsize=None)
def real_case():
    from legroll_cases import host_loop
    pb, rows, o = host_loop("actual")
    T = o["actual"].shape[1]
    wr = gaits.log_wrench(rows["push"], rows["push_ticks"], pb["tick"], T)
    acc = lite3_model.plant_base_acc_host(o["actual"], o["forces"], o["feet_log"], rows["body"], wrench=wr)
    case = {"actual": o["actual"], "forces": o["forces"], "feet_log": o["feet_log"], "base_acc": acc, "body": rows["body"],
            "q": o["q"], "qd": o["qd"], "contact_log": np.ascontiguousarray(o["contact_log"], dtype=np.uint8),
            "init": np.ascontiguousarray(o["actual"][:, 0]), "trust": None, "height": None}
    case["imu"] = estimator.imu_log_host(case["actual"], case["forces"], case["feet_log"], base_acc=acc)
    assert all(np.isfinite(case[k]).all() for k in ("imu", "q", "qd", "init"))
    return case


@functools.lru_cache(maxsize=None)
def exact_case():
    B, T, d = EXACT_B, EXACT_T, DELTA
    rng = np.random.default_rng(24)
    pb = gaits.make_phase_batch(B, ("stand",), 12, seed=24)
    t = np.arange(T) * d
    p0, feet = pb["x"][:, 3:6], pb["feet"]
    acc, v0, yaw0, wz = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros(B), np.zeros(B)
    a, b = slice(0, EXACT_SPLIT), slice(EXACT_SPLIT, B)
    acc[a, 2] = rng.uniform(-0.5, 0.5, EXACT_SPLIT)
    v0[a, :2] = rng.uniform(-0.1, 0.1, (EXACT_SPLIT, 2)) / np.sqrt(2.0)
    v0[a, 2] = -acc[a, 2] * (0.5 * T * d)
    v0[b] = rng.uniform(-0.1, 0.1, (B - EXACT_SPLIT, 3)) / np.sqrt(3.0)
    yaw0[b], wz[b] = rng.uniform(-0.2, 0.2, B - EXACT_SPLIT), rng.uniform(-0.3, 0.3, B - EXACT_SPLIT)
    actual = np.zeros((B, T, 12))
    actual[:, :, 2] = yaw0[:, None] + wz[:, None] * t
    actual[:, :, 3:6] = p0[:, None] + v0[:, None] * t[None, :, None] + 0.5 * acc[:, None] * (t * t)[None, :, None]
    actual[:, :, 8] = wz[:, None]
    actual[:, :, 9:12] = v0[:, None] + acc[:, None] * t[None, :, None]
    feet_log = np.ascontiguousarray(np.broadcast_to(feet[:, None], (B, T, 4, 3)))
    forces = np.zeros((B, T, 12))
    q, qd, _, _, reach = lite3_model.joint_rates_host(actual, forces, feet_log)
    assert (reach == 1).all()
    base_acc = np.zeros((B, T, 6))
    base_acc[:, :, 3:6] = acc[:, None]
    case = {"actual": actual, "forces": forces, "feet_log": feet_log, "base_acc": base_acc, "body": None, "q": q, "qd": qd,
            "contact_log": np.ones((B, T, 4), np.uint8), "init": np.ascontiguousarray(actual[:, 0]), "trust": None, "height": None,
            "feet_z": np.ascontiguousarray(feet[:, :, 2])}
    case["imu"] = estimator.imu_log_host(actual, forces, feet_log, base_acc=base_acc)
    return case


def edge_cases():
    """(B, T, with height) of every synthetic case: height for every other one."""
    return [(B, T, (i * len(EDGE_T) + j) % 2 == 1) for i, B in enumerate(EDGE_B) for j, T in enumerate(EDGE_T)]


@functools.lru_cache(maxsize=None)
def edge_case(B, T, with_height):
    rng = np.random.default_rng(1000 * B + T)
    imu = rng.normal(0.0, 0.3, (B, T, 6))
    imu[..., 5] += 9.81
    q = np.array([0.0, -0.9, 1.7]) + rng.normal(0.0, 0.15, (B, T, 4, 3))
    qd = rng.normal(0.0, 1.0, (B, T, 4, 3))
    contact = (rng.random((B, T, 4)) > 0.4).astype(np.uint8)
    trust = np.where(rng.random((B, T, 4)) < 0.5, rng.uniform(0.05, 0.95, (B, T, 4)), contact.astype(np.float64))
    init = rng.normal(0.0, 0.1, (B, 12))
    init[:, 5] += 0.3
    case = {"imu": imu, "q": q, "qd": qd, "contact_log": contact, "init": init, "trust": trust,
            "height": rng.normal(0.0, 0.01, (B, 4)) if with_height else None}
    # and the operands of imu_log on the same sizes
    case["actual"] = rng.normal(0.0, 0.3, (B, T, 12))
    case["forces"] = rng.normal(0.0, 20.0, (B, T, 12)) * np.repeat(contact, 3, axis=-1)
    case["feet_log"] = rng.normal(0.0, 0.2, (B, T, 4, 3))
    case["base_acc"] = rng.normal(0.0, 2.0, (B, T, 6)) if with_height else None
    case["body"] = mpcqp.synth.make_plant_rows(B, seed=B + T)["body"] if T != 2 else None
    case["bias"] = rng.normal(0.0, 0.01, (B, 6)) if T != 1 else None
    case["noise"] = rng.normal(0.0, 0.05, (B, T, 6)) if B != 64 else None
    return case


def imu_operands(case):
    return {"base_acc": case.get("base_acc"), "body": case.get("body"), "bias": case.get("bias"), "noise": case.get("noise")}


@functools.lru_cache(maxsize=None)
def host_result(kind, io, *key):
    """estimate_track_host on a case as the I/O dtype holds it, computed once."""
    case = as_io({"real": real_case, "exact": exact_case, "edge": edge_case}[kind](*key), io)
    return estimator.estimate_track_host(**operands(case), delta=DELTA)


def measure_growth(eps=1e-10, seed=11):
    """The worst relative output change of the real case over its 25 rows under perturbations of eps of the start state and the
    operands, over eps."""
    case = real_case()
    rng = np.random.default_rng(seed)
    ops = operands(case)
    pert = {k: (v + eps * rng.choice([-1.0, 1.0], v.shape) if k in ("imu", "q", "qd", "init") else v) for k, v in ops.items()}
    a, b = estimator.estimate_track_host(**ops, delta=DELTA), estimator.estimate_track_host(**pert, delta=DELTA)
    return max(float((np.abs(a[k] - b[k]) / np.maximum(1.0, np.abs(a[k]))).max()) for k in estimator.OUT) / eps


if __name__ == "__main__":                                                      # regenerate tests/golden/estimate_growth.npz
    g = measure_growth()
    np.savez(GROWTH_NPZ, growth=np.float64(g), eps=np.float64(1e-10))
    print("growth over the real case's 25 rows", g)
