"""The state estimator on the host (mpcqp.estimator, the counterparts of include/mpcqp_estimate.h); the cases are in
tests/estimate_cases.py.  No GPU.

  1. estimate_track_host (three 6-state filters, scalar updates) equals estimate_joint_host (18 states, batch update) within the band,
     without the growth factor, on the real case and on every synthetic edge.
  2. On the exact case est equals the constructed truth within the band, feet_est the feet, and nis stays below 1e-12.
  3. Convergence on the exact case's first kind of motion with init off by (0.05, -0.03, 0.04) m and 0.2 m/s, height given, defaults.
  4. P symmetric bit for bit, its smallest eigenvalue above -1e-12 on every row, sigma does not grow across an update.
  5. A call in two pieces (13 + 12 rows, with state) equals one call bit for bit.
  6. imu_log_host: flight, standing, a pushed row.
"""
import numpy as np
import pytest

import estimate_cases as C
from legsim_cases import DELTA
from mpcqp import estimator, lite3_model, plant


def _close(name, a, b, scale=1.0):
    err, band = C.error(a, b, "f64")
    print(f"{name}: error {err:.3e}, band {band * scale:.3e}")
    assert err <= band * scale, name


def _both_forms(case):
    ops = C.operands(case)
    a, b = estimator.estimate_track_host(**ops, delta=DELTA), estimator.estimate_joint_host(**ops, delta=DELTA)
    for k in estimator.OUT:
        _close(k, a[k], b[k])


def test_sequential_equals_joint_real():
    _both_forms(C.real_case())
    _both_forms(dict(C.real_case(), height=np.zeros((16, 4))))


@pytest.mark.parametrize("B,T,with_height", C.edge_cases())
def test_sequential_equals_joint_edges(B, T, with_height):
    _both_forms(C.edge_case(B, T, with_height))


def test_exact_case():
    c, o = C.exact_case(), C.host_result("exact", "f64")
    _close("est", o["est"], c["actual"])
    _close("feet", o["feet"], c["feet_log"])
    print("largest nis", o["nis"].max())
    assert o["nis"].max() < 1e-12


def _offset_run(dv):
    c = C.exact_case()
    a = slice(0, C.EXACT_SPLIT)
    ops = {k: (None if v is None else v[a]) for k, v in C.operands(c).items()}
    ops["init"] = ops["init"].copy()
    ops["init"][:, 3:6] += np.array([0.05, -0.03, 0.04])
    ops["init"][:, 9:12] += np.asarray(dv)
    ops["height"] = c["feet_z"][a]
    e = estimator.estimate_track_host(**ops, delta=DELTA)["est"][:, -1] - c["actual"][a, -1]
    return np.linalg.norm(e[:, 9:12], axis=-1).max(), np.abs(e[:, 5]).max(), np.abs(e[:, 3:5] - np.array([0.05, -0.03])).max()


def test_convergence():
    """The velocity offset of 0.2 m/s is vertical where the three conditions are asserted together: position along z is observable
    through the height rows, and the xy filters then see an exact velocity, so the initial xy offset stays to the last bit -- the
    absolute xy is not observable.  With the same 0.2 m/s on every axis the velocity and the height still converge (asserted), and
    while the horizontal velocity converges the common mode of CoM and feet moves with it: the xy error then differs from the initial
    offset by 4.9e-6 m at the last row (printed, not asserted: it is the filter's answer to a wrong start velocity, not a defect)."""
    v, pz, pxy = _offset_run((0.0, 0.0, 0.2))
    print(f"vertical velocity offset: v error {v:.3e}, p_z error {pz:.3e}, |p_xy error - offset| {pxy:.3e}")
    assert v < 0.02 and pz < 0.004 and pxy <= 1e-6
    v, pz, pxy = _offset_run((0.2, 0.2, 0.2))
    print(f"velocity offset on every axis: v error {v:.3e}, p_z error {pz:.3e}, |p_xy error - offset| {pxy:.3e}")
    assert v < 0.1 * 0.2 * np.sqrt(3.0) and pz < 0.004


@pytest.mark.parametrize("kind", ["real", "edge"])
def test_covariance(kind):
    case = C.real_case() if kind == "real" else C.edge_case(65, 25, True)
    ops = C.operands(case)
    B, T = ops["imu"].shape[:2]
    state, worst = None, 0.0
    for t in range(T):
        row = {k: (v[:, t:t + 1] if k in ("imu", "q", "qd", "contact_log", "trust") and v is not None else v) for k, v in ops.items()}
        o = estimator.estimate_track_host(**row, state=state, delta=DELTA)
        if state is not None:                                                   # sigma of the row against the prior the row started from
            P0 = state[:, 22:130].reshape(B, 3, 6, 6)
            prior = np.sqrt(np.concatenate([P0[:, :, 0, 0], P0[:, :, 1, 1]], axis=-1))
            assert (o["sigma"][:, 0] <= prior).all()
        state = o["state"]
        P = state[:, 22:130].reshape(B, 3, 6, 6)
        assert np.array_equal(P, np.transpose(P, (0, 1, 3, 2)))
        worst = min(worst, float(np.linalg.eigvalsh(P).min()))
    print("smallest eigenvalue of P over the rows", worst)
    assert worst > -1e-12


@pytest.mark.parametrize("kind", ["real", "edge"])
def test_pieces(kind):
    case = C.real_case() if kind == "real" else C.edge_case(65, 25, True)
    ops = C.operands(case)
    cut = lambda s: {k: (v[:, s] if k in ("imu", "q", "qd", "contact_log", "trust") and v is not None else v) for k, v in ops.items()}
    whole = estimator.estimate_track_host(**ops, delta=DELTA)
    a = estimator.estimate_track_host(**cut(slice(0, 13)), delta=DELTA)
    b = estimator.estimate_track_host(**cut(slice(13, 25)), state=a["state"], delta=DELTA)
    for k in estimator.OUT:
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), whole[k]), k
    assert np.array_equal(b["state"], whole["state"]) and (whole["state"][:, 130] == 1.0).all()


def test_poison_host():
    case = C.edge_case(65, 25, True)
    ops = C.operands(case)
    clean = estimator.estimate_track_host(**ops, delta=DELTA)
    imu = ops["imu"].copy()
    imu[7, 11, 4] = np.nan
    o = estimator.estimate_track_host(**dict(ops, imu=imu), delta=DELTA)
    others = np.arange(65) != 7
    for k in estimator.OUT:
        assert np.array_equal(o[k][others], clean[k][others]) and np.array_equal(o[k][7, :11], clean[k][7, :11]) and np.isnan(o[k][7, 11:]).all()
    assert np.isnan(o["state"][7]).all() and np.array_equal(o["state"][others], clean["state"][others])


def test_imu_log_host():
    rng = np.random.default_rng(3)
    B, T, m = 5, 4, lite3_model._BODY[0]
    actual = rng.normal(0.0, 0.3, (B, T, 12))
    feet = rng.normal(0.0, 0.2, (B, T, 4, 3))
    R = plant.quat_to_matrix(plant.rotvec_to_quat(actual[..., 0:3]))
    # a flight row reads zero specific force, exactly
    imu = estimator.imu_log_host(actual, np.zeros((B, T, 12)), feet)
    assert np.array_equal(imu[..., 3:6], np.zeros((B, T, 3)))
    np.testing.assert_allclose(imu[..., 0:3], np.einsum("btji,btj->bti", R, actual[..., 6:9]), rtol=0, atol=1e-15)
    # standing under forces that balance gravity: R^T (0, 0, 9.81)
    stand = np.zeros((B, T, 4, 3))
    stand[..., 2] = m * 9.81 / 4.0
    imu = estimator.imu_log_host(actual, stand.reshape(B, T, 12), feet)
    np.testing.assert_allclose(imu[..., 3:6], 9.81 * R[..., 2, :], rtol=0, atol=1e-13)
    # a pushed row reads the pushed acceleration: the plant's right-hand side with the push's wrench
    forces = rng.normal(0.0, 20.0, (B, T, 12))
    wr = rng.normal(0.0, 10.0, (B, T, 6))
    acc = lite3_model.plant_base_acc_host(actual, forces, feet, wrench=wr)
    unpushed = lite3_model.plant_base_acc_host(actual, forces, feet)
    np.testing.assert_allclose(acc[..., 3:6] - unpushed[..., 3:6], wr[..., 0:3] / m, rtol=0, atol=1e-12)
    imu = estimator.imu_log_host(actual, forces, feet, base_acc=acc)
    np.testing.assert_allclose(imu[..., 3:6], np.einsum("btji,btj->bti", R, acc[..., 3:6] + np.array([0.0, 0.0, 9.81])), rtol=0, atol=1e-12)
    # base_acc = None is the unpushed right-hand side
    np.testing.assert_allclose(estimator.imu_log_host(actual, forces, feet), estimator.imu_log_host(actual, forces, feet, base_acc=unpushed),
                               rtol=0, atol=1e-12)
    # bias and noise are added as given; a NaN makes its row NaN and no other
    bias, noise = rng.normal(0.0, 0.01, (B, 6)), rng.normal(0.0, 0.05, (B, T, 6))
    full = estimator.imu_log_host(actual, forces, feet, bias=bias, noise=noise)
    np.testing.assert_allclose(full, estimator.imu_log_host(actual, forces, feet) + bias[:, None] + noise, rtol=0, atol=1e-13)
    noise[2, 1, 0] = np.nan
    bad = estimator.imu_log_host(actual, forces, feet, bias=bias, noise=noise)
    keep = np.ones((B, T), bool)
    keep[2, 1] = False
    assert np.isnan(bad[2, 1]).all() and np.array_equal(bad[keep], full[keep])


def test_estimator_row():
    assert estimator.estimator_row() == estimator.DEFAULTS
    for kw in ({"gravity": 9.81}, {"kappa": -1.0}, {"r_v": float("nan")}, {"q_f": -1e-9}, {"nope": 1.0}):
        with pytest.raises(ValueError):
            estimator.estimator_row(**kw)


def test_growth_recorded():
    g = C.growth()
    print("recorded growth", g)
    assert 1.0 <= g and abs(C.measure_growth() - g) <= 1e-3 * g


def test_estimate_abi_table_matches_the_header():
    """The binding's table of include/mpcqp_estimate.h against the header's prototypes and struct, as tests/test_capi.py holds the
    other tables; the product library exports the header and its defaults are the host's."""
    import ctypes
    import re

    import mpcqp
    import test_capi as tc
    capi = mpcqp._capi
    protos = tc._prototypes(capi.ESTIMATE_HEADER)
    table = {name: (restype, argtypes) for name, restype, argtypes in capi.ESTIMATE_ABI[capi.ESTIMATE_HEADER]}
    assert set(table) == set(protos) == set(capi.ESTIMATE_SYMBOLS) and len(protos) == 3
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is tc._C_RETURN[ret] and len(argtypes) == len(params), name
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            ctype = decl.rsplit(" ", 1)[0]
            if "*" in ctype or ctype == "mpcqp_handle":
                assert tc._is_pointer_type(t), (name, i, decl, t)
            else:
                assert t is tc._C_INTEGER[ctype], (name, i, decl, t)
    text = open(tc.os.path.join(tc.REPO, "include", capi.ESTIMATE_HEADER)).read()
    body = re.search(r"typedef struct MpcQpEstimator \{(.*?)\} MpcQpEstimator;", text, re.S).group(1)
    fields = [n for decl in re.findall(r"^\s*(?:uint32_t|double) ([^;]*);", body, re.M) for n in re.split(r",\s*", decl)]
    assert fields == [name for name, _ in capi.MpcQpEstimator._fields_] and fields[1:] == list(estimator.DEFAULTS)
    assert ctypes.sizeof(capi.MpcQpEstimator) == 8 + 8 * len(estimator.DEFAULTS) and capi.EST_STATE == estimator.EST_STATE == 131
    assert "#define MPCQP_EST_STATE 131" in text
    lib = mpcqp.product_library()
    assert lib.has_estimate and all(lib.calls[name][0] is not None for name in capi.ESTIMATE_SYMBOLS)
    par = lib.default_estimator()
    assert par.size == ctypes.sizeof(capi.MpcQpEstimator) and {k: getattr(par, k) for k in estimator.DEFAULTS} == estimator.DEFAULTS
