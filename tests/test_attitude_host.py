"""The velocity-aided attitude rule on the host (mpcqp.estimator and mpcqp.gaits with attitude=, the counterparts of
include/mpcqp_attitude.h); the cases are in tests/attitude_cases.py.  No GPU.

  1. estimate_track_host(attitude=) equals estimate_joint_host(attitude=), the 18-state form, within tests/test_estimate_host.py's band
     (the project's 1e-9 relative, no growth factor), on the real case and on every synthetic edge.
  2. Identity: k_s = 1, k_v = k_b = 0 with a zero att_state is attitude = None as values, and gyro_bias is zero.
  3. 13 + 12 rows through `state` and `att_state` are 25 rows in one call bit for bit, also with the cut on a flight row.
  4. Replay: the aided gated call's trust fed to the aided ungated call gives the same outputs and states bit for bit.
  5. Poison: a NaN in one robot's att_state, and in one robot's imu row mid-log.
  6. What it is for: on the eight gaits the RMS tilt error at the defaults is at most half of today's filter's, and under a gyro bias of
     0.02 rad/s smaller than today's and than the gyro-only setting's.
  7. Convergence on the standing case from a tilt error of 0.1 rad and under a constant gyro bias.
  8. Parameter checks, the ABI table against the header, the recorded growth, the roll-out's host counterpart.
"""
import numpy as np
import pytest

import attitude_cases as A
import estimate_cases as C
from legsim_cases import DELTA
from mpcqp import estimator

ROWWISE = ("imu", "q", "qd", "contact_log", "trust")
# Measured on the host (see the tests' docstrings): the first rows from which the aided tilt error stays below a quarter of the
# gyro-only run's, and the rows at which that is asserted, R + 20 %.
ROW_TILT, ROW_BIAS = 150, 39


def _close(name, a, b):
    err, band = C.error(a, b, "f64")
    print(f"{name}: error {err:.3e}, band {band:.3e}")
    assert err <= band, name
    return err


def _both_forms(case):
    ops = C.operands(case)
    a = estimator.estimate_track_host(**ops, delta=DELTA, attitude=A.ATT)
    b = estimator.estimate_joint_host(**ops, delta=DELTA, attitude=A.ATT)
    return max([_close(k, a[k], b[k]) for k in A.OUT] + [_close("att_state", a["att_state"], b["att_state"])])


def test_sequential_equals_joint_real():
    """Worst error measured: 2.3e-15 relative on the real case, 6.0e-15 over the edges (nis)."""
    w = max(_both_forms(C.real_case()), _both_forms(dict(C.real_case(), height=np.zeros((16, 4)))))
    print("worst", w)


@pytest.mark.parametrize("B,T,with_height", C.edge_cases())
def test_sequential_equals_joint_edges(B, T, with_height):
    _both_forms(C.edge_case(B, T, with_height))


@pytest.mark.parametrize("kind", ["real", "edge"])
def test_identity(kind):
    case = C.real_case() if kind == "real" else C.edge_case(65, 25, True)
    ops = C.operands(case)
    B = ops["imu"].shape[0]
    plain = estimator.estimate_track_host(**ops, delta=DELTA)
    ident = estimator.estimate_track_host(**ops, delta=DELTA, attitude=A.IDENTITY, att_state=np.zeros((B, 8)))
    for k in estimator.OUT + ("state",):
        assert np.array_equal(ident[k], plain[k], equal_nan=True), k
    assert np.array_equal(ident["gyro_bias"], np.zeros((B, 25, 3))) and np.array_equal(ident["att_state"][:, 0:3], np.zeros((B, 3)))
    assert np.array_equal(ident["att_state"][:, 6:8], np.zeros((B, 2))) and np.abs(ident["att_state"][:, 3:6]).max() > 0
    aided = estimator.estimate_track_host(**ops, delta=DELTA, attitude=A.ATT)
    assert not np.array_equal(aided["est"], plain["est"]) and np.abs(aided["gyro_bias"]).max() > 0          # not vacuous


def _cut(ops, s):
    return {k: (v[:, s] if k in ROWWISE and v is not None else v) for k, v in ops.items()}


def _pieces(ops, at, **kw):
    T = ops["imu"].shape[1]
    whole = estimator.estimate_track_host(**ops, delta=DELTA, **kw)
    a = estimator.estimate_track_host(**_cut(ops, slice(0, at)), delta=DELTA, **kw)
    b = estimator.estimate_track_host(**_cut(ops, slice(at, T)), state=a["state"], att_state=a["att_state"], delta=DELTA, **kw)
    for k in A.OUT + (("trust",) if "gate" in kw else ()):
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), whole[k]), k
    assert np.array_equal(b["state"], whole["state"]) and np.array_equal(b["att_state"], whole["att_state"])
    assert np.abs(a["att_state"][:, 0:6]).min(axis=0).max() > 0                  # b^ and e_b do cross the cut


@pytest.mark.parametrize("kind", ["real", "edge"])
def test_pieces(kind):
    case = C.real_case() if kind == "real" else C.edge_case(65, 25, True)
    _pieces(C.operands(case), 13, attitude=A.ATT)
    _pieces(C.operands(case), 13, attitude=A.ATT, gate={})


def test_pieces_cut_on_a_flight_row():
    ops = dict(C.operands(C.real_case()))
    contact = ops["contact_log"].copy()
    contact[:, 9] = 0                                                            # every leg in the air on row 9, the second piece's first
    _pieces(dict(ops, contact_log=contact), 9, attitude=A.ATT)


@pytest.mark.parametrize("kind", ["real", "edge"])
def test_gated_replay(kind):
    case = C.real_case() if kind == "real" else C.edge_case(65, 25, True)
    ops = C.operands(case)
    gated = estimator.estimate_track_host(**ops, delta=DELTA, attitude=A.ATT, gate={})
    if kind == "edge":                                                           # (the real case's feet hold: its gate stays open)
        assert (gated["trust"] < ops["trust"]).any()
    rep = estimator.estimate_track_host(**dict(ops, trust=gated["trust"]), delta=DELTA, attitude=A.ATT)
    for k in A.OUT + ("state", "att_state"):
        assert np.array_equal(rep[k], gated[k]), k


def test_poison_host():
    ops = C.operands(C.edge_case(65, 25, True))
    st, att = A.live_state(65, 25, True, "f64")
    run = lambda **kw: estimator.estimate_track_host(**dict(ops, **{k: v for k, v in kw.items() if k in ops}), delta=DELTA, attitude=A.ATT,
                                                     state=kw.get("state", st), att_state=kw.get("att_state", att))
    clean = run()
    others = np.arange(65) != 7
    bad_att = att.copy()
    bad_att[7, 1] = np.nan
    o = run(att_state=bad_att)
    for k in A.OUT:
        assert np.isnan(o[k][7]).all() and np.array_equal(o[k][others], clean[k][others]), k
    imu = ops["imu"].copy()
    imu[7, 11, 4] = np.nan
    p = run(imu=imu)
    for k in A.OUT:
        assert np.array_equal(p[k][others], clean[k][others]) and np.array_equal(p[k][7, :11], clean[k][7, :11]) and np.isnan(p[k][7, 11:]).all(), k
    for r in (o, p):
        for k in ("state", "att_state"):
            assert np.isnan(r[k][7]).all() and np.array_equal(r[k][others], clean[k][others]), k
    # a fresh robot does not read att_state: its NaN row is not poison
    fresh = estimator.estimate_track_host(**ops, delta=DELTA, attitude=A.ATT, att_state=bad_att)
    assert np.array_equal(fresh["est"], estimator.estimate_track_host(**ops, delta=DELTA, attitude=A.ATT)["est"])


def test_what_it_is_for_no_bias():
    """RMS tilt error in mrad over the eight gaits (trot, flying trot, pace, bound, pronk, gallop, walk, stand), measured:
    today 25.2 31.7 52.0 60.3 19.3 69.6 23.3 25.8; aided 1.0 1.1 1.2 5.4 1.7 7.0 0.7 10.6; worst ratio 0.41, on stand."""
    import gate_cases as G
    truth = G.slip_run(G.FIRM)["actual"]
    today, aided = A.rms_tilt(A.gait_pass(0.0, "today")["est"], truth), A.rms_tilt(A.gait_pass(0.0, "aided")["est"], truth)
    for n, a, b in zip(G.NAMES, today, aided):
        print(f"{n:12s} today {1e3 * a:6.1f} mrad, aided {1e3 * b:6.1f} mrad, ratio {b / a:.3f}")
    assert (aided <= 0.5 * today).all()


def test_what_it_is_for_gyro_bias():
    """With 0.02 rad/s on all three gyro axes, RMS tilt error in mrad, measured: today 20.6 25.9 49.7 55.0 27.4 63.1 20.1 24.8; gyro only
    17.1 17.9 17.9 17.6 17.4 17.8 17.6 15.9; aided 9.0 9.4 9.4 8.4 8.9 9.6 8.7 12.6."""
    import gate_cases as G
    truth = G.slip_run(G.FIRM)["actual"]
    today, gyro, aided = (A.rms_tilt(A.gait_pass(0.02, s)["est"], truth) for s in ("today", "gyro", "aided"))
    for n, a, g, b in zip(G.NAMES, today, gyro, aided):
        print(f"{n:12s} today {1e3 * a:6.1f} mrad, gyro only {1e3 * g:6.1f} mrad, aided {1e3 * b:6.1f} mrad")
    assert (aided < today).all() and (aided < gyro).all()
    bh = A.gait_pass(0.02, "aided")["att_state"][:, 0:3]
    print("b^ at the last row", np.round(bh, 4).tolist())


def test_convergence_from_a_tilt_error():
    """The standing case started 0.1 rad off about a horizontal axis, no bias.  The gyro-only run keeps its 0.1 rad; the aided run's tilt
    error stays below a quarter of it from row R on (measured on the host: R = 125 -- the PI loop is underdamped, and the error swings back
    to 0.030 rad around row 120 before it settles below 0.011), asserted from row R + 20 % = 150."""
    a, g = A.standing_run("tilt", "aided")[0], A.standing_run("tilt", "gyro")[0]
    R = A.first_row_below_quarter("tilt")
    print(f"first row below a quarter: {R}; aided at row {ROW_TILT}: {a[:, ROW_TILT].max():.4f} rad, gyro only {g[:, ROW_TILT].min():.4f} rad; "
          f"aided at the last row {a[:, -1].max():.5f} rad")
    assert (a[:, ROW_TILT:] < 0.25 * g[:, ROW_TILT:]).all()


def test_convergence_under_a_gyro_bias():
    """The standing case with a constant gyro bias of (0.02, -0.015, 0.01) rad/s and exact init.  The gyro-only tilt grows by 0.025 rad/s;
    the aided run stays below a quarter of it from row R on (measured on the host: R = 32), asserted from row R + 20 % = 39 (rounded up).  b^'s x and
    y entries end nearer the true bias than zero is; z is printed (it is not observable)."""
    a, g = A.standing_run("bias", "aided")[0], A.standing_run("bias", "gyro")[0]
    R = A.first_row_below_quarter("bias")
    bh = A.standing_run("bias", "aided")[1]["att_state"][:, 0:3]
    print(f"first row below a quarter: {R}; aided at the last row {a[:, -1].max():.5f} rad, gyro only {g[:, -1].min():.4f} rad; b^ {np.round(bh, 4).tolist()}")
    assert (a[:, ROW_BIAS:] < 0.25 * g[:, ROW_BIAS:]).all()
    true = np.asarray(A.STAND_BIAS)
    assert (np.abs(bh[:, 0:2] - true[0:2]) < np.abs(true[0:2])).all()


def test_attitude_row():
    assert estimator.attitude_row() == estimator.ATT_DEFAULTS == A.ATT
    for k in estimator.ATT_DEFAULTS:
        for v in (-1e-9, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                estimator.attitude_row(**{k: v})
    with pytest.raises(ValueError):
        estimator.attitude_row(nope=1.0)
    ops = C.operands(C.edge_case(1, 2, False))
    for fn in (estimator.estimate_track_host, estimator.estimate_joint_host):
        with pytest.raises(ValueError):
            fn(**ops, delta=DELTA, attitude={"k_v": -1.0})
        with pytest.raises(ValueError):
            fn(**ops, delta=DELTA, att_state=np.zeros((1, 8)))


def test_growth_recorded():
    g = A.growth()
    print("recorded growth under the aided rule", g, "unaided", C.growth())
    assert 1.0 <= g and abs(A.measure_growth() - g) <= 1e-3 * g


def test_attitude_abi_table_matches_the_header():
    import ctypes
    import re

    import mpcqp
    import test_capi as tc
    capi = mpcqp._capi
    protos = tc._prototypes(capi.ATTITUDE_HEADER)
    table = {name: (restype, argtypes) for name, restype, argtypes in capi.ATTITUDE_ABI[capi.ATTITUDE_HEADER]}
    assert set(table) == set(protos) == set(capi.ATTITUDE_SYMBOLS) and len(protos) == 3
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is tc._C_RETURN[ret] and len(argtypes) == len(params), name
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            ctype = decl.rsplit(" ", 1)[0]
            if "*" in ctype or ctype == "mpcqp_handle":
                assert tc._is_pointer_type(t), (name, i, decl, t)
            else:
                assert t is tc._C_INTEGER[ctype], (name, i, decl, t)
    text = open(tc.os.path.join(tc.REPO, "include", capi.ATTITUDE_HEADER)).read()
    body = re.search(r"typedef struct MpcQpAttitude \{(.*?)\} MpcQpAttitude;", text, re.S).group(1)
    fields = [n for decl in re.findall(r"^\s*(?:uint32_t|double) ([^;]*);", body, re.M) for n in re.split(r",\s*", decl)]
    assert fields == [name for name, _ in capi.MpcQpAttitude._fields_] and fields[1:] == list(estimator.ATT_DEFAULTS)
    assert "#define MPCQP_ATT_STATE 8" in text and capi.ATT_STATE == estimator.ATT_STATE == 8
    assert re.search(r"#define MPCQP_AIDED_GATE 1\b", text) and capi.AIDED_GATE == 1
    lib = mpcqp.product_library()
    assert lib.has_attitude and all(lib.calls[name][0] is not None for name in capi.ATTITUDE_SYMBOLS)
    par = lib.default_attitude()
    assert par.size == ctypes.sizeof(capi.MpcQpAttitude) and {k: getattr(par, k) for k in estimator.ATT_DEFAULTS} == estimator.ATT_DEFAULTS


def test_rollout_observe_host_attitude():
    """The host roll-out with attitude=: feed = "truth" leaves every shared key the unaided run's, its estimator rows are the log pass's
    on its own sensor logs bit for bit, and feed = "estimate" differs from the unaided loop."""
    import gate_cases as G
    from mpcqp import gaits, lite3_model
    pb, T = G.gait_batch(), 8
    bias = np.zeros((G.GAIT_B, 6))
    bias[:, 0:3] = 0.02
    run = lambda feed, **kw: gaits.rollout_observe_host(G.checker(), *G._head(pb), T, np.full(G.GAIT_B, G.STEP_HEIGHT), np.full(G.GAIT_B, G.ICE),
                                                        lite3_model.foot_mass(), feed=feed, bias=bias, **kw)
    plain, aided = run("truth"), run("truth", attitude={}, gate={})
    assert set(aided) == set(plain) | {"gyro_bias", "att_state", "trust"}
    for k in ("x", "actual", "forces", "feet_log", "contact_log", "imu", "q_enc", "qd_enc", "slip"):
        assert np.array_equal(aided[k], plain[k]), k
    rep = estimator.estimate_track_host(aided["imu"], aided["q_enc"], aided["qd_enc"], aided["contact_log"], pb["x"][:, :12], delta=G.DELTA,
                                        attitude={}, gate={})
    for k, src in (("est", "est"), ("feet_est", "feet"), ("sigma", "sigma"), ("nis", "nis"), ("trust", "trust"), ("gyro_bias", "gyro_bias"),
                   ("est_state", "state"), ("att_state", "att_state")):
        assert np.array_equal(aided[k], rep[src]), k
    assert np.abs(aided["gyro_bias"][:, -1]).max() > 0 and not np.array_equal(aided["est"], plain["est"])
    fed = run("estimate", attitude={})
    assert not np.array_equal(fed["actual"], run("estimate")["actual"]) and "trust" not in fed
    with pytest.raises(ValueError):
        run("truth", att_state=np.zeros((G.GAIT_B, 8)))
