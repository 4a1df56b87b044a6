"""disturbance.rollout_compensated_host, the host counterpart of mpcqp_rollout_observe_compensated (include/mpcqp_compensate.h), on the
CPU checker: it is composed of what exists, so the tests are about the composition -- one piece is one roll-out and one track, no
gain is no compensation, the sensed source estimates the push -- and about the binding's table.  The cases are in
tests/compensate_cases.py.  No GPU."""
import re

import numpy as np
import pytest

import compensate_cases as K
import disturbance_cases as C
import mpcqp
from mpcqp import disturbance

LOGS = ("actual", "desired", "forces", "feet_log", "contact_log", "cmd", "est", "feet_est", "imu", "q", "tau", "flag", "slip_log", "disp")


def test_hold_of_the_whole_call_is_one_rollout_and_one_track():
    T = K.T_FIX
    for source in ("truth", "sensed"):
        got = K.host_run(source, T)
        roll = K.host_observe(T, rows="zero")
        view = disturbance.sensed_logs(roll) if source == "sensed" else roll
        track = disturbance.disturbance_track_host(view, C.checker().cfg)
        for k in LOGS + K.STATE + ("solved",):
            assert np.array_equal(got[k], roll[k], equal_nan=True), (source, k)
        assert np.array_equal(got["dist"], track["dist"]) and np.array_equal(got["resid"], track["resid"])
        assert np.array_equal(got["dist_state"], track["state"]) and np.abs(track["dist"][1:, -1, 0]).min() > 1.0


def test_without_a_gain_nothing_is_compensated():
    got, roll = K.host_run("truth", 1, K.T_FIX, kappa=0.0), K.host_observe(K.T_FIX, rows="zero")
    for k in LOGS + K.STATE + ("solved",):
        assert np.array_equal(got[k], roll[k], equal_nan=True), k
    assert not got["dist"].any() and np.abs(got["resid"][1:, 1:, 0]).min() > 1.0    # the residual sees the push, the estimate stays 0
    # and zero rows are no rows (x + 0 and xdes - 0 are exact)
    plain = K.host_observe(K.T_FIX)
    assert np.array_equal(plain["actual"], roll["actual"]) and np.array_equal(plain["forces"], roll["forces"])


def test_pieces_of_a_multiple_of_hold_are_the_uncut_call():
    pb, T = K.batch(), K.T_FIX
    whole = K.host_run("truth", 3, T)
    st = {k: pb[k] for k in ("x", "ref", "feet", "legs", "tick")}
    st.update(slip=None, est_state=None, dist_state=None)
    parts = []
    for _ in range(2):
        o = disturbance.rollout_compensated_host(C.checker(), st["x"], st["ref"], st["feet"], st["legs"], pb["gait"], pb["stand"], pb["gain"],
                                                 st["tick"], pb["mu"], T // 2, pb["step_height"], pb["ground"], pb["foot_mass"],
                                                 compensate={"hold": 3}, dist_state=st["dist_state"], slip=st["slip"], est_state=st["est_state"],
                                                 **K.host_kw(pb))
        st.update({k: o[k] for k in st})
        parts.append(o)
    for k in LOGS + ("dist", "resid"):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k], equal_nan=True), k
    for k in K.STATE + ("dist_state",):
        assert np.array_equal(parts[-1][k], whole[k]), k


def test_the_sensed_source_estimates_the_push():
    """Ground 1e3, no noise, an exact est_init, 24 ticks at hold = 1.  The sensed observer differs from the truth observer by what the
    estimator gets wrong: a residual takes m (v^ - v^_prev) / delta in the place of m (v - v_prev) / delta and the commanded forces
    in the place of the applied ones, and d^ is a convex combination of residuals, so the difference is at most
    2 m max|v^ - v| / delta + 4 max|f_cmd - f|.  Recorded on the fixture (tests/golden/compensate_fixture.npz): 2.792 N worst over the
    run against a bound of 54.7 N from a velocity error of 0.0924 m/s (the estimator takes the push's acceleration for tilt until
    its leg updates correct it); commanded and applied forces are equal there.  The recorded figure holds with the factor of two
    tests/test_disturbance_host.py gives its recorded torque error."""
    err, ev, df = K.sensed_figures()
    bound = 2.0 * C.checker().cfg.m * ev / C.DELTA + 4.0 * df
    s = K.host_run("sensed", 1, K.SENSED_T)
    last = np.abs(s["dist"][:, -1, :3] - C.PUSH[:, :3]).max()
    print(f"sensed against truth estimate {err:.4f} N (recorded {K.recorded():.4f}), bound from the estimator's error {bound:.2f} N "
          f"(velocity error {ev:.4f} m/s, commanded against applied {df:.3e} N); last row against the push {last:.3f} N")
    assert np.all(s["solved"] == K.SENSED_T)
    assert err <= bound and err <= 2.0 * K.recorded()
    assert last <= 0.8 ** (K.SENSED_T - 1) * np.abs(C.PUSH[:, :3]).max() + err


def test_argument_checks():
    for kw in ({"source": "both"}, {"hold": 0}, {"hold": 1.5}, {"kappa": 2.0}, {"gain": 1.0}):
        with pytest.raises(ValueError):
            disturbance.compensate_row(**kw)
    row = disturbance.compensate_row()
    assert row == {**disturbance.OBSERVER_DEFAULTS, "source": "truth", "hold": 1, "body": None}
    par, body = disturbance.compensate_struct({"source": "sensed", "hold": 3, "kappa": 0.5}, gated=True, aided=True)
    capi = mpcqp._capi
    assert (par.size, par.flags, par.source, par.hold) == (capi.ctypes.sizeof(capi.MpcQpCompensate), 3, capi.WRENCH_SENSED, 3) and body is None
    assert par.observer.kappa == 0.5 and par.observer.size == capi.ctypes.sizeof(capi.MpcQpWrenchObserver)


def test_abi_table_matches_the_header(oracle_lib):
    import test_capi as tc
    capi = mpcqp._capi
    protos = tc._prototypes(capi.COMPENSATE_HEADER)
    table = {name: (restype, argtypes) for name, restype, argtypes in capi.COMPENSATE_ABI[capi.COMPENSATE_HEADER]}
    assert set(table) == set(protos) == set(capi.COMPENSATE_SYMBOLS) and len(protos) == 2
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is tc._C_RETURN[ret] and len(argtypes) == len(params), name
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            ctype = decl.rsplit(" ", 1)[0]
            if "*" in ctype or ctype == "mpcqp_handle":
                assert tc._is_pointer_type(t), (name, i, decl, t)
            else:
                assert t is tc._C_INTEGER[ctype], (name, i, decl, t)
    # the call is the aided roll-out's with five more operands in front of the stream
    aided = tc._prototypes(capi.ATTITUDE_HEADER)["mpcqp_rollout_observe_aided"][1]
    assert protos["mpcqp_rollout_observe_compensated"][1][:len(aided) - 1] == aided[:-1]
    text = open(tc.os.path.join(tc.REPO, "include", capi.COMPENSATE_HEADER)).read()
    body = re.search(r"typedef struct MpcQpCompensate \{(.*?)\} MpcQpCompensate;", text, re.S).group(1)
    fields = re.findall(r"^\s*(?:uint32_t|int32_t|MpcQpWrenchObserver) (\w+);", body, re.M)
    assert fields == [name for name, _ in capi.MpcQpCompensate._fields_]
    for macro, value in (("WRENCH_TRUTH", capi.WRENCH_TRUTH), ("WRENCH_SENSED", capi.WRENCH_SENSED), ("COMP_GATED", capi.COMP_GATED),
                         ("COMP_AIDED", capi.COMP_AIDED)):
        assert int(re.search(rf"#define MPCQP_{macro} (\d+)", text).group(1)) == value
    plib = mpcqp.product_library()
    assert plib.has_compensate and not oracle_lib.has_compensate
    for name, restype, argtypes in capi.COMPENSATE_ABI[capi.COMPENSATE_HEADER]:
        fn = getattr(plib.lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    par = plib.default_compensate()                                             # (no GPU call: the defaults are host code)
    assert (par.size, par.flags, par.source, par.hold) == (capi.ctypes.sizeof(capi.MpcQpCompensate), 0, capi.WRENCH_TRUTH, 1)
    assert {k: getattr(par.observer, k) for k in disturbance.OBSERVER_DEFAULTS} == disturbance.OBSERVER_DEFAULTS
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    with pytest.raises(mpcqp.MpcQpError, match=r"does not export include/mpcqp_compensate.h \(product library only\)"):
        eng.rollout_observe_compensated_ptr(*([1] * 62))
