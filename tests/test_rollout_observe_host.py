"""The slip roll-out with the estimator inside its tick loop, on the host (gaits.rollout_observe_host, the counterpart of
include/mpcqp_observe.h); the cases are in tests/observe_cases.py.  No GPU.

  1. feed="truth" is rollout_slip_host on every shared key, bit for bit.
  2. For both feeds, without and with height rows, estimate_track_host on the returned sensor logs reproduces the four estimator logs
     and est_state bit for bit, finite on every robot without a poisoned leg-row.
  3. The host encoders are the q / qd logs where the slip entry is zero (and the leg-row is not poisoned).
  4. The six-robot feedback case: what reading the estimate does to the regulated height, without and with height rows.
  5. The binding's table of include/mpcqp_observe.h against the header: one prototype and the two MPCQP_FEED_* defines.
"""
import re

import numpy as np
import pytest

import drive_cases as dc
import mpcqp
import observe_cases as oc
from legsim_cases import DELTA, ROLL_B, ROLL_T, STEP_HEIGHT, rollout_batch
from mpcqp import estimator, gaits, lite3_model

_CACHE = {}


def _engine(oracle_lib):
    return mpcqp.Engine(oracle_lib, oracle_lib.default_config(N=10, delta=DELTA, max_iter=4000))


def _runs(oracle_lib):
    """The legsim batch on ground 0.3 under the even robots with tau_max x 0.5: rollout_slip_host and both feeds, each without and
    with height rows, once; keys "slip" and (feed, with_height)."""
    if "runs" not in _CACHE:
        eng = _engine(oracle_lib)
        pb, rows = rollout_batch()
        sens = oc.sensor_draw()
        a = [pb[k] for k in ("x", "ref", "feet")] + [np.zeros((ROLL_B, 4, 7))] + [pb[k] for k in ("gait", "stand", "gain", "tick", "mu")]
        tail = (ROLL_T, np.full(ROLL_B, STEP_HEIGHT), oc.ground_rows(), lite3_model.foot_mass())
        kw = {"body": rows["body"], "push": rows["push"], "push_ticks": rows["push_ticks"], "inertia": dc.weak_row(0.5)}
        height = pb["stand"][:, :, 2].copy()
        obs = {k: sens[k] for k in ("bias", "noise", "enc_noise")}
        runs = {"slip": gaits.rollout_slip_host(eng, *a, *tail, **kw)}
        for feed in ("truth", "estimate"):
            for with_height in (False, True):
                runs[(feed, with_height)] = gaits.rollout_observe_host(eng, *a, *tail, feed=feed, height=height if with_height else None,
                                                                       **obs, **kw)
        _CACHE["runs"] = (pb, runs, height)
    return _CACHE["runs"]


def test_truth_feed_is_rollout_slip_host(oracle_lib):
    _, runs, _ = _runs(oracle_lib)
    slip = runs["slip"]
    for with_height in (False, True):
        truth = runs[("truth", with_height)]
        assert set(truth) == set(slip) | set(oc.EST_LOGS) | {"est_state"}
        for k, v in slip.items():
            assert np.array_equal(v, truth[k], equal_nan=True), k
        assert not np.array_equal(runs[("estimate", with_height)]["forces"], slip["forces"])
    assert int(((slip["flag"] & 128) != 0).sum()) > 0


@pytest.mark.parametrize("with_height", [True, False])
@pytest.mark.parametrize("feed", ["truth", "estimate"])
def test_in_the_loop_equals_after_the_fact(oracle_lib, feed, with_height):
    pb, runs, height = _runs(oracle_lib)
    o = runs[(feed, with_height)]
    rep = estimator.estimate_track_host(o["imu"], o["q_enc"], o["qd_enc"], o["contact_log"], o["actual"][:, 0],
                                        height=height if with_height else None, state=np.zeros((ROLL_B, estimator.EST_STATE)), delta=DELTA)
    ok = ~(o["flag"] == 0xff).any(axis=(1, 2))                                      # robots without a poisoned leg-row
    assert ok.sum() >= (3 * ROLL_B) // 4
    for k, src in (("est", "est"), ("feet_est", "feet"), ("sigma", "sigma"), ("nis", "nis")):
        assert np.array_equal(o[k], rep[src], equal_nan=True) and np.isfinite(o[k][ok]).all(), k
    assert np.array_equal(o["est_state"], rep["state"], equal_nan=True) and np.isfinite(o["est_state"][ok]).all()
    assert (o["est_state"][ok, 130] == 1.0).all()


@pytest.mark.parametrize("feed", ["truth", "estimate"])
def test_encoders_are_the_joint_logs_where_no_foot_slides(oracle_lib, feed):
    _, runs, _ = _runs(oracle_lib)
    o = runs[(feed, True)]
    quiet = ~oc.sensor_draw()["noisy"][:, None, None] & ~o["slip_log"].any(axis=-1) & (o["flag"] != 0xff)
    sliding = o["slip_log"].any(axis=-1) & (o["contact_log"] != 0)
    print(f"{feed}: {int(quiet.sum())} quiet leg-rows, {int(sliding.sum())} sliding stance leg-rows")
    assert quiet.sum() > 200 and sliding.sum() > 0
    assert np.array_equal(o["q_enc"][quiet], o["q"][quiet]) and np.array_equal(o["qd_enc"][quiet], o["qd"][quiet])
    assert not np.array_equal(o["qd_enc"][sliding & ~oc.sensor_draw()["noisy"][:, None, None]],
                              o["qd"][sliding & ~oc.sensor_draw()["noisy"][:, None, None]])


def test_what_the_feedback_does(oracle_lib):
    eng = _engine(oracle_lib)
    pb = oc.feedback_batch()
    a = [pb[k] for k in ("x", "ref", "feet", "legs", "gait", "stand", "gain", "tick", "mu")]
    run = lambda **kw: gaits.rollout_observe_host(eng, *a, oc.FEED_T, pb["step_height"], pb["ground"], pb["foot_mass"], feed="estimate",
                                                  est_init=pb["est_init"], land="rule", **kw)
    blind, seen = run(), run(height=pb["height"])
    oc.check_feedback("host", (blind["actual"], blind["est"]), (seen["actual"], seen["est"]), blind["solved"], seen["solved"])


def test_observe_abi_table_matches_the_header():
    """The binding's table of include/mpcqp_observe.h against the header's prototype, as tests/test_estimate_host.py holds its table."""
    import test_capi as tc
    capi = mpcqp._capi
    protos = tc._prototypes(capi.OBSERVE_HEADER)
    table = {name: (restype, argtypes) for name, restype, argtypes in capi.OBSERVE_ABI[capi.OBSERVE_HEADER]}
    assert set(table) == set(protos) == set(capi.OBSERVE_SYMBOLS) == {"mpcqp_rollout_observe"}
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is tc._C_RETURN[ret] and len(argtypes) == len(params), name
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            ctype = decl.rsplit(" ", 1)[0]
            if "*" in ctype or ctype == "mpcqp_handle":
                assert tc._is_pointer_type(t), (name, i, decl, t)
            else:
                assert t is tc._C_INTEGER[ctype], (name, i, decl, t)
    # every argument of mpcqp_rollout_slip, in its order, up to disp_log
    slip = tc._prototypes(capi.SLIP_HEADER)["mpcqp_rollout_slip"][1]
    assert protos["mpcqp_rollout_observe"][1][:len(slip) - 1] == slip[:-1] and slip[-2] == "void* disp_log"
    text = open(tc.os.path.join(tc.REPO, "include", capi.OBSERVE_HEADER)).read()
    defines = dict(re.findall(r"^#define (MPCQP_FEED_[A-Z]+) (\d+)", text, re.M))
    assert defines == {"MPCQP_FEED_TRUTH": str(capi.FEED_TRUTH), "MPCQP_FEED_ESTIMATE": str(capi.FEED_ESTIMATE)}
    assert '#include "mpcqp_slip.h"' in text and '#include "mpcqp_estimate.h"' in text
    lib = mpcqp.product_library()
    assert lib.has_observe and lib.calls["mpcqp_rollout_observe"][0] is not None
