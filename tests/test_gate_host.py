"""The estimator's per-leg trust gate on the host (include/mpcqp_gate.h; estimator.estimate_track_host and
gaits.rollout_observe_host with gate=); the cases and the conditions are in tests/gate_cases.py.  No GPU.

  1. The rule: open thresholds are the ungated filter bit for bit; the gated call's "trust" replays through the ungated filter bit for
     bit, in both I/O roundings; pieces chained through `state`; poison; the independent 18-state form handed the gated trust.
  2. In the loop equals after the fact: estimate_track_host(gate=) on the gated closed loop's own sensor logs.
  3. What the gate does: the conditions on ground 1e3 and on ground 0.3, log pass and closed loop.
  4. The thresholds' checks and the binding's table of include/mpcqp_gate.h against the header.
"""
import ctypes

import numpy as np
import pytest

import gate_cases as G
import mpcqp
from mpcqp import estimator

KEYS = estimator.OUT + ("state",)


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _ice_ops(noise=False):
    o = G.slip_run(G.ICE)
    imu, q, qd = G.sensors(G.ICE, noise)
    return dict(imu=imu, q=q, qd=qd, contact_log=o["contact_log"], init=o["actual"][:, 0], delta=G.DELTA)


# ------------------------------------------------------------------------------------------------------------------------ 1. the rule
def test_open_gate_is_the_ungated_filter():
    ops = _ice_ops()
    plain, opened = estimator.estimate_track_host(**ops), estimator.estimate_track_host(**ops, gate=G.OPEN)
    assert _same(plain, opened)
    assert np.array_equal(opened["trust"], (np.asarray(ops["contact_log"]) != 0).astype(np.float64))
    given = np.random.default_rng(3).uniform(0.0, 1.0, opened["trust"].shape)
    a, b = estimator.estimate_track_host(**ops, trust=given), estimator.estimate_track_host(**ops, trust=given, gate=G.OPEN)
    assert _same(a, b) and np.array_equal(b["trust"], given)
    assert set(opened) == set(plain) | {"trust", "gate_d"}


@pytest.mark.parametrize("io", [np.float64, np.float32])
def test_trust_replays_through_the_ungated_filter(io):
    ops = _ice_ops(noise=True)
    gated = estimator.estimate_track_host(**ops, gate=G.GATE, io_dtype=io)
    w = gated["trust"]
    stance = np.asarray(ops["contact_log"]) != 0
    assert (w[stance] < 1).any() and ((w > 0) & (w < 1))[stance].any() and (w[stance] == 1).any() and not w[~stance].any()
    assert np.array_equal(w, w.astype(io).astype(np.float64))                  # rounded through the I/O type
    assert _same(estimator.estimate_track_host(**ops, trust=w), gated)
    if io is np.float32:                                                        # ... once: the fp64 trust is another filter
        assert not np.array_equal(w, estimator.estimate_track_host(**ops, gate=G.GATE)["trust"])


def test_the_rule_by_hand():
    """Row 0 of a fresh filter: v = init's, P_vv = p0_v, so d and w follow from rhod alone."""
    ops = _ice_ops()
    row = {k: (v[:, :1] if k in ("imu", "q", "qd", "contact_log") else v) for k, v in ops.items()}
    from mpcqp import plant
    R = plant.quat_to_matrix(plant.rotvec_to_quat(np.asarray(ops["init"])[:, 0:3]))
    _, rhod = estimator.leg_kinematics(row["q"][:, 0], row["qd"][:, 0], R, row["imu"][:, 0, 0:3])
    e = -rhod[:, :, :2] - np.asarray(ops["init"])[:, None, 9:11]
    d = (e[..., 0] * e[..., 0]) / (1.0 + 0.1) + (e[..., 1] * e[..., 1]) / (1.0 + 0.1)
    lo, hi = (float(v) for v in np.quantile(d, [0.25, 0.75]))                   # thresholds that split these 32 legs three ways
    got = estimator.estimate_track_host(**row, gate={"d_lo": lo, "d_hi": hi})
    g = np.clip((hi - d) / (hi - lo), 0.0, 1.0)
    assert np.array_equal(got["gate_d"][:, 0], d)
    assert np.allclose(got["trust"][:, 0], (row["contact_log"][:, 0] != 0) * g, rtol=0, atol=1e-15)
    assert (g == 0).any() and (g == 1).any() and ((g > 0) & (g < 1)).any()


def test_pieces_and_poison():
    ops = _ice_ops(noise=True)
    rowwise = ("imu", "q", "qd", "contact_log")
    whole = estimator.estimate_track_host(**ops, gate=G.GATE)
    part = lambda s: {k: (v[:, s] if k in rowwise else v) for k, v in ops.items()}
    a = estimator.estimate_track_host(**part(slice(0, 13)), gate=G.GATE)
    b = estimator.estimate_track_host(**part(slice(13, 25)), gate=G.GATE, state=a["state"])
    for k in estimator.OUT + ("trust",):
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), whole[k][:, :25]), k
    bad = dict(ops, qd=ops["qd"].copy())
    bad["qd"][2, 7, 1, 0] = np.inf
    out = estimator.estimate_track_host(**bad, gate=G.GATE)
    others = np.arange(G.GAIT_B) != 2
    for k in estimator.OUT + ("trust",):
        assert np.isnan(out[k][2, 7:]).all() and np.array_equal(out[k][2, :7], whole[k][2, :7]), k
        assert np.array_equal(out[k][others], whole[k][others]), k
    assert np.isnan(out["state"][2]).all() and np.array_equal(out["state"][others], whole["state"][others])


def test_independent_form_with_the_gated_trust():
    import estimate_cases as C
    ops = _ice_ops(noise=True)
    gated = estimator.estimate_track_host(**ops, gate=G.GATE)
    joint = estimator.estimate_joint_host(**ops, trust=gated["trust"])
    for k in estimator.OUT:
        err, band = C.error(gated[k], joint[k], "f64")
        print(f"{k}: error {err:.3e}, band {band:.3e}")
        assert err <= band, k


# ------------------------------------------------------------------------------------------- 2. in the loop equals after the fact
def test_in_the_loop_equals_after_the_fact():
    o = G.closed_loop_host(G.ICE, True)
    rep = estimator.estimate_track_host(o["imu"], o["q_enc"], o["qd_enc"], o["contact_log"], o["actual"][:, 0], delta=G.DELTA, gate=G.GATE)
    for k, src in (("est", "est"), ("feet_est", "feet"), ("sigma", "sigma"), ("nis", "nis"), ("trust", "trust"), ("est_state", "state")):
        assert np.array_equal(o[k], rep[src], equal_nan=True), k
    stance = np.asarray(o["contact_log"]) != 0
    assert (o["trust"][stance] < 1).any() and np.isfinite(o["trust"]).all()
    plain = G.closed_loop_host(G.ICE, False)
    assert "trust" not in plain and set(o) == set(plain) | {"trust"}


# ------------------------------------------------------------------------------------------------------------ 3. what the gate does
@pytest.mark.parametrize("noise", [False, True])
def test_firm_ground_is_left_alone(noise):
    o = G.slip_run(G.FIRM)
    plain, gated = G.log_pass(G.FIRM, noise, False), G.log_pass(G.FIRM, noise, True)
    _, live = G.sliding(o)
    dmax = float(gated["gate_d"][live].max())
    print(f"ground 1e3, noise {noise}: largest d over {int(live.sum())} stance leg-rows {dmax:.3f}")
    assert dmax < G.GATE["d_lo"]
    assert np.array_equal(gated["trust"], (np.asarray(o["contact_log"]) != 0).astype(np.float64))
    assert _same(plain, gated)


def test_ice_log_pass():
    o = G.slip_run(G.ICE)
    plain, gated = G.log_pass(G.ICE, False, False), G.log_pass(G.ICE, False, True)
    slid, live = G.sliding(o)
    w = gated["trust"]
    print(f"ground 0.3: {int((w[slid] < 1).sum())} of {int(slid.sum())} sliding stance leg-rows flagged, "
          f"{int((w[live & ~slid] < 1).sum())} of {int((live & ~slid).sum())} held ones")
    assert slid.sum() > 0 and (w[slid] < 1).any()
    assert not (w[live & ~slid] < 1).any()                                      # every flagged leg-row is one the plant marks sliding
    v0, v1 = G.rms_vxy(plain["est"], o["actual"]), G.rms_vxy(gated["est"], o["actual"])
    p0, p1 = G.rms_pz(plain["est"], o["actual"]), G.rms_pz(gated["est"], o["actual"])
    for b, n in enumerate(G.NAMES):
        print(f"  {n:12s} RMS v_xy error {1e3 * v0[b]:6.1f} -> {1e3 * v1[b]:6.1f} mm/s ({v0[b] / v1[b]:.2f} x), p_z {1e3 * p0[b]:6.2f} -> "
              f"{1e3 * p1[b]:6.2f} mm")
    for n in G.HALVED:
        b = G.NAMES.index(n)
        assert v1[b] <= 0.5 * v0[b], n
    assert (v1 <= v0).all()


def test_ice_closed_loop():
    G.check_flying_trot("host", G.closed_loop_host(G.ICE, False), G.closed_loop_host(G.ICE, True))


# ----------------------------------------------------------------------------------------------------- 4. thresholds and the binding
def test_gate_row_checks():
    assert estimator.gate_row() == G.GATE == estimator.GATE_DEFAULTS
    assert estimator.gate_row(d_hi=9.0) == {"d_lo": 1.0, "d_hi": 9.0}
    for bad in ({"d_lo": -0.1}, {"d_lo": 4.0}, {"d_hi": 0.5}, {"d_lo": float("nan")}, {"d_hi": float("inf")}):
        with pytest.raises(ValueError, match="trust gate: d_lo and d_hi must be finite with 0 <= d_lo < d_hi"):
            estimator.gate_row(**bad)
    with pytest.raises(ValueError, match="MpcQpTrustGate has no field"):
        estimator.gate_row(d_mid=2.0)
    s = estimator.gate_struct({"d_lo": 0.5})
    assert isinstance(s, mpcqp._capi.MpcQpTrustGate) and (s.size, s.d_lo, s.d_hi) == (24, 0.5, 4.0) and estimator.gate_struct(s) is s


def test_gate_abi_table_matches_the_header():
    """The binding's table of include/mpcqp_gate.h against the header's prototypes, as tests/test_rollout_observe_host.py holds its table."""
    import test_capi as tc
    capi = mpcqp._capi
    protos = tc._prototypes(capi.GATE_HEADER)
    table = {name: (restype, argtypes) for name, restype, argtypes in capi.GATE_ABI[capi.GATE_HEADER]}
    assert set(table) == set(protos) == set(capi.GATE_SYMBOLS) == {"mpcqp_default_trust_gate", "mpcqp_estimate_track_gated",
                                                                    "mpcqp_rollout_observe_gated"}
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is tc._C_RETURN[ret] and len(argtypes) == len(params), name
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            ctype = decl.rsplit(" ", 1)[0]
            if "*" in ctype or ctype == "mpcqp_handle":
                assert tc._is_pointer_type(t), (name, i, decl, t)
            else:
                assert t is tc._C_INTEGER[ctype], (name, i, decl, t)
    # each gated call is its ungated prototype up to the last output, then gate, the trust output, stream
    for gated, header, plain, last in (("mpcqp_estimate_track_gated", capi.ESTIMATE_HEADER, "mpcqp_estimate_track", "void* nis"),
                                       ("mpcqp_rollout_observe_gated", capi.OBSERVE_HEADER, "mpcqp_rollout_observe", "void* nis_log")):
        old = tc._prototypes(header)[plain][1]
        assert protos[gated][1][:len(old) - 1] == old[:-1] and old[-2] == last
        assert protos[gated][1][len(old) - 1] == "const MpcQpTrustGate* gate" and protos[gated][1][-1] == "void* stream"
        assert len(protos[gated][1]) == len(old) + 2
    assert len(capi.ABI) == 5 and capi.GATE_HEADER not in capi.ABI
    assert ctypes.sizeof(capi.MpcQpTrustGate) == 24 and capi.MpcQpTrustGate.FIELDS == ("d_lo", "d_hi")
    lib = mpcqp.product_library()
    assert lib.has_gate and all(lib.calls[s][0] is not None for s in capi.GATE_SYMBOLS)
    g = lib.default_trust_gate()
    assert (g.size, g.d_lo, g.d_hi) == (24, 1.0, 4.0)
    assert lib.version() == 0x00010301
