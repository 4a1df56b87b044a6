"""The velocity-aided attitude rule on the device (include/mpcqp_attitude.h, mpcqp_estimate_track_aided and
mpcqp_rollout_observe_aided) against its host counterparts; the cases are in tests/attitude_cases.py.  Every test calls the new entry
points unconditionally: a library without them fails here, it does not skip.

Log pass (estimate_track(attitude=...)):
  1. Device against host, both I/O dtypes: the real 16 x 25 case and the synthetic edges at B in {1, 15, 16, 17, 63, 64, 65, 257} x T in
     {1, 2, 25}, each without and with the gate, without and with height, and from a live state with a non-zero att_state.  The band is
     the project's (1e-9 relative in fp64, two float32 spacings in fp32 I/O) times the recorded growth of the aided rule
     (tests/golden/attitude_growth.npz).
  2. Bit for bit: the same call twice; 2560 shuffled robots against the 16; 13 + 12 rows through `state` and `att_state` against one
     call; bias_log = NULL changes no other output.
  3. Poison through att_state and through an imu row.
  4. The ABI: argument errors that name the entry point, no-ops.
Roll-out (rollout_observe(attitude=...)) at B in {16, 65}, T = 12, trot and flying trot rows, ground 0.3, bias and noise on the odd robots:
  5. feed = "truth" is rollout_slip bit for bit in state and every shared log.
  6. estimate_track(attitude=) on the roll-out's own sensor logs reproduces its estimator logs and both states bit for bit, gated and ungated.
  7. feed = "estimate" against gaits.rollout_observe_host(attitude={}) (f64 I/O): the closed loop is held as tests/test_gpu_rollout_observe.py
     holds the unaided pair's (observe_cases.check_feedback): the CoM and its estimate within 5 mm of the host's, every tick solved.
"""
import numpy as np
import pytest

import attitude_cases as A
import estimate_cases as C
import mpcqp
import observe_cases as oc
import test_gpu_rollout_observe as ro
from legsim_cases import DELTA
from mpcqp import estimator, gaits, lite3_model

pytestmark = pytest.mark.gpu

_t, _np = ro._t, ro._np
_ENGINES, _CACHE = {}, {}
ROWWISE = ("imu", "q", "qd", "contact_log", "trust")
STATES = ("state", "att_state")
ROLL_T, ICE = 12, 0.3


def _sol(io):
    if io not in _ENGINES:
        _ENGINES[io] = mpcqp.MPCBatch(N=10, delta=DELTA, io_dtype=io)
    return _ENGINES[io]


def _track(sol, ops, state=None, att_state=None, attitude=A.ATT, **kw):
    """estimate_track(attitude=) on host operands -> numpy outputs; `state` and `att_state` (numpy, None = zeros) come back advanced."""
    import torch
    d = {k: _t(v, torch.uint8 if k == "contact_log" else sol.tdtype) for k, v in ops.items()}
    B = d["imu"].shape[0]
    st = _t(np.zeros((B, 131)) if state is None else state, torch.float64)
    at = _t(np.zeros((B, 8)) if att_state is None else att_state, torch.float64)
    out = sol.estimate_track(d["imu"], d["q"], d["qd"], d["contact_log"], d["init"], trust=d["trust"], height=d["height"], state=st,
                             attitude=attitude, att_state=at, **kw)
    torch.cuda.synchronize()
    assert out["att_state"] is at
    res = {k: (None if v is None else _np(v)) for k, v in out.items()}
    res["state"] = _np(st)
    return res


def _check(tag, dev, host, io, keys):
    g = A.growth()
    worst = 0.0
    for k in keys + STATES:
        err, band = C.error(dev[k], host[k], "f64" if k in STATES else io)
        print(f"{tag} {io} {k}: error {err:.3e}, band {band * g:.3e} (growth {g:.1f})")
        assert err <= band * g, (tag, k)
        worst = max(worst, err / band)
    return worst


def _variants(case, B, T, io):
    """(tag, operands, extra keywords of both forms) of a case: without / with the gate, without / with height, and from a live state
    with a non-zero att_state."""
    ops = C.operands(case)
    hz = ops["height"] if ops["height"] is not None else C.r32(np.random.default_rng(B + T).normal(0.0, 0.01, (B, 4)))
    for gate in (None, {}):
        for h in (None, hz):
            yield f"gate={gate is not None} height={h is not None}", dict(ops, height=h), ({} if gate is None else {"gate": gate})
    st, att = A.live_state(B, T, ops["height"] is not None, io)
    yield "live state", ops, {"gate": {}, "state": st, "att_state": att}


def _against_host(tag, case, io):
    sol = _sol(io)
    case = C.as_io(case, io)
    B, T = case["imu"].shape[:2]
    npio = np.float64 if io == "f64" else np.float32
    worst = 0.0
    for what, ops, kw in _variants(case, B, T, io):
        host = estimator.estimate_track_host(**ops, delta=DELTA, attitude=A.ATT, io_dtype=npio, **kw)
        dev = _track(sol, ops, **kw)
        assert set(dev) == set(estimator.OUT) | {"gyro_bias", "att_state", "state"} | ({"trust"} if "gate" in kw else set())
        worst = max(worst, _check(f"{tag} {what}", dev, host, io, A.OUT + (("trust",) if "gate" in kw else ())))
        live = ~np.isnan(dev["state"]).any(axis=1)
        assert (dev["state"][live, 130] == 1.0).all() and not dev["att_state"][live, 6:8].any()
    print(f"{tag} {io}: worst error / band {worst:.3e}")


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_track_against_host_real(io):
    """Measured on an MI355X, worst error over the one-row band: see DESIGN.md (the aided rule's section)."""
    _against_host("real", C.real_case(), io)


@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("B,T", A.edge_pairs())
def test_track_against_host_edges(io, B, T):
    _against_host(f"edge {B}x{T}", C.edge_case(B, T, (B + T) % 2 == 1), io)


def _equal(a, b, keys):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_repeat_shuffle_pieces_and_null_bias_log(io):
    import torch
    sol = _sol(io)
    ops = C.operands(C.as_io(C.real_case(), io))
    keys = A.OUT + ("trust",) + STATES
    a, b = _track(sol, ops, gate={}), _track(sol, ops, gate={})
    assert _equal(a, b, keys) and np.isfinite(a["est"]).all() and np.abs(a["gyro_bias"]).max() > 0
    # 2560 shuffled robots against the 16
    src = np.random.default_rng(5).permutation(2560) % 16
    big = _track(sol, {k: (None if v is None else v[src]) for k, v in ops.items()}, gate={})
    for k in keys:
        assert np.array_equal(big[k], a[k][src]), k
    # 13 + 12 rows through state and att_state, and a cut on a flight row
    for cut, contact in ((13, ops["contact_log"]), (9, np.where(np.arange(25)[None, :, None] == 9, 0, ops["contact_log"]).astype(np.uint8))):
        o = dict(ops, contact_log=contact)
        piece = lambda s: {k: (v[:, s] if k in ROWWISE and v is not None else v) for k, v in o.items()}
        whole = a if cut == 13 else _track(sol, o, gate={})
        p1 = _track(sol, piece(slice(0, cut)), gate={})
        p2 = _track(sol, piece(slice(cut, 25)), state=p1["state"], att_state=p1["att_state"], gate={})
        for k in A.OUT + ("trust",):
            assert np.array_equal(np.concatenate([p1[k], p2[k]], axis=1), whole[k]), (cut, k)
        assert _equal(p2, whole, STATES) and np.abs(p1["att_state"][:, 0:6]).min(axis=0).max() > 0
    # bias_log = NULL (and att_state = NULL on a fresh start) changes no other output
    d = {k: _t(v, torch.uint8 if k == "contact_log" else sol.tdtype) for k, v in ops.items()}
    p = lambda t: 0 if t is None else t.data_ptr()
    outs = [torch.empty(s, dtype=sol.tdtype, device="cuda") for s in ((16, 25, 12), (16, 25, 4, 3), (16, 25, 6), (16, 25), (16, 25, 4))]
    state = torch.zeros((16, 131), dtype=torch.float64, device="cuda")
    sol.engine.estimate_track_aided_ptr(16, 25, p(d["imu"]), p(d["q"]), p(d["qd"]), p(d["contact_log"]), 0, 0, p(d["init"]), p(state),
                                        *[p(o) for o in outs], 0, flags=mpcqp._capi.AIDED_GATE, att_state=0,
                                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k, o in zip(estimator.OUT + ("trust",), outs):
        assert np.array_equal(_np(o), a[k]), k
    assert np.array_equal(_np(state), a["state"])


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_gated_replay_and_identity(io):
    sol = _sol(io)
    case = C.as_io(C.edge_case(65, 25, True), io)
    ops = C.operands(case)
    gated = _track(sol, ops, gate={})
    assert (gated["trust"] < ops["trust"]).any()
    rep = _track(sol, dict(ops, trust=gated["trust"]))
    assert _equal(rep, gated, A.OUT + STATES)
    # k_s = 1, k_v = k_b = 0 from a zero att_state: today's call as values, and a zero gyro_bias
    import torch
    d = {k: _t(v, torch.uint8 if k == "contact_log" else sol.tdtype) for k, v in ops.items()}
    st = torch.zeros((65, 131), dtype=torch.float64, device="cuda")
    plain = sol.estimate_track(d["imu"], d["q"], d["qd"], d["contact_log"], d["init"], trust=d["trust"], height=d["height"], state=st)
    torch.cuda.synchronize()
    ident = _track(sol, ops, attitude=A.IDENTITY)
    for k in estimator.OUT:
        assert np.array_equal(ident[k], _np(plain[k])), k
    assert np.array_equal(ident["state"], _np(st)) and not ident["gyro_bias"].any() and not ident["att_state"][:, 0:3].any()


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_poison(io):
    sol = _sol(io)
    case = C.as_io(C.edge_case(65, 25, True), io)
    ops = C.operands(case)
    st, att = A.live_state(65, 25, True, io)
    clean = _track(sol, ops, state=st, att_state=att, gate={})
    keys, others = A.OUT + ("trust",), np.arange(65) != 7
    bad = att.copy()
    bad[7, 2] = np.nan
    o = _track(sol, ops, state=st, att_state=bad, gate={})
    imu = ops["imu"].copy()
    imu[7, 11, 4] = np.nan
    p = _track(sol, dict(ops, imu=imu), state=st, att_state=att, gate={})
    for k in keys:
        assert np.isnan(o[k][7]).all() and np.array_equal(o[k][others], clean[k][others]), k
        assert np.isnan(p[k][7, 11:]).all() and np.array_equal(p[k][7, :11], clean[k][7, :11]) and np.array_equal(p[k][others], clean[k][others]), k
    for r in (o, p):
        for k in STATES:
            assert np.isnan(r[k][7]).all() and np.array_equal(r[k][others], clean[k][others]), k
    fresh = _track(sol, ops, att_state=bad)                                     # a fresh robot does not read its att_state row
    assert _equal(fresh, _track(sol, ops), A.OUT + STATES)


def _att(**kw):
    a = mpcqp.product_library().default_attitude()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD_ATT = [(dict(size=8), "attitude struct size mismatch"), (dict(k_v=-1.0), "attitude: k_s, k_v, k_b and b_max"),
           (dict(k_s=float("nan")), "attitude: k_s, k_v, k_b and b_max"), (dict(b_max=float("inf")), "attitude: k_s, k_v, k_b and b_max"),
           (dict(k_b=-1e-9), "attitude: k_s, k_v, k_b and b_max")]


def test_arguments_and_empty_calls(oracle_lib):
    import torch
    sol = _sol("f64")
    eng, B, T = sol.engine, 3, 2
    ops = C.operands(C.edge_case(17, 2, True))
    d = {k: _t(v[:B], torch.uint8 if k == "contact_log" else sol.tdtype) for k, v in ops.items()}
    p = lambda t: t.data_ptr()
    outs = [torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((B, T, 12), (B, T, 4, 3), (B, T, 6), (B, T), (B, T, 4), (B, T, 3))]
    state, att = torch.zeros((B, 131), dtype=torch.float64, device="cuda"), torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    good = dict(B=B, T=T, imu=p(d["imu"]), q=p(d["q"]), qd=p(d["qd"]), contact_log=p(d["contact_log"]), trust=0, height=p(d["height"]),
                init=p(d["init"]), state=p(state), est=p(outs[0]), feet_est=p(outs[1]), sigma=p(outs[2]), nis=p(outs[3]), trust_out=p(outs[4]),
                bias_log=p(outs[5]), att_state=p(att))
    bad = [(dict(attitude=_att(**kw)), text) for kw, text in BAD_ATT]
    bad += [(dict(flags=2), "flags has a bit other than MPCQP_AIDED_GATE"), (dict(B=-1), "size out of range"),
            (dict(imu=0), r"null buffer \(imu, q, qd\)"),
            (dict(est=0, feet_est=0, sigma=0, nis=0, trust_out=0, bias_log=0),
             r"no output buffer \(est, feet_est, sigma, nis, trust_out and bias_log are all null\)")]
    for change, text in bad:
        with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_estimate_track_aided: " + text):
            eng.estimate_track_aided_ptr(**dict(good, **change))
    for change in (dict(B=0), dict(T=0)):                                       # no-ops
        eng.estimate_track_aided_ptr(**dict(good, **change))
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((state == 0.0).all()) and bool((att == 0.0).all())
    eng.estimate_track_aided_ptr(**dict(good, est=0, feet_est=0, sigma=0, nis=0, trust_out=0))        # bias_log alone is an output
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs[:5]) and bool(torch.isfinite(outs[5]).all()) and bool((state[:, 130] == 1.0).all())
    state.zero_(); att.zero_()
    eng.estimate_track_aided_ptr(**good)                                        # without the gate's flag trust_out is c
    torch.cuda.synchronize()
    assert torch.equal(outs[4], (d["contact_log"] != 0).to(torch.float64))
    with pytest.raises(ValueError, match="attitude: k_v must be finite and non-negative"):
        _track(sol, ops, attitude={"k_v": -2.0})
    # the roll-out's entry point: the same checks, a null att_state, and the empty calls
    rops = _roll_ops("f64", 16)
    for kw, text in BAD_ATT:
        with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_observe_aided: " + text):
            rops.observe(rops.state(), 1, "truth", attitude=_att(**kw))
    st = rops.state()
    zero = rops.observe(st, 0, "estimate", attitude={})
    torch.cuda.synchronize()
    assert zero["gyro_bias"].shape == (16, 0, 3) and not bool(zero["att_state"].any()) and not bool(st["est"].any())
    args = [1, 1] + [1] * 9 + [0, 0, 0] + [10, 1, 0, 0, 0, 1, 1, 1, 1] + [0] * 26 + [1, 1]
    with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_observe_aided: null att_state buffer"):
        eng.rollout_observe_aided_ptr(*args, att_state=0)
    oeng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    with pytest.raises(mpcqp.MpcQpError, match=r"does not export include/mpcqp_attitude.h \(product library only\)"):
        oeng.estimate_track_aided_ptr(**good)
    plib = mpcqp.product_library()
    assert plib.has_attitude and not oracle_lib.has_attitude


# ------------------------------------------------------------------------------------------------------------------------ roll-out
def _roll_batch(B):
    pb = gaits.make_phase_batch(B, ("trot", "flying_trot"), 12, seed=6)
    return pb


def _roll_ops(io, B):
    """The roll-out's operands: B robots on trot and flying trot rows, ground 0.3 under all of them, sensor draws on the odd ones."""
    if ("ops", io, B) not in _CACHE:
        ops = ro._Ops(io, B, ROLL_T, pb=_roll_batch(B), rows=None)
        ops.ground = _t(np.full(B, ICE), ops.sol.tdtype)
        _CACHE[("ops", io, B)] = ops
    return _CACHE[("ops", io, B)]


def _roll(io, B, feed, gate, attitude=A.ATT):
    import torch
    key = ("roll", io, B, feed, gate is not None, attitude is not None)
    if key not in _CACHE:
        ops = _roll_ops(io, B)
        st = ops.state()
        if attitude is not None:
            st["att"] = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
        kw = {} if attitude is None else {"attitude": attitude, "att_state": st["att"]}
        logs = ops.observe(st, ROLL_T, feed, height=ops.height, gate=gate, **kw)
        torch.cuda.synchronize()
        _CACHE[key] = (ops, st, logs)
    return _CACHE[key]


@pytest.mark.parametrize("B", [16, 65])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_truth_feed_is_rollout_slip(io, B):
    import torch
    ops, st, logs = _roll(io, B, "truth", {})
    ref_st = ops.state()
    ref = ops.slip(ref_st, ROLL_T)
    torch.cuda.synchronize()
    assert set(logs) == set(ref) | set(oc.EST_LOGS) | {"trust", "gyro_bias", "att_state"} and logs["att_state"] is st["att"]
    for k in ro.SLIP_STATE:
        assert torch.equal(st[k], ref_st[k]), k
    for k in ro.SLIP_LOGS:
        assert ro._same(logs[k], ref[k]), k
    assert int(((ref["flag"] & 128) != 0)[ref["contact_log"] != 0].sum()) > 0       # feet do slide
    assert bool(torch.isfinite(logs["gyro_bias"]).all()) and float(logs["gyro_bias"].abs().max()) > 0


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("feed", ["truth", "estimate"])
@pytest.mark.parametrize("B", [16, 65])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_in_the_loop_equals_after_the_fact(io, B, feed, gated):
    import torch
    gate = {} if gated else None
    ops, st, logs = _roll(io, B, feed, gate)
    sol = ops.sol
    ok = ~(_np(logs["flag"]) == 0xff).any(axis=(1, 2))                              # robots without a poisoned leg-row
    assert ok.sum() >= (3 * B) // 4
    okt = torch.as_tensor(ok).cuda()
    state = torch.zeros((B, 131), dtype=torch.float64, device="cuda")
    att = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    rep = sol.estimate_track(logs["imu"], logs["q_enc"], logs["qd_enc"], logs["contact_log"], logs["actual"][:, 0].contiguous(),
                             height=ops.height, state=state, gate=gate, attitude=A.ATT, att_state=att)
    torch.cuda.synchronize()
    pairs = (("est", "est"), ("feet_est", "feet"), ("sigma", "sigma"), ("nis", "nis"), ("gyro_bias", "gyro_bias")) + ((("trust", "trust"),) if gated else ())
    assert ("trust" in logs) == gated
    for k, src in pairs:
        assert torch.equal(logs[k][okt], rep[src][okt]) and bool(torch.isfinite(logs[k][okt]).all()), k
    assert torch.equal(st["est"][okt], state[okt]) and torch.equal(st["att"][okt], att[okt])
    assert float(att[okt][:, 0:6].abs().max()) > 0 and not bool(att[okt][:, 6:8].any())
    _, _, plain = _roll(io, B, feed, gate, attitude=None)
    assert not ro._same(plain["est"], logs["est"])                                  # the rule is in the loop
    # in pieces, and without logs
    ps = ops.state()
    ps["att"] = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    run = lambda n, first, **kw: ops.observe(ps, n, feed, first=first, height=ops.height, gate=gate, attitude=A.ATT, att_state=ps["att"], **kw)
    p1, p2 = run(5, 0), run(ROLL_T - 5, 5)
    torch.cuda.synchronize()
    for k in ro.SLIP_STATE + ("est", "att"):
        assert ro._same(ps[k], st[k]), k
    for k, _ in pairs:
        assert ro._same(torch.cat([p1[k], p2[k]], dim=1), logs[k]), k


@pytest.mark.parametrize("B", [16, 65])
def test_estimate_feed_against_host(B):
    """f64 I/O against gaits.rollout_observe_host(attitude={}) on the same batch.  The device solves in mixed precision and the checker to
    1e-10, so the two closed loops are not compared row by row in the one-row band; they are held as the unaided pair is
    (observe_cases.check_feedback): positions within 5 mm, every tick solved."""
    ops, st, logs = _roll("f64", B, "estimate", None)
    pb = ops.pb
    s = oc.sensor_draw(B, ROLL_T)
    lib = mpcqp.Library(C.ORACLE_SO)
    eng = mpcqp.Engine(lib, lib.default_config(N=10, delta=DELTA, max_iter=4000))
    host = gaits.rollout_observe_host(eng, pb["x"], pb["ref"], pb["feet"], np.zeros((B, 4, 7)), pb["gait"], pb["stand"], pb["gain"], pb["tick"],
                                      pb["mu"], ROLL_T, np.full(B, ro.STEP_HEIGHT), np.full(B, ICE), lite3_model.foot_mass(), feed="estimate",
                                      height=pb["stand"][:, :, 2], bias=s["bias"], noise=s["noise"], enc_noise=s["enc_noise"], attitude={})
    ok = ~(_np(logs["flag"]) == 0xff).any(axis=(1, 2)) & ~(host["flag"] == 0xff).any(axis=(1, 2))
    assert ok.sum() >= (3 * B) // 4
    for k in ("actual", "est"):
        err = np.abs(_np(logs[k])[ok][..., 3:6] - host[k][ok][..., 3:6]).max()
        print(f"B={B} {k}: CoM against the host within {1e3 * err:.4f} mm")
        assert err < 0.005, k
    err = np.abs(_np(logs["gyro_bias"])[ok] - host["gyro_bias"][ok]).max()
    print(f"B={B} gyro_bias against the host within {err:.3e} rad/s; solved {_np(logs['solved']).tolist()[:16]}")
    assert (_np(logs["solved"])[ok] == ROLL_T).all() and (host["solved"][ok] == ROLL_T).all()
