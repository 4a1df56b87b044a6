"""The estimator's per-leg trust gate on the device (include/mpcqp_gate.h, mpcqp_estimate_track_gated and
mpcqp_rollout_observe_gated); the shared cases are in tests/gate_cases.py.  Every test calls the new entry points unconditionally: a
library without them fails here, it does not skip.

The batch is the 16 x 25 legsim batch of tests/test_gpu_rollout_observe.py: ground 0.3 under the even robots with tau_max x 0.5, sensor
draws on the odd robots.  The log pass runs on the sensor logs of its ungated roll-out with feed = "truth".

Log pass (estimate_track(gate=...)):
  1. Open thresholds are estimate_track bit for bit, and trust is the clock, or the given trust.
  2. Replay: ungated estimate_track with trust = the gated call's "trust" gives its outputs and state bit for bit.
  3. Host parity: estimator.estimate_track_host(gate=, io_dtype=), row by row from the device's own state before the row and over the
     whole log, both in the one-row band (1e-9 relative in fp64 I/O, two float32 spacings in fp32 I/O), after the host has shown w < 1,
     0 < w < 1 and w = 1 on stance legs.
  4. The independent 18-state form handed the device's trust.
  5. 13 + 12 rows through `state` are one call.   6. B = 1, 33, 65.   7. Poison.   8. Argument errors and empty calls.
Roll-out (rollout_observe(gate=...)):
  1. feed = "truth" is rollout_slip.   2. Open thresholds are rollout_observe, both feeds.
  3. In the loop equals after the fact, both feeds, at the defaults.   4. 13 + 12 ticks are one call.
  5. Host parity is held the way tests/test_gpu_rollout_observe.py holds the ungated loop: the loop's estimator rows are the log
     pass's bit for bit (3.), the log pass is compared with the host row by row (log pass 3.), and the closed-loop conditions of
     gate_cases.check_flying_trot hold on the device as they do on the host (f64 I/O).
"""
import numpy as np
import pytest

import drive_cases as dc
import estimate_cases as C
import gate_cases as G
import mpcqp
import observe_cases as oc
import test_gpu_rollout_observe as ro
from legsim_cases import DELTA, ROLL_B, ROLL_T
from mpcqp import estimator

pytestmark = pytest.mark.gpu

_t, _np, _same = ro._t, ro._np, ro._same
OUT = estimator.OUT + ("trust",)
EST_PAIRS = (("est", "est"), ("feet_est", "feet"), ("sigma", "sigma"), ("nis", "nis"), ("trust", "trust"))
_CACHE = {}


def _log_ops(io):
    """The sensor logs of the ungated roll-out with feed = "truth" as estimate_track's operands (device tensors), once per I/O dtype."""
    if io not in _CACHE:
        ops, _, logs = ro._run(io, "truth")
        _CACHE[io] = (ops.sol, {"imu": logs["imu"], "q": logs["q_enc"], "qd": logs["qd_enc"], "contact_log": logs["contact_log"],
                                "init": logs["actual"][:, 0].contiguous(), "height": ops.height})
    return _CACHE[io]


def _track(sol, d, rows=slice(None), state=None, idx=None, **kw):
    """estimate_track on the operands `d` (rows `rows`, robots `idx`) -> numpy outputs; `state` (numpy [B,131] or None = zeros) comes
    back advanced as "state"."""
    import torch
    pick = lambda v, rowwise: v if v is None else (v[:, rows] if rowwise else v)
    d = {k: pick(v, k in ("imu", "q", "qd", "contact_log", "trust")) for k, v in d.items()}
    if idx is not None:
        d = {k: (None if v is None else v[idx]) for k, v in d.items()}
    d = {k: (None if v is None else v.contiguous()) for k, v in d.items()}
    B = d["imu"].shape[0]
    st = _t(np.zeros((B, 131)) if state is None else state, torch.float64)
    out = sol.estimate_track(d["imu"], d["q"], d["qd"], d["contact_log"], d["init"], trust=d.get("trust"), height=d["height"], state=st, **kw)
    torch.cuda.synchronize()
    res = {k: (None if v is None else _np(v)) for k, v in out.items()}
    res["state"] = _np(st)
    return res


def _equal(a, b, keys):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _gated(io):
    if ("gated", io) not in _CACHE:
        sol, d = _log_ops(io)
        _CACHE[("gated", io)] = _track(sol, d, gate=G.GATE)
    return _CACHE[("gated", io)]


def _host_ops(d):
    return {k: (None if v is None else _np(v)) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------------------------------ log pass
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_open_gate_is_estimate_track(io):
    sol, d = _log_ops(io)
    plain, opened = _track(sol, d), _track(sol, d, gate=G.OPEN)
    assert set(opened) == set(plain) | {"trust"}
    assert _equal(plain, opened, estimator.OUT + ("state",))
    ok = ~np.isnan(plain["nis"]).any(axis=1)
    assert ok.sum() >= (3 * ROLL_B) // 4
    assert np.array_equal(opened["trust"][ok], (_np(d["contact_log"]) != 0).astype(np.float64)[ok])
    given = _t(np.random.default_rng(3).uniform(0.0, 1.0, (ROLL_B, ROLL_T, 4)), sol.tdtype)
    a, b = _track(sol, dict(d, trust=given)), _track(sol, dict(d, trust=given), gate=G.OPEN)
    assert _equal(a, b, estimator.OUT + ("state",)) and np.array_equal(b["trust"][ok], _np(given)[ok])
    assert not _equal(a, plain, ("est",))


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_replay(io):
    sol, d = _log_ops(io)
    gated = _gated(io)
    ok = ~np.isnan(gated["trust"]).any(axis=(1, 2))
    assert ok.sum() >= (3 * ROLL_B) // 4
    w = gated["trust"]
    stance = (_np(d["contact_log"]) != 0)[ok]
    assert (w[ok][stance] < 1).any() and ((w[ok] > 0) & (w[ok] < 1))[stance].any() and not w[ok][~stance].any()
    rep = _track(sol, dict(d, trust=_t(np.nan_to_num(w), sol.tdtype)))
    for k in estimator.OUT + ("state",):
        assert np.array_equal(rep[k][ok], gated[k][ok]), k
    assert not _equal(_track(sol, d), gated, ("est",))


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_host_parity(io):
    """Measured on an MI355X, error over band: f64 at most 1.8e-6 row by row and 1.7e-6 over the whole log (nis); f32 every output equal
    to the host's value rounded once, the fp64 state 1.1e-7."""
    import torch
    sol, d = _log_ops(io)
    h = _host_ops(d)
    npio = np.float64 if io == "f64" else np.float32
    host = estimator.estimate_track_host(h["imu"], h["q"], h["qd"], h["contact_log"], h["init"], height=h["height"], delta=DELTA, gate=G.GATE,
                                         io_dtype=npio)
    ok = ~np.isnan(host["nis"]).any(axis=1)
    w, stance = host["trust"][ok], (h["contact_log"] != 0)[ok]
    assert (w[stance] < 1).any() and ((w > 0) & (w < 1))[stance].any() and (w[stance] == 1).any()        # not vacuous
    print(f"{io}: host w < 1 on {int((w[stance] < 1).sum())}, 0 < w < 1 on {int(((w > 0) & (w < 1))[stance].sum())}, w = 1 on "
          f"{int((w[stance] == 1).sum())} of {int(stance.sum())} stance leg-rows")
    state = np.zeros((ROLL_B, 131))
    worst = {k: 0.0 for k in OUT + ("state",)}
    for t in range(ROLL_T):
        dev = _track(sol, d, rows=slice(t, t + 1), state=state, gate=G.GATE)
        row = estimator.estimate_track_host(h["imu"][:, t:t + 1], h["q"][:, t:t + 1], h["qd"][:, t:t + 1], h["contact_log"][:, t:t + 1],
                                            h["init"], height=h["height"], state=state, delta=DELTA, gate=G.GATE, io_dtype=npio)
        for k in OUT + ("state",):
            err, band = C.error(dev[k], row[k], "f64" if k == "state" else io)
            worst[k] = max(worst[k], err / band)
        state = dev["state"]
    print(f"{io} row by row from the device's state, error / band: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    whole = _gated(io)
    assert np.array_equal(state, whole["state"], equal_nan=True)                # (the 25 one-row calls are the one call)
    for k in OUT + ("state",):                                                  # ... and the whole log, in the same band without a growth factor
        err, band = C.error(whole[k], host[k], "f64" if k == "state" else io)
        print(f"{io} whole log against the host, {k}: error / band {err / band:.3e}")
        assert err <= band, k
    for k, v in worst.items():
        assert v <= 1.0, k


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_independent_form(io):
    sol, d = _log_ops(io)
    h = _host_ops(d)
    gated = _gated(io)
    joint = estimator.estimate_joint_host(h["imu"], h["q"], h["qd"], h["contact_log"], h["init"], trust=gated["trust"], height=h["height"],
                                          delta=DELTA)
    for k in estimator.OUT:                                                     # the band without a growth factor, as on the host
        err, band = C.error(gated[k], joint[k], io)
        print(f"{io} {k} against the 18-state form: error {err:.3e}, band {band:.3e}")
        assert err <= band, k


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_pieces(io):
    sol, d = _log_ops(io)
    whole = _gated(io)
    a = _track(sol, d, rows=slice(0, 13), gate=G.GATE)
    b = _track(sol, d, rows=slice(13, 25), state=a["state"], gate=G.GATE)
    for k in OUT:
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), whole[k], equal_nan=True), k
    assert np.array_equal(b["state"], whole["state"], equal_nan=True)
    mixed = _track(sol, d, rows=slice(13, 25), state=_track(sol, d, rows=slice(0, 13))["state"], gate=G.GATE)       # the two calls share the state's layout
    assert mixed["trust"].shape == (ROLL_B, 12, 4) and np.isfinite(mixed["state"][~np.isnan(whole["state"]).any(axis=1)]).all()


@pytest.mark.parametrize("B", [1, 33, 65])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_partial_and_crossing_blocks(io, B):
    """64 robots fill a block of 256 lanes: 65 crosses it, 33 and 1 leave it partly empty.  Robot i is robot i mod 16 of the batch."""
    import torch
    sol, d = _log_ops(io)
    whole = _gated(io)
    idx = np.arange(B) % ROLL_B
    out = _track(sol, d, idx=torch.as_tensor(idx).cuda(), gate=G.GATE)
    for k in OUT + ("state",):
        assert np.array_equal(out[k], whole[k][idx], equal_nan=True), k


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_poison(io):
    sol, d = _log_ops(io)
    clean = _gated(io)
    who = int(np.flatnonzero(~np.isnan(clean["state"]).any(axis=1))[5])
    qd = d["qd"].clone()
    qd[who, 3, 1, 0] = float("inf")
    out = _track(sol, dict(d, qd=qd), gate=G.GATE)
    others = np.arange(ROLL_B) != who
    for k in OUT:
        assert np.isnan(out[k][who, 3:]).all() and np.array_equal(out[k][who, :3], clean[k][who, :3]), k
        assert np.array_equal(out[k][others], clean[k][others], equal_nan=True), k
    assert np.isnan(out["state"][who]).all() and np.array_equal(out["state"][others], clean["state"][others], equal_nan=True)


def _gate(**kw):
    g = mpcqp.product_library().default_trust_gate()
    for k, v in kw.items():
        setattr(g, k, v)
    return g


BAD_GATES = [(dict(size=8), "trust gate struct size mismatch"), (dict(d_lo=float("nan")), "trust gate: d_lo and d_hi"),
             (dict(d_hi=float("inf")), "trust gate: d_lo and d_hi"), (dict(d_lo=-0.5), "trust gate: d_lo and d_hi"),
             (dict(d_lo=4.0), "trust gate: d_lo and d_hi"), (dict(d_hi=0.5), "trust gate: d_lo and d_hi")]


def test_arguments_and_empty_calls(oracle_lib):
    import torch
    sol, d = _log_ops("f64")
    eng, B, T = sol.engine, 3, 2
    p = lambda t: t.data_ptr()
    c = {k: (v[:B, :T] if k in ("imu", "q", "qd", "contact_log") else v[:B]).contiguous() for k, v in d.items()}
    outs = [torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((B, T, 12), (B, T, 4, 3), (B, T, 6), (B, T), (B, T, 4))]
    state = torch.zeros((B, 131), dtype=torch.float64, device="cuda")
    good = dict(B=B, T=T, imu=p(c["imu"]), q=p(c["q"]), qd=p(c["qd"]), contact_log=p(c["contact_log"]), trust=0, height=p(c["height"]),
                init=p(c["init"]), state=p(state), est=p(outs[0]), feet_est=p(outs[1]), sigma=p(outs[2]), nis=p(outs[3]), trust_out=p(outs[4]))
    bad = [(dict(gate=_gate(**kw)), text) for kw, text in BAD_GATES]
    bad += [(dict(B=-1), "size out of range"), (dict(imu=0), r"null buffer \(imu, q, qd\)"), (dict(init=0), "null init buffer"),
            (dict(contact_log=0), "null contact_log buffer without trust"),
            (dict(est=0, feet_est=0, sigma=0, nis=0, trust_out=0), r"no output buffer \(est, feet_est, sigma, nis and trust_out are all null\)")]
    for change, text in bad:
        with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_estimate_track_gated: " + text):
            eng.estimate_track_gated_ptr(**dict(good, **change))
    for change in (dict(B=0), dict(T=0)):                                       # no-ops
        eng.estimate_track_gated_ptr(**dict(good, **change))
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((state == 0.0).all())
    eng.estimate_track_gated_ptr(**dict(good, est=0, feet_est=0, sigma=0, nis=0))      # trust_out alone is an output
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs[:4]) and bool(torch.isfinite(outs[4]).all()) and bool((state[:, 130] == 1.0).all())
    alone = outs[4].clone()
    state.zero_()
    eng.estimate_track_gated_ptr(**good)
    torch.cuda.synchronize()
    assert torch.equal(outs[4], alone) and all(bool(torch.isfinite(o).all()) and not bool((o == 7.0).all()) for o in outs)
    # the Python layer checks a dict before the call; the roll-out's entry point checks the structure like the log pass's
    with pytest.raises(ValueError, match="trust gate: d_lo and d_hi must be finite with 0 <= d_lo < d_hi"):
        _track(sol, d, gate={"d_lo": 2.0, "d_hi": 1.0})
    ops = ro._ops("f64")
    for kw, text in BAD_GATES:
        with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_observe_gated: " + text):
            ops.observe(ops.state(), 1, "truth", gate=_gate(**kw))
    with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_observe_gated: feed is neither"):
        ops.observe(ops.state(), 1, 2, gate={})
    zst, fresh = ops.state(), ops.state()
    zero = ops.observe(zst, 0, "estimate", gate={})
    torch.cuda.synchronize()
    assert zero["trust"].shape == (ROLL_B, 0, 4) and all(torch.equal(zst[k], fresh[k]) for k in ro.SLIP_STATE + ("est",))
    # the checker library does not have the calls, and says which header is missing
    oeng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    with pytest.raises(mpcqp.MpcQpError, match=r"does not export include/mpcqp_gate.h \(product library only\)"):
        oeng.estimate_track_gated_ptr(**good)
    plib = mpcqp.product_library()
    assert plib.has_gate and all(plib.calls[s][0] is not None for s in mpcqp._capi.GATE_SYMBOLS) and not oracle_lib.has_gate


# ------------------------------------------------------------------------------------------------------------------------ roll-out
def _loop(io, feed, gate):
    """The gated roll-out on the ice, once per (I/O dtype, feed, thresholds): (ops, final state, logs)."""
    import torch
    key = ("loop", io, feed, tuple(sorted(gate.items())))
    if key not in _CACHE:
        ops = ro._ops(io)
        st = ops.state()
        logs = ops.observe(st, ROLL_T, feed, inertia=dc.weak_row(0.5), height=ops.height, gate=gate)
        torch.cuda.synchronize()
        _CACHE[key] = (ops, st, logs)
    return _CACHE[key]


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_truth_feed_is_rollout_slip(io):
    import torch
    ops, st, logs = _loop(io, "truth", G.GATE)
    ref_st = ops.state()
    ref = ops.slip(ref_st, ROLL_T, inertia=dc.weak_row(0.5))
    torch.cuda.synchronize()
    assert set(logs) == set(ref) | set(oc.EST_LOGS) | {"trust"}
    for k in ro.SLIP_STATE:
        assert torch.equal(st[k], ref_st[k]), k
    for k in ro.SLIP_LOGS:
        assert _same(logs[k], ref[k]), k
    assert int(((ref["flag"] & 128) != 0)[ref["contact_log"] != 0].sum()) > 0


@pytest.mark.parametrize("feed", ["truth", "estimate"])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_open_gate_is_rollout_observe(io, feed):
    import torch
    ops, st, logs = _loop(io, feed, G.OPEN)
    _, ref_st, ref = ro._run(io, feed)
    assert set(logs) == set(ref) | {"trust"}
    for k in ro.SLIP_STATE + ("est",):
        assert _same(st[k], ref_st[k]), k
    for k in ro.SLIP_LOGS + oc.EST_LOGS:
        assert _same(logs[k], ref[k]), k
    ok = torch.isfinite(logs["nis"]).all(dim=1)
    assert int(ok.sum()) >= (3 * ROLL_B) // 4
    assert torch.equal(logs["trust"][ok], (logs["contact_log"][ok] != 0).to(ops.sol.tdtype))


@pytest.mark.parametrize("feed", ["truth", "estimate"])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_in_the_loop_equals_after_the_fact(io, feed):
    import torch
    ops, st, logs = _loop(io, feed, G.GATE)
    sol, B = ops.sol, ops.B
    ok = ~(_np(logs["flag"]) == 0xff).any(axis=(1, 2))                              # robots without a poisoned leg-row
    assert ok.sum() >= (3 * B) // 4
    okt = torch.as_tensor(ok).cuda()
    state = torch.zeros((B, 131), dtype=torch.float64, device="cuda")
    rep = sol.estimate_track(logs["imu"], logs["q_enc"], logs["qd_enc"], logs["contact_log"], logs["actual"][:, 0].contiguous(),
                             height=ops.height, state=state, gate=G.GATE)
    torch.cuda.synchronize()
    for k, src in EST_PAIRS:
        assert torch.equal(logs[k][okt], rep[src][okt]) and bool(torch.isfinite(logs[k][okt]).all()), k
    assert torch.equal(st["est"][okt], state[okt])
    w, stance = _np(logs["trust"])[ok], (_np(logs["contact_log"]) != 0)[ok]
    slid = ((_np(logs["flag"]) & 128) != 0)[ok] & stance
    print(f"{io} {feed}: w < 1 on {int((w[stance] < 1).sum())} of {int(stance.sum())} stance leg-rows, {int(slid.sum())} marked sliding; "
          f"solved {logs['solved'].tolist()}")
    assert (w[stance] < 1).any() and (w[stance] == 1).any() and not w[~stance].any()
    _, _, plain = ro._run(io, feed)
    assert not _same(plain["est"], logs["est"])                                     # the gate is in the loop


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_rollout_pieces(io):
    import torch
    ops, whole_st, whole = _loop(io, "estimate", G.GATE)
    run = lambda st, n, first=0, **kw: ops.observe(st, n, "estimate", first=first, inertia=dc.weak_row(0.5), height=ops.height, gate=G.GATE, **kw)
    st = ops.state()
    p1 = run(st, 13)
    p2 = run(st, ROLL_T - 13, first=13)
    quiet_st = ops.state()
    quiet = run(quiet_st, ROLL_T, log=False)
    torch.cuda.synchronize()
    for k in ro.SLIP_STATE + ("est",):
        assert _same(st[k], whole_st[k]) and _same(quiet_st[k], whole_st[k]), k
    for k in ro.SLIP_LOGS + oc.EST_LOGS + ("trust",):
        if k == "solved":
            assert torch.equal(p1[k] + p2[k], whole[k]) and torch.equal(quiet[k], whole[k])
        else:
            assert _same(torch.cat([p1[k], p2[k]], dim=1), whole[k]) and quiet[k] is None, k


def test_what_the_gate_does_flying_trot():
    """Measured on an MI355X (f64 I/O): ungated lowest CoM 199.2 mm, tilt 0.905 rad; gated 283.0 mm, 0.076 rad; 36 of 36 ticks solved in
    both.  The conditions are gate_cases.check_flying_trot's."""
    import torch
    pb = G.gait_batch()
    ops = ro._Ops("f64", G.GAIT_B, G.GAIT_T, pb=pb, rows=None)
    ice = _t(np.full(G.GAIT_B, G.ICE), ops.sol.tdtype)
    runs = []
    for gate in (None, G.GATE):
        st = ops.state()
        out = ops.observe(st, G.GAIT_T, "estimate", sens=False, ground=ice, land="rule", gate=gate)
        torch.cuda.synchronize()
        runs.append({k: _np(v) for k, v in out.items() if v is not None})
    G.check_flying_trot("device f64", *runs)
