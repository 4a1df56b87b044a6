"""The slip roll-out with sensors and the state estimator inside its tick loop, on the device (include/mpcqp_observe.h,
mpcqp_rollout_observe); the shared cases are in tests/observe_cases.py.

The case is the 16 x 25 batch of tests/legsim_cases.py (period 12, two robots pushed) on ground 0.3 under the even robots with
tau_max x 0.5, so feet slide and legs clamp; bias, IMU noise and encoder noise are drawn once (observe_cases.sensor_draw) and are
non-zero for the odd robots.

  1. feed="truth" is rollout_slip: state and every log, bit for bit; once more with a model table and an actuator table whose rows differ.
  2. In the loop equals after the fact, for both feeds: estimate_track / imu_log / joint_rates on the roll-out's own logs.
  3. The MPC read what it was told: one-tick calls against solve_batch_phase on the estimate (or on the truth).
  4. Pieces, determinism, NULL logs, B in {1, 33, 65}.
  5. Poison, argument errors, empty calls, the checker library.
  6. What the feedback does to the regulated height (f64 I/O).

The encoders are compared with the q / qd logs bit for bit on the robots without encoder noise (a noisy encoder is the log plus its
noise, which is held in fp64 I/O, where the sum is not rounded again).  The one-row band is the project's: 1e-9 relative in fp64 I/O,
two float32 spacings in fp32 I/O."""
import numpy as np
import pytest

import drive_cases as dc
import mpcqp
import observe_cases as oc
import test_gpu_stance_drive as drv
from legsim_cases import DELTA, ROLL_B, ROLL_T, STEP_HEIGHT
from mpcqp import actuators, estimator, gaits, lite3_model

_t, _np = drv._t, drv._np
SLIP_STATE = ("x", "ref", "feet", "legs", "tick", "slip")
SLIP_LOGS = drv.ALL_LOGS + ("cmd", "slip_log", "disp")
_CACHE = {}


def _same(a, b):
    return np.array_equal(_np(a), _np(b), equal_nan=True)


def _band_error(dev, ref, io):
    """(error, band) of the one-row band: fp64 |dev - ref| / max(1, |ref|) against 1e-9, fp32 float32 spacings of ref against 2."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(dev), np.isnan(ref))
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0, 1.0
    if io == "f64":
        return float((np.abs(dev - ref)[ok] / np.maximum(1.0, np.abs(ref[ok]))).max()), dc.F64_BAND
    sp = np.spacing(np.maximum(np.abs(ref[ok]).astype(np.float32), np.float32(2.0 ** -20))).astype(np.float64)
    return float((np.abs(dev - ref)[ok] / sp).max()), dc.F32_SPACINGS


class _Ops:
    """The device operands of one batch (tests/test_gpu_slip.py's pattern): the constant rows once, a fresh copy of the state per run.
    B robots are the legsim batch's, repeated in order where B > 16."""

    def __init__(self, io, B=ROLL_B, T=ROLL_T, pb=None, rows=None):
        import torch
        if pb is None:
            pb, rows = drv._case(io, ROLL_B)
            idx = np.arange(B) % ROLL_B
            per_robot = lambda v: isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == ROLL_B
            pb = {k: (v[idx] if per_robot(v) else v) for k, v in pb.items()}
            rows = {k: (v[idx] if per_robot(v) else v) for k, v in rows.items()}
        self.io, self.B, self.T, self.pb, self.rows = io, B, T, pb, rows
        self.sol = mpcqp.MPCBatch(N=10, delta=DELTA, io_dtype=io, precision="mixed")
        dt = self.sol.tdtype
        self.const = {"gait": _t(pb["gait"], torch.int32), "stand": _t(pb["stand"], dt), "gain": _t(pb["gain"], dt), "mu": _t(pb["mu"], dt),
                      "step_height": _t(np.full(B, STEP_HEIGHT), dt)}
        self.kw = {} if rows is None else {"body": _t(rows["body"], dt), "push": _t(rows["push"], dt),
                                           "push_ticks": _t(rows["push_ticks"], torch.int32)}
        self.ground = _t(oc.ground_rows(B), dt)
        self.me = _t(np.full(B, lite3_model.foot_mass()), dt)
        self.height = _t(pb["stand"][:, :, 2], dt)
        s = oc.sensor_draw(B, T)
        self.noisy = s["noisy"]
        self.sens = {k: _t(s[k], dt) for k in ("bias", "noise", "enc_noise")}

    def state(self):
        import torch
        dt, z = self.sol.tdtype, lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
        return {"x": _t(self.pb["x"], dt), "ref": _t(self.pb["ref"], dt), "feet": _t(self.pb["feet"], dt), "legs": z(self.B, 4, 7),
                "tick": _t(self.pb["tick"], torch.int32), "slip": z(self.B, 4, 2), "est": z(self.B, 131)}

    def _args(self, st, T):
        c = self.const
        return (st["x"], st["ref"], st["feet"], st["legs"], c["gait"], c["stand"], c["gain"], st["tick"], c["mu"], T, c["step_height"])

    def slip(self, st, T, **kw):
        return self.sol.rollout_slip(*self._args(st, T), self.ground, self.me, st["slip"], **self.kw, **kw)

    def observe(self, st, T, feed, sens=True, first=0, **kw):
        """`first`: the row of the call's first tick in the sensor draws (a roll-out in pieces)."""
        if sens:
            for k, v in self.sens.items():
                kw.setdefault(k, v if k == "bias" else v[:, first:first + T].contiguous())
        kw.setdefault("ground", self.ground)
        return self.sol.rollout_observe(*self._args(st, T), kw.pop("ground"), self.me, st["slip"], st["est"], feed, **self.kw, **kw)


def _ops(io, B=ROLL_B):
    if (io, B) not in _CACHE:
        _CACHE[(io, B)] = _Ops(io, B)
    return _CACHE[(io, B)]


def _run(io, feed, with_height=True, B=ROLL_B):
    """The roll-out of tests 1, 2 and 4 on the ice, once per (I/O dtype, feed, height given or not, B): (ops, final state, logs)."""
    import torch
    key = ("run", io, feed, with_height, B)
    if key not in _CACHE:
        ops = _ops(io, B)
        st = ops.state()
        logs = ops.observe(st, ROLL_T, feed, inertia=dc.weak_row(0.5), height=ops.height if with_height else None)
        torch.cuda.synchronize()
        _CACHE[key] = (ops, st, logs)
    return _CACHE[key]


# ----------------------------------------------------------------------------------------------------------- 1. shadow mode is rollout_slip
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_truth_feed_is_rollout_slip(io):
    import torch
    ops, st, logs = _run(io, "truth")
    ref_st = ops.state()
    ref = ops.slip(ref_st, ROLL_T, inertia=dc.weak_row(0.5))
    torch.cuda.synchronize()
    assert set(logs) == set(ref) | set(oc.EST_LOGS)
    for k in SLIP_STATE:
        assert torch.equal(st[k], ref_st[k]), k
    for k in SLIP_LOGS:
        assert _same(logs[k], ref[k]), k
    assert int(((ref["flag"] & 128) != 0)[ref["contact_log"] != 0].sum()) > 0 and int(((ref["flag"] & 2) != 0).sum()) > 0
    assert bool(torch.isfinite(logs["est"]).all()) and bool((st["est"][:, 130] == 1.0).all())
    # ... and under a model table and an actuator table whose rows differ per robot
    B, sol = ops.B, ops.sol
    scale = np.linspace(0.8, 1.25, B)
    models = np.stack([8.885 * scale, 0.24 * scale, 1.0 * scale, 1.0 * scale, np.full(B, sol.cfg.f_min), sol.cfg.f_max * np.linspace(0.7, 1.0, B)],
                      axis=1)
    tmax = lite3_model.leg_inertia()["tau_max"]
    act = np.concatenate([tmax[None] * np.linspace(0.35, 1.0, B)[:, None], np.tile([6.0, 6.0, 4.0], (B, 1)) * scale[:, None] + 2.0,
                          np.tile([14.0, 14.0, 10.0], (B, 1)) + 4.0 * scale[:, None]], axis=1)
    assert actuators.valid_rows(act).all() and len({tuple(r) for r in act}) == B and len({tuple(r) for r in models}) == B
    try:
        sol.set_models(models)
        sol.set_actuators(act)
        a, b = ops.state(), ops.state()
        want = ops.slip(a, ROLL_T)
        got = ops.observe(b, ROLL_T, "truth", height=ops.height)
        torch.cuda.synchronize()
    finally:
        sol.clear_actuators()
        sol.clear_models()
    for k in SLIP_STATE:
        assert torch.equal(a[k], b[k]), k
    for k in SLIP_LOGS:
        assert _same(want[k], got[k]), k
    assert not torch.equal(want["forces"], ref["forces"])


# ------------------------------------------------------------------------------------------------- 2. in the loop equals after the fact
def _replay(ops, st, logs, with_height, io):
    """Test 2 on one roll-out; returns the counts of the rows it needed."""
    import torch
    sol, B, T = ops.sol, ops.B, logs["actual"].shape[1]
    flag, stance = _np(logs["flag"]), _np(logs["contact_log"]) != 0
    ok = ~(flag == 0xff).any(axis=(1, 2))                                           # robots without a poisoned leg-row
    assert ok.sum() >= (3 * B) // 4
    okt = torch.as_tensor(ok).cuda()
    state = torch.zeros((B, 131), dtype=torch.float64, device="cuda")
    rep = sol.estimate_track(logs["imu"], logs["q_enc"], logs["qd_enc"], logs["contact_log"], logs["actual"][:, 0].contiguous(),
                             height=ops.height if with_height else None, state=state)
    torch.cuda.synchronize()
    for k, src in (("est", "est"), ("feet_est", "feet"), ("sigma", "sigma"), ("nis", "nis")):
        assert torch.equal(logs[k][okt], rep[src][okt]), k
        assert bool(torch.isfinite(logs[k][okt]).all()), k
    assert torch.equal(st["est"][okt], state[okt])
    # the encoders against the joint logs
    slog = _np(logs["slip_log"])
    still, live = ~slog.any(axis=-1), flag != 0xff
    quiet = ~ops.noisy[:, None, None] & still & live
    q, qd, qe, qde = (_np(logs[k]) for k in ("q", "qd", "q_enc", "qd_enc"))
    assert np.array_equal(qe[quiet], q[quiet]) and np.array_equal(qde[quiet], qd[quiet])
    if io == "f64":                                                                 # a noisy encoder is the log plus its noise
        en = _np(ops.sens["enc_noise"])[:, :T]
        m = still & live
        assert np.array_equal(qe[m], (q + en[..., 0:3])[m]) and np.array_equal(qde[m], (qd + en[..., 3:6])[m])
    sliding = ~still & stance & live & ~ops.noisy[:, None, None]
    fv = torch.cat([logs["slip_log"].to(sol.tdtype), torch.zeros((B, T, 4, 1), dtype=sol.tdtype, device="cuda")], dim=-1).contiguous()
    jr = sol.joint_rates(logs["actual"], logs["forces"], logs["feet_log"], foot_vel=fv)
    torch.cuda.synchronize()
    for k, dev in (("q", qe), ("qd", qde)):
        err, band = _band_error(dev[sliding], _np(jr[k])[sliding], io)
        print(f"{io} B={B} sliding stance rows, {k}_enc against joint_rates: error {err:.3e}, band {band:.1e} on {int(sliding.sum())} leg-rows")
        assert err <= band, k
    # the IMU rows
    wr = gaits.log_wrench(ops.rows["push"], ops.rows["push_ticks"], ops.pb["tick"], T)
    pushed = wr.any(axis=-1)
    kw = {"bias": ops.sens["bias"], "noise": ops.sens["noise"][:, :T].contiguous()}
    imu = sol.imu_log(logs, body=ops.kw["body"], **kw)
    torch.cuda.synchronize()
    pt = torch.as_tensor(pushed).cuda()
    assert torch.equal(logs["imu"][~pt], imu[~pt]) and not torch.equal(logs["imu"][pt], imu[pt])
    h = {k: _np(logs[k]) for k in ("actual", "forces", "feet_log")}
    acc = lite3_model.plant_base_acc_host(h["actual"], h["forces"], h["feet_log"], _np(ops.kw["body"]), wrench=wr)
    host = estimator.imu_log_host(h["actual"], h["forces"], h["feet_log"], base_acc=acc, bias=_np(kw["bias"]), noise=_np(kw["noise"]))
    err, band = _band_error(_np(logs["imu"])[pushed], host[pushed], io)
    print(f"{io} B={B} pushed rows, imu against imu_log_host: error {err:.3e}, band {band:.1e} on {int(pushed.sum())} rows")
    assert err <= band
    flight = ~stance.any(axis=-1) & ~ops.noisy[:, None]                            # flight rows of the robots without bias and noise
    assert not _np(logs["imu"])[flight][:, 3:6].any()                              # a flight tick reads an exact zero
    return {"sliding": int(sliding.sum()), "flight": int(flight.sum()), "pushed": int(pushed.sum()), "noisy": int((ops.noisy & ok).sum())}


@pytest.mark.gpu
@pytest.mark.parametrize("with_height", [True, False])
@pytest.mark.parametrize("feed", ["truth", "estimate"])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_in_the_loop_equals_after_the_fact(io, feed, with_height):
    ops, st, logs = _run(io, feed, with_height)
    n = _replay(ops, st, logs, with_height, io)
    print(f"{io} {feed}: {n}; solved {logs['solved'].tolist()}")
    assert n["sliding"] > 0 and n["flight"] > 0 and n["pushed"] > 0 and n["noisy"] > 0     # not vacuous


# --------------------------------------------------------------------------------------------------- 3. the MPC read what it was told
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_the_mpc_read_what_it_was_told(io):
    import torch
    ops = _ops(io)
    sol, c, B = ops.sol, ops.const, ops.B
    assert not sol.warm_start
    init = _t(ops.pb["x"][:, :12] + 0.04 * (np.arange(12) == 5), sol.tdtype)
    first = {}
    for feed in ("estimate", "truth"):
        st = ops.state()
        for t in range(ROLL_T):
            x0, ref0, tick0, feet0 = st["x"].clone(), st["ref"].clone(), st["tick"].clone(), st["feet"].clone()
            row = ops.observe(st, 1, feed, first=t, inertia=dc.weak_row(0.5), est_init=init)
            if feed == "estimate":
                xr, fr = torch.cat([row["est"][:, 0], x0[:, 12:]], dim=1).contiguous(), row["feet_est"][:, 0].contiguous()
            else:
                xr, fr = x0, feet0
            want = sol.solve_batch_phase(xr, ref0, fr, c["gait"], tick0, c["stand"], c["gain"], c["mu"])["u"][:, 0].clone()
            torch.cuda.synchronize()
            assert _same(row["cmd"][:, 0], want), (feed, t)
            if t == 0:
                first[feed] = row["cmd"][:, 0].clone()
        assert int(st["tick"].min()) == ROLL_T
    differ = (first["estimate"] != first["truth"]).any(dim=1)
    assert bool(differ.all()), differ.tolist()


# --------------------------------------------------------------------------------------------------------------------- 4. composition
@pytest.mark.gpu
@pytest.mark.parametrize("feed", ["truth", "estimate"])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_pieces_determinism_and_null_logs(io, feed):
    import torch
    ops, whole_st, whole = _run(io, feed)
    run = lambda st, n, first=0, **kw: ops.observe(st, n, feed, first=first, inertia=dc.weak_row(0.5), height=ops.height, **kw)
    flight = np.nonzero((~(_np(whole["contact_log"]) != 0).any(axis=-1)).any(axis=0))[0]
    cuts = [13] + [int(t) for t in flight if 0 < t < ROLL_T and t != 13][:1]
    assert len(cuts) == 2 or 13 in flight, flight                                   # one cut where a robot is in flight
    for cut in cuts:
        st = ops.state()
        p1 = run(st, cut)
        p2 = run(st, ROLL_T - cut, first=cut)
        torch.cuda.synchronize()
        for k in SLIP_STATE + ("est",):
            assert _same(st[k], whole_st[k]), (cut, k)
        for k in SLIP_LOGS + oc.EST_LOGS:
            if k == "solved":
                assert torch.equal(p1[k] + p2[k], whole[k])
            else:
                assert _same(torch.cat([p1[k], p2[k]], dim=1), whole[k]), (cut, k)
    again_st, quiet_st = ops.state(), ops.state()
    again = run(again_st, ROLL_T)
    quiet = run(quiet_st, ROLL_T, log=False)
    torch.cuda.synchronize()
    for k in SLIP_STATE + ("est",):
        assert _same(again_st[k], whole_st[k]) and _same(quiet_st[k], whole_st[k]), k
    for k in SLIP_LOGS + oc.EST_LOGS:
        assert _same(again[k], whole[k]), k
        assert k == "solved" or quiet[k] is None, k
    assert torch.equal(quiet["solved"], whole["solved"])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 33, 65])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_partial_and_crossing_blocks(io, B):
    """64 robots fill a block of 256 lanes: 65 crosses it, 33 and 1 leave it partly empty."""
    import torch
    ops, st, logs = _run(io, "estimate", True, B)
    n = _replay(ops, st, logs, True, io) if B > 1 else None
    if B == 1:                                                                       # (one robot: the first, neither pushed nor noisy)
        state = torch.zeros((1, 131), dtype=torch.float64, device="cuda")
        rep = ops.sol.estimate_track(logs["imu"], logs["q_enc"], logs["qd_enc"], logs["contact_log"], logs["actual"][:, 0].contiguous(),
                                     height=ops.height, state=state)
        torch.cuda.synchronize()
        assert all(torch.equal(logs[k], rep[s]) for k, s in (("est", "est"), ("feet_est", "feet"), ("sigma", "sigma"), ("nis", "nis")))
        assert torch.equal(st["est"], state) and bool(torch.isfinite(state).all())
    else:
        assert n["sliding"] > 0 and n["noisy"] > 0


# ------------------------------------------------------------------------------------------------------------ 5. poison and arguments
@pytest.mark.gpu
@pytest.mark.parametrize("feed", ["truth", "estimate"])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_poison(io, feed):
    import torch
    ops, clean_st, clean = _run(io, feed)
    noise = ops.sens["noise"].clone()
    noise[5, 3] = float("nan")
    st = ops.state()
    out = ops.observe(st, ROLL_T, feed, inertia=dc.weak_row(0.5), height=ops.height, noise=noise)
    torch.cuda.synchronize()
    for k in oc.EST_LOGS:
        if k in ("est", "feet_est", "sigma", "nis"):
            assert bool(torch.isnan(out[k][5, 3:]).all()), k
        assert _same(out[k][5, :3], clean[k][5, :3]), k
    assert bool(torch.isnan(out["imu"][5, 3]).all()) and bool(torch.isnan(st["est"][5]).all())
    if feed == "estimate":
        assert int(out["solved"][5]) == 3
    else:
        for k in SLIP_STATE:
            assert torch.equal(st[k][5], clean_st[k][5]), k
        for k in SLIP_LOGS:
            assert _same(out[k][5], clean[k][5]), k
    keep = torch.arange(ops.B, device="cuda") != 5
    for k in SLIP_STATE + ("est",):
        assert _same(st[k][keep], clean_st[k][keep]), k
    for k in SLIP_LOGS + oc.EST_LOGS:
        assert _same(out[k][keep], clean[k][keep]), k


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_arguments_and_empty_calls(oracle_lib, io):
    import torch
    ops = _ops(io)
    B, sol, c = ops.B, ops.sol, ops.const
    with pytest.raises(ValueError, match="feed must be 'truth' or 'estimate', got 'both'"):
        ops.observe(ops.state(), 1, "both")
    with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_observe: feed is neither MPCQP_FEED_TRUTH nor MPCQP_FEED_ESTIMATE"):
        ops.observe(ops.state(), 1, 2)
    st = ops.state()
    st["est"] = None
    with pytest.raises(ValueError, match="operand mismatch: est_state expected"):
        ops.observe(st, 1, "truth")
    with pytest.raises(ValueError, match="estimator: kappa must be finite and non-negative"):
        ops.observe(ops.state(), 1, "truth", estimator={"kappa": -1.0})
    par = sol.engine.library.default_estimator()
    par.kappa = -1.0
    with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_observe: estimator: kappa, q_\\*, r_\\*, k_swing and p0_\\* must be"):
        ops.observe(ops.state(), 1, "truth", estimator=par)
    par = sol.engine.library.default_estimator()
    par.size = 8
    with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_observe: estimator struct size mismatch"):
        ops.observe(ops.state(), 1, "truth", estimator=par)
    with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_observe: drive is neither MPCQP_DRIVE_IDEAL nor MPCQP_DRIVE_LIMITED"):
        ops.observe(ops.state(), 1, "truth", drive=2)
    # at the C-ABI est_state is required, as ground, foot_mass and slip are
    st = ops.state()
    p = lambda t: t.data_ptr()
    head = [B, 1, p(st["x"]), p(st["ref"]), p(st["feet"]), p(st["legs"]), p(c["gait"]), p(c["stand"]), p(c["gain"]), p(st["tick"]), p(c["mu"]),
            0, 0, 0, 10, p(c["step_height"]), 0, 0, 0, 1]
    trio = [p(ops.ground), p(ops.me), p(st["slip"])]
    with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_observe: null buffer"):
        sol.engine.rollout_observe_ptr(*head, *trio, *([0] * 24), 1, 0)
    with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_observe: null buffer"):
        sol.engine.rollout_observe_ptr(*head, p(ops.ground), p(ops.me), 0, *([0] * 24), 1, p(st["est"]))
    # T = 0 and B = 0 are no-ops
    zst, fresh = ops.state(), ops.state()
    zero = ops.observe(zst, 0, "estimate")
    torch.cuda.synchronize()
    for k in SLIP_STATE + ("est",):
        assert torch.equal(zst[k], fresh[k]), k
    assert zero["est"].shape == (B, 0, 12) and zero["nis"].shape == (B, 0) and not bool(zero["solved"].any())
    sol.engine.rollout_observe_ptr(0, 4, *([0] * 9), 0, 0, 0, 10, 0, 0, 0, 0, 1, 0, 0, 0, *([0] * 24), 1, 0)
    # the checker library does not have the call, and says which header is missing
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    with pytest.raises(mpcqp.MpcQpError, match=r"does not export include/mpcqp_observe.h \(product library only\)"):
        eng.rollout_observe_ptr(*([1, 1] + [1] * 9 + [0, 0, 0] + [10, 1, 0, 0, 0, 1, 1, 1, 1] + [0] * 24 + [1, 1]))
    plib = mpcqp.product_library()
    assert plib.has_observe and all(plib.calls[s][0] is not None for s in mpcqp._capi.OBSERVE_SYMBOLS) and not oracle_lib.has_observe


# ------------------------------------------------------------------------------------------------------- 6. what the feedback does
@pytest.mark.gpu
def test_what_the_feedback_does():
    """Measured on an MI355X (f64 I/O, last 10 of 60 rows): without height rows |z^ - z_ref| <= 4.50 mm, mean(z^ - z) 40.00 .. 42.12 mm,
    |z - z_ref| 37.99 .. 45.52 mm; with height rows |z - z_ref| <= 3.58 mm -- the host's figures to the printed digits."""
    import torch
    pb = oc.feedback_batch()
    ops = _Ops("f64", oc.FEED_B, oc.FEED_T, pb=pb, rows=None)
    dt = ops.sol.tdtype
    init, height, grip = _t(pb["est_init"], dt), _t(pb["height"], dt), _t(pb["ground"], dt)
    runs = []
    for h in (None, height):
        st = ops.state()
        out = ops.observe(st, oc.FEED_T, "estimate", sens=False, ground=grip, est_init=init, height=h, land="rule")
        torch.cuda.synchronize()
        runs.append(out)
    blind, seen = runs
    oc.check_feedback("device f64", (_np(blind["actual"]), _np(blind["est"])), (_np(seen["actual"]), _np(seen["est"])),
                      _np(blind["solved"]), _np(seen["solved"]))
