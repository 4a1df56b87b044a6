"""The roll-out with the swing legs inside it on the device (include/mpcqp_sim.h, mpcqp_rollout_legs) on legsim_cases.rollout_batch():
16 robots on the eight named gaits, period 12, 25 ticks, two of them pushed, per-robot bodies; N = 10, mixed precision.

  1. land = rule changes nothing: x, ref, feet, tick and the six logs of rollout_phase, bit for bit.
  2. In the loop equals after the fact: the leg logs against phase_swing / swing_track (host and device) on the roll-out's own logs.
  3. land = actual, replayed row by row on the host from the device's logs; the landing identities.
  4. Two pieces chained through x, ref, feet, legs, tick are one call, bit for bit.
  5. NULL logs, argument checks, no-ops, a block that is not full, poisoned gains, the extension gate.

Bands are those of tests/test_gpu_swing_track.py -- identical fp64 arithmetic on identical inputs: 1e-9 against max(1, |host|) for fp64
I/O, 2 float32 spacings against the host value rounded once for fp32 I/O -- times the growth factor recorded for this batch in
tests/golden/swing_track_growth.npz (47.0) where a state is carried over the 25 rows, and times the one-row growth recorded in
tests/golden/rollout_legs_growth.npz (69.3, measured on the CPU checker's loop by tests/legroll_cases.py) where one row is replayed.
`legs` is fp64 in both I/O types and is held to the fp64 band."""
import re

import numpy as np
import pytest

import mpcqp
from legroll_cases import LEG_LOGS, PHASE_LOGS, ROW_GROWTH_NPZ, STATE, replay_rows
from legsim_cases import DELTA, GROWTH_NPZ, ROLL_B, ROLL_T, STEP_HEIGHT, flag_margins, rollout_batch
from mpcqp import gaits, lite3_model

TRACK_OUT = lite3_model.SWING_OUT                                               # q, qd, tau, foot, err, flag
_CACHE = {}


def _t(a, dt):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _ulps32(dev, host64):
    ref = np.asarray(host64, np.float64).astype(np.float32)
    dev = np.asarray(dev)
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(dev))
    sp = np.spacing(np.maximum(np.abs(ref[~nan]), np.float32(2.0 ** -20)))
    err = np.abs(dev[~nan].astype(np.float64) - ref[~nan].astype(np.float64)) / sp
    return float(err.max()) if err.size else 0.0


def _error(dev, host, io):
    """(error, band): f64 |dev - host| / max(1, |host|) against 1e-9, f32 float32 spacings against 2; the NaN pattern must match."""
    if io == "f32":
        return _ulps32(dev, host), 2.0
    dev, host = np.asarray(dev, np.float64), np.asarray(host, np.float64)
    nan = np.isnan(host)
    assert np.array_equal(nan, np.isnan(dev))
    err = np.abs(dev[~nan] - host[~nan]) / np.maximum(1.0, np.abs(host[~nan]))
    return (float(err.max()) if err.size else 0.0), 1e-9


def _case(io, B=ROLL_B):
    """(pb, rows) of the batch as the I/O type holds it."""
    if B == ROLL_B:
        pb, rows = rollout_batch()
    else:                                                                       # any other size: the same gaits, unpushed, per-robot bodies
        pb = gaits.make_phase_batch(B, tuple(gaits.GAITS), 12, seed=8)
        rows = {"body": mpcqp.synth.make_plant_rows(B, seed=8)["body"], "push": np.zeros((B, 6)), "push_ticks": np.zeros((B, 2), np.int32)}
    if io == "f32":
        pb = {k: (_r32(v) if k in ("x", "ref", "feet", "stand", "gain", "mu") else v) for k, v in pb.items()}
        rows = dict(rows, body=_r32(rows["body"]), push=_r32(rows["push"]))
    return pb, rows


class _Ops:
    """The device operands of one batch: the constant rows once, a fresh copy of the state per run."""

    def __init__(self, sol, pb, rows):
        import torch
        self.sol, self.pb, self.rows, dt = sol, pb, rows, sol.tdtype
        self.B = len(pb["x"])
        self.const = {"gait": _t(pb["gait"], torch.int32), "stand": _t(pb["stand"], dt), "gain": _t(pb["gain"], dt), "mu": _t(pb["mu"], dt),
                      "body": _t(rows["body"], dt), "push": _t(rows["push"], dt), "push_ticks": _t(rows["push_ticks"], torch.int32),
                      "step_height": _t(np.full(self.B, STEP_HEIGHT), dt)}

    def state(self):
        import torch
        dt = self.sol.tdtype
        return {"x": _t(self.pb["x"], dt), "ref": _t(self.pb["ref"], dt), "feet": _t(self.pb["feet"], dt),
                "legs": torch.zeros((self.B, 4, 7), dtype=torch.float64, device="cuda"), "tick": _t(self.pb["tick"], torch.int32)}

    def legs(self, st, T, land, **kw):
        c = self.const
        return self.sol.rollout_legs(st["x"], st["ref"], st["feet"], st["legs"], c["gait"], c["stand"], c["gain"], st["tick"], c["mu"], T,
                                     c["step_height"], land, body=c["body"], push=c["push"], push_ticks=c["push_ticks"], **kw)

    def phase(self, st, T):
        c = self.const
        return self.sol.rollout_phase(st["x"], st["ref"], st["feet"], c["gait"], c["stand"], c["gain"], st["tick"], c["mu"], T, body=c["body"],
                                      push=c["push"], push_ticks=c["push_ticks"])


def _run(io, land):
    """The whole roll-out of the batch, once per (I/O type, land): (ops, final state, logs), tensors on the device."""
    import torch
    if (io, land) not in _CACHE:
        pb, rows = _case(io)
        sol = mpcqp.MPCBatch(N=10, delta=DELTA, io_dtype=io, precision="mixed")
        ops = _Ops(sol, pb, rows)
        st = ops.state()
        logs = ops.legs(st, ROLL_T, land)
        torch.cuda.synchronize()
        _CACHE[(io, land)] = (ops, st, logs)
    return _CACHE[(io, land)]


def _host_logs(logs):
    return {k: (v.cpu().numpy() if v.dtype.is_floating_point is False else v.cpu().numpy().astype(np.float64)) for k, v in logs.items()}


def _touchdowns(pb, T):
    """bool [B,T,4]: leg l touches down at the tick after row t."""
    return np.stack([gaits.touchdown_mask(pb["gait"], pb["tick"].astype(np.int64) + t + 1) for t in range(T)], axis=1)


# ------------------------------------------------------------------------------------------------------- 1. land = rule changes nothing
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_land_rule_changes_nothing(io):
    import torch
    ops, st, logs = _run(io, "rule")
    ref_st = ops.state()
    ref = ops.phase(ref_st, ROLL_T)
    torch.cuda.synchronize()
    for k in ("x", "ref", "feet", "tick"):
        assert torch.equal(st[k], ref_st[k]), k
    for k in PHASE_LOGS:
        assert torch.equal(logs[k], ref[k]), k
    assert int(ref["solved"].min()) > 0 and bool((st["tick"] == ROLL_T).all())


# --------------------------------------------------------------------------------------------------- 2. in the loop equals after the fact
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_in_the_loop_equals_after_the_fact(io):
    import torch
    growth = float(np.load(GROWTH_NPZ)["growth"])
    assert 1.0 <= growth < 1e3
    ops, st, logs = _run(io, "rule")
    sol, pb, rows, c = ops.sol, ops.pb, ops.rows, ops.const
    dt = sol.tdtype
    tick0 = _t(pb["tick"], torch.int32)
    sw = sol.phase_swing(logs, c["gait"], tick0, c["stand"], c["gain"], c["step_height"], want_des=False)
    torch.cuda.synchronize()
    h = _host_logs(logs)
    err, band = _error(logs["swing"].cpu().numpy(), sw["swing"].cpu().numpy().astype(np.float64), io)
    print(f"legs {io} swing_log against phase_swing on the logs: err {err:.3e} band {band:.1e}")
    assert err <= band
    # the host on the device's logs, with the pushed right-hand side
    wr = gaits.log_wrench(rows["push"], rows["push_ticks"], pb["tick"], ROLL_T)
    acc = lite3_model.plant_base_acc_host(h["actual"], h["forces"], h["feet_log"], rows["body"], wrench=wr)
    if io == "f32":
        acc = _r32(acc)                                                         # a base_acc row as the I/O type holds it (include/mpcqp_sim.h)
    assert np.abs(acc - lite3_model.plant_base_acc_host(h["actual"], h["forces"], h["feet_log"], rows["body"])).max() > 0.1   # (the pushes are in it)
    host = lite3_model.swing_track_host(h["actual"], h["forces"], h["feet_log"], h["contact_log"], h["swing"], acc, delta=DELTA)
    near = flag_margins(host)
    print(f"legs {io}: {int(near.sum())} of {near.size} (robot, tick, leg) within 1e-9 of a flag threshold")
    assert near.sum() <= 1e-3 * near.size
    assert np.array_equal(h["flag"][~near], host["flag"][~near])
    for k in TRACK_OUT[:5]:
        err, band = _error(logs[k].cpu().numpy(), host[k], io)
        print(f"legs {io} {k}_log against the host: err {err:.3e} band {band:.1e} x growth {growth:.1f} (max |{k}| {np.nanmax(np.abs(host[k])):.3f})")
        assert err <= band * growth, (k, err)
    err, band = _error(st["legs"].cpu().numpy(), host["state"], "f64")
    print(f"legs {io} final legs against the host: err {err:.3e} band {band:.1e} x growth {growth:.1f}")
    assert err <= band * growth
    up = h["contact_log"] == 0
    assert up.sum() > 100 and np.all((h["flag"][up] & 1) == 1) and np.all((h["flag"][~up] & 1) == 0)
    # device against device: swing_track on the same logs, told the pushed right-hand side
    state = torch.zeros((ROLL_B, 4, 7), dtype=dt, device="cuda")
    out = sol.swing_track(logs, logs["swing"], base_acc=_t(acc, dt), state=state)
    torch.cuda.synchronize()
    flag = out["flag"].cpu().numpy()
    assert np.array_equal(flag[~near], h["flag"][~near])
    for k in TRACK_OUT[:5]:
        err, band = _error(logs[k].cpu().numpy(), out[k].cpu().numpy().astype(np.float64), io)
        print(f"legs {io} {k}_log against swing_track on the device: err {err:.3e} band {band:.1e} x growth {growth:.1f}")
        assert err <= band * growth, (k, err)
    err, band = _error(state.cpu().numpy(), st["legs"].cpu().numpy(), io)
    print(f"legs {io} swing_track's final state against legs: err {err:.3e} band {band:.1e} x growth {growth:.1f}")
    assert err <= band * growth
    # the miss of a landing is what the landing row of the next tick logs as its err
    td = _touchdowns(pb, ROLL_T)
    assert td[:, :-1].sum() >= 2 * 14 and np.array_equal((h["flag"][:, 1:] & 64) != 0, td[:, :-1])
    assert np.all(h["miss"][~td] == 0.0) and np.all(h["miss"][td] > 1e-4)
    print(f"legs {io}: landing misses {np.round(h['miss'][td].min() * 1e3, 2)} to {np.round(h['miss'][td].max() * 1e3, 2)} mm over {int(td.sum())} landings")
    if io == "f64":
        err, band = _error(h["miss"][:, :-1][td[:, :-1]], h["err"][:, 1:][td[:, :-1]], io)
        print(f"legs {io} miss_log[t] against err_log[t + 1] on landing rows: err {err:.3e} band {band:.1e} x growth {growth:.1f}")
        assert err <= band * growth


# ------------------------------------------------------------------------------------------------- 3. land = actual, replayed row by row
@pytest.mark.gpu
def test_land_actual_replayed_row_by_row():
    rg = float(np.load(ROW_GROWTH_NPZ)["growth"])
    assert 1.0 <= rg < 1e3
    ops, st, logs = _run("f64", "actual")
    pb, rows = ops.pb, ops.rows
    h = _host_logs(logs)
    B, T = ROLL_B, ROLL_T
    after, host = replay_rows(h, pb, rows, pb["tick"])
    up = h["contact_log"] == 0
    both = up[:, :-1] & up[:, 1:]                                               # a swing row followed by a swing row: its state is logged next
    assert both.sum() > 100 and not np.isnan(h["q"]).any()
    for k, sl in (("q", slice(0, 3)), ("qd", slice(3, 6))):
        err, band = _error(h[k][:, 1:][both], after[:, :-1, :, sl][both], "f64")
        print(f"replay {k}_log[t + 1] from row t: err {err:.3e} band {band:.1e} x one-row growth {rg:.1f}")
        assert err <= band * rg, (k, err)
    # the landings: the state one tick on, from the logs and the final state
    nxt = np.concatenate([h["actual"][:, 1:], st["x"].cpu().numpy()[:, None, :12]], axis=1)
    feet_nxt = np.concatenate([h["feet_log"][:, 1:], st["feet"].cpu().numpy()[:, None]], axis=1)
    td = _touchdowns(pb, T)
    assert np.array_equal(td[:, :-1], up[:, :-1] & ~up[:, 1:]) and td.sum() >= 2 * 14
    flat = lambda a: a.reshape((B * T,) + a.shape[2:])
    p_act = gaits.leg_feet_host(flat(nxt), flat(after)).reshape(B, T, 4, 3)                 # the host's forward kinematics at the replayed q
    rep = lambda a: np.repeat(np.asarray(a), T, axis=0)
    rule = gaits.touchdown_foothold(flat(nxt)[:, 3:6], gaits.measured_yaw(flat(nxt)[:, 0:3]), flat(nxt)[:, 9:12], flat(h["desired"])[:, 9:12],
                                    rep(pb["stand"]), rep(pb["gain"]), rep(pb["gait"]), DELTA).reshape(B, T, 4, 3)
    err, band = _error(feet_nxt[td][:, :2], p_act[td][:, :2], "f64")
    print(f"landed feet xy against c + R p_foot(q): err {err:.3e} band {band:.1e}")
    assert err <= band
    assert np.array_equal(feet_nxt[td][:, 2], np.broadcast_to(pb["stand"][:, None, :, 2], (B, T, 4))[td])
    miss = np.linalg.norm(p_act - rule, axis=-1)
    err, band = _error(h["miss"][td], miss[td], "f64")
    print(f"miss_log against |p_act - touchdown_foothold(actual[t + 1])|: err {err:.3e} band {band:.1e}")
    assert err <= band and np.all(h["miss"][~td] == 0.0)
    assert np.array_equal(feet_nxt[~td], h["feet_log"][~td])                   # a foot that does not land is not written
    # against the land = rule run of the same robots: every stepping robot lands off the rule somewhere
    _, rst, rlogs = _run("f64", "rule")
    rfeet = np.concatenate([rlogs["feet_log"].cpu().numpy()[:, 1:], rst["feet"].cpu().numpy()[:, None]], axis=1)
    moved = np.linalg.norm((feet_nxt - rfeet)[..., :2], axis=-1)
    steps = td.any(axis=(1, 2))
    worst = np.array([moved[b][td[b]].max() if steps[b] else 0.0 for b in range(B)])
    print(f"landed feet against the land = rule run: largest xy difference per robot {np.round(worst * 1e3, 2)} mm")
    assert steps.sum() >= 14 and np.all(worst[steps] > 1e-6) and np.all(worst[~steps] == 0.0)
    print(f"solved per robot: land = actual {logs['solved'].cpu().numpy()}, land = rule {rlogs['solved'].cpu().numpy()}")


# ------------------------------------------------------------------------------------------------------------- 4. two pieces are one call
@pytest.mark.gpu
@pytest.mark.parametrize("cut", [5, 12])                                        # no leg of any gait lands at tick 5; a landing tick
def test_two_pieces_are_one_call(cut):
    import torch
    ops, st, whole = _run("f64", "actual")
    td = _touchdowns(ops.pb, ROLL_T)
    assert td[:, cut - 1].any() == (cut == 12)
    s2 = ops.state()
    first = ops.legs(s2, cut, "actual")
    torch.cuda.synchronize()
    live = s2["legs"][:, :, 6].cpu().numpy()
    assert live.any() and bool((s2["tick"] == cut).all())                       # legs in mid-swing cross the cut
    second = ops.legs(s2, ROLL_T - cut, "actual")
    torch.cuda.synchronize()
    for k in PHASE_LOGS[:5] + LEG_LOGS:
        assert torch.equal(torch.cat([first[k], second[k]], dim=1), whole[k]), (cut, k)
    assert torch.equal(first["solved"] + second["solved"], whole["solved"])
    for k in STATE:
        assert torch.equal(s2[k], st[k]), (cut, k)


# ---------------------------------------------------------------------------------------------------- 5. arguments, NULLs and poison
def _raw(ops, st, T, land, logs, drop=(), over=None):
    """mpcqp_rollout_legs through the raw binding: `logs` {name: tensor}, the names in `drop` passed as NULL; `over` {name: value} replaces arguments."""
    c = ops.const
    a = {"B": ops.B, "T": T, "x": st["x"].data_ptr(), "ref": st["ref"].data_ptr(), "feet": st["feet"].data_ptr(), "legs": st["legs"].data_ptr(),
         "gait": c["gait"].data_ptr(), "stand": c["stand"].data_ptr(), "gain": c["gain"].data_ptr(), "tick": st["tick"].data_ptr(),
         "mu": c["mu"].data_ptr(), "body": c["body"].data_ptr(), "push": c["push"].data_ptr(), "push_ticks": c["push_ticks"].data_ptr(),
         "substeps": 10, "step_height": c["step_height"].data_ptr(), "gains": 0, "leg_substeps": 0, "land": land}
    a.update(over or {})
    names = PHASE_LOGS + LEG_LOGS
    ops.sol.engine.rollout_legs_ptr(*a.values(), *[0 if k in drop else logs[k].data_ptr() for k in names])


@pytest.mark.gpu
def test_null_logs_arguments_and_noops():
    import torch
    ops, _, _ = _run("f64", "actual")
    T = 8                                                                       # lift-offs, swing rows and the landings at tick 6
    st = ops.state()
    full = ops.legs(st, T, "actual")
    torch.cuda.synchronize()
    names = PHASE_LOGS + LEG_LOGS
    assert bool((full["miss"] > 0).any())
    for drop in [(k,) for k in names] + [names]:
        s2 = ops.state()
        bufs = {k: torch.full_like(full[k], 7) for k in names}
        _raw(ops, s2, T, 1, bufs, drop)
        torch.cuda.synchronize()
        for k in names:
            assert bool((bufs[k] == 7).all()) if k in drop else torch.equal(bufs[k], full[k]), (drop, k)
        for k in STATE:
            assert torch.equal(s2[k], st[k]), (drop, k)
    s2 = ops.state()
    keep = {k: v.clone() for k, v in s2.items()}
    for over, msg in (({"land": 2}, "land"), ({"land": -1}, "land"), ({"leg_substeps": -1}, "leg_substeps"), ({"leg_substeps": 1001}, "leg_substeps"),
                      ({"legs": 0}, "null buffer"), ({"step_height": 0}, "null buffer"), ({"push_ticks": 0}, "push without push_ticks"),
                      ({"substeps": 1001}, "substeps"), ({"T": -1}, "size"), ({"B": -1}, "size")):
        with pytest.raises(mpcqp.MpcQpError, match=rf"-1.*mpcqp_rollout_legs: .*{msg}"):
            _raw(ops, s2, T, 1, full, over=over)
    _raw(ops, s2, 0, 1, full)                                                   # no ticks, no robots: no-ops
    _raw(ops, s2, T, 1, full, over={"B": 0})
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(s2[k], keep[k]), k
    with pytest.raises(ValueError, match="land"):
        ops.legs(s2, T, "landed")
    with pytest.raises(ValueError, match="legs"):
        ops.legs(dict(s2, legs=s2["legs"].float()), T, "rule")


@pytest.mark.gpu
def test_a_block_that_is_not_full():
    """B = 33: 132 lanes in one block of 256, whole quads; every swing row replays on the host and nothing is NaN."""
    import torch
    rg = float(np.load(ROW_GROWTH_NPZ)["growth"])
    B, T = 33, 13
    pb, rows = _case("f64", B)
    ops = _Ops(mpcqp.MPCBatch(N=10, delta=DELTA, io_dtype="f64", precision="mixed"), pb, rows)
    st = ops.state()
    logs = ops.legs(st, T, "actual")
    torch.cuda.synchronize()
    h = _host_logs(logs)
    assert not any(np.isnan(h[k]).any() for k in LEG_LOGS if k != "flag") and not np.any(h["flag"] == 0xff)
    after, _ = replay_rows(h, pb, rows, pb["tick"])
    up = h["contact_log"] == 0
    both = up[:, :-1] & up[:, 1:]
    assert both[32].any() and both.sum() > 200
    for k, sl in (("q", slice(0, 3)), ("qd", slice(3, 6))):
        err, band = _error(h[k][:, 1:][both], after[:, :-1, :, sl][both], "f64")
        print(f"B = 33 replay {k}: err {err:.3e} band {band:.1e} x one-row growth {rg:.1f}")
        assert err <= band * rg, (k, err)
    err, band = _error(st["legs"].cpu().numpy()[:, :, :6], after[:, -1, :, :6], "f64")
    assert err <= band * rg and bool((st["tick"] == T).all())


@pytest.mark.gpu
@pytest.mark.parametrize("land", ["actual", "rule"])
def test_a_poisoned_gains_row(land):
    import torch
    ops, st, clean = _run("f64", land)
    r = 1                                                                       # a flying trot: it steps
    gains = np.tile([[lite3_model.SWING_KP, lite3_model.SWING_KD]], (ROLL_B, 1)); gains[r, 0] = np.nan
    s2 = ops.state()
    logs = ops.legs(s2, ROLL_T, land, gains=_t(gains, ops.sol.tdtype))
    torch.cuda.synchronize()
    others = torch.arange(ROLL_B, device="cuda") != r
    for k in PHASE_LOGS + LEG_LOGS:                                             # (default gains given as a row are the default gains)
        assert torch.equal(logs[k][others], clean[k][others]), k
    for k in STATE:
        assert torch.equal(s2[k][others], st[k][others]), k
    for k in ("q", "qd", "tau", "foot", "err"):
        assert bool(torch.isnan(logs[k][r]).all()), k
    assert bool((logs["flag"][r] == 0xff).all()) and torch.equal(logs["swing"][r, 0], clean["swing"][r, 0])
    td = _touchdowns(ops.pb, ROLL_T)[r]
    t0 = int(np.nonzero(td.any(axis=1))[0][0])                                  # the first landing happens after row t0
    miss = logs["miss"][r].cpu().numpy()
    assert np.all(np.isnan(miss[td])) and np.all(miss[~td] == 0.0)
    solved, clean_solved = int(logs["solved"][r]), int(clean["solved"][r])
    print(f"poisoned gains, land = {land}: robot {r} first lands after row {t0}, solved {solved} of {ROLL_T} (clean run {clean_solved})")
    if land == "actual":                                                        # the NaN foot reaches the next solve, and every one after
        assert solved <= t0 + 1 < clean_solved
        assert bool(torch.isnan(s2["feet"][r]).any())
    else:                                                                       # the poisoned leg never reaches x or feet
        for k in PHASE_LOGS:
            assert torch.equal(logs[k][r], clean[k][r]), k
        for k in ("x", "ref", "feet", "tick"):
            assert torch.equal(s2[k][r], st[k][r]), k
        assert bool(torch.isnan(s2["legs"][r, :, :6]).any())


def test_the_checker_library_names_the_missing_header(oracle_lib):
    capi = mpcqp._capi
    assert not oracle_lib.has_legroll and not oracle_lib.has_sim and not hasattr(oracle_lib.lib, "mpcqp_rollout_legs")
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    with pytest.raises(mpcqp.MpcQpError, match=rf"mpcqp_rollout_legs: {re.escape(oracle_lib.path)} does not export include/mpcqp_sim.h \(product library only\)"):
        eng.rollout_legs_ptr(1, 1, *([0] * 31))
    plib = mpcqp.product_library()
    assert plib.has_sim and plib.has_legroll and set(capi.LEGROLL_SYMBOLS) <= set(capi.SIM_SYMBOLS)
    assert capi.LAND_RULE == 0 and capi.LAND_ACTUAL == 1
