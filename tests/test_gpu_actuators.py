"""Per-robot actuator rows with a torque-speed curve on the device (include/mpcqp_actuators.h, mpcqp_set_actuators).

  1. stance_drive with a table against lite3_model.stance_drive_host on actuator_cases.drive_draw(): 33 robots (132 legs, a partial
     block), one row per robot, legs clamped on the falling part of their curve and at tau_max, an invalid row; both I/O dtypes.
  2. The flat table is no table: stance_drive, swing_track, leg_effort, rollout_legs and rollout_drive give the no-table bits with
     actuators.actuator_rows(B) set, and again after clear_actuators.
  3. Row by row, zero tolerance: rollout_drive (limited, land = actual) on legsim_cases.rollout_batch() with four classes of rows cycling
     through the 16 robots against no-table runs (the flat classes) and runs with one row tiled over the batch (the curved ones).
  4. The logs of 3 replay through stance_drive with the table tiled (bit for bit) and through swing_track (the bands of
     tests/test_gpu_rollout_legs.py); two pieces are one call.
  5. Arguments, the gate, a table set and used on one side stream.

Bands: those of tests/test_gpu_stance_drive.py and tests/test_gpu_rollout_legs.py times max(1, growth factor), the host's own
sensitivity recorded in tests/golden/actuator_growth.npz by tests/test_actuators_host.py (draw 39.4: outputs per unit of the stance rate;
roll-out 53.7: swing_track_host over the 25 rows with the table of 3)."""
import numpy as np
import pytest

import actuator_cases as ac
import drive_cases as dc
import legsim_cases
import mpcqp
import test_gpu_rollout_legs as rl
import test_gpu_stance_drive as sd
from legsim_cases import DELTA, ROLL_B, ROLL_T
from mpcqp import actuators, gaits, lite3_model

_t, _np, _r32 = sd._t, sd._np, sd._r32
_CACHE = {}
STATE, ALL_LOGS = sd.STATE, sd.ALL_LOGS + ("cmd",)


def _ops(io, B=ROLL_B):
    """The operands of tests/test_gpu_stance_drive.py on an engine of this module's own: a table left behind reaches no other module."""
    if ("ops", io, B) not in _CACHE:
        _CACHE[("ops", io, B)] = sd._Ops(io, B)
    return _CACHE[("ops", io, B)]


def _eq(a, b):
    return np.array_equal(_np(a), _np(b), equal_nan=True)


# ---------------------------------------------------------------------------------------------------- 1. stance_drive against the host
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_stance_drive_with_a_table_against_the_host(io):
    import torch
    growth = max(1.0, ac.recorded_growth()["draw"])
    c = ac.as_io(ac.drive_draw(), np.float64 if io == "f64" else np.float32)
    host = ac.drive(c)
    B, b = c["x"].shape[0], ac.INVALID_ROBOT
    sol = mpcqp.MPCBatch(io_dtype=io)
    dt = sol.tdtype
    x, f, feet, ground = (_t(c[k], dt) for k in ("x", "f", "feet", "ground"))
    contact = _t(c["contact"], torch.uint8)
    sol.set_actuators(c["rows"])
    out = sol.stance_drive(x, f, feet, contact, ground)
    mended = c["rows"].copy()
    mended[b] = actuators.actuator_rows(1)[0]
    sol.set_actuators(_t(mended, torch.float64))                                # (a device tensor is taken as it is)
    ref = sol.stance_drive(x, f, feet, contact, ground)
    torch.cuda.synchronize()
    dev = {"f": _np(out["f"]).reshape(-1, 4, 3), "tau": _np(out["tau"]), "flag": _np(out["flag"])}
    st = c["contact"] != 0
    near = dc.near_threshold(host)
    print(f"stance_drive with a table {io}: {int(near.sum())} of {near.size} legs within FLAG_MARGIN of a threshold")
    assert near.mean() <= dc.MARGIN_SHARE
    keep = ~near
    assert np.array_equal(dev["flag"][keep], host["flag"][keep])
    f_in, hf = _np(f).reshape(-1, 4, 3), host["f"].reshape(-1, 4, 3)
    free = keep & ((host["flag"] & 34) == 0)                                    # untouched forces keep their bits
    assert np.array_equal(dev["f"][free], f_in[free], equal_nan=True)
    rest = keep & ~free
    for k, d, h in (("f_out", dev["f"], hf), ("tau", dev["tau"], host["tau"])):
        err, band = sd._error(d[rest], h[rest], io)
        print(f"stance_drive with a table {io} {k}: err {err:.3e} band {band:.1e} x growth {growth:.1f} on {int(rest.sum())} legs")
        assert err <= band * growth, (k, err)
    err, band = sd._error(dev["tau"][free], host["tau"][free], io)
    assert err <= band
    app = actuators.clamp_host(c["rows"], host["tau_cmd"], host["rate"])
    fall, flat, moving = ac.classify(c["rows"], host["tau_cmd"], app, host["rate"])
    live = st & (host["flag"] != 0xff)
    assert (fall & live).sum() >= 20 and (flat & live).sum() >= 10 and (moving & live).sum() >= 10
    # the invalid row: NaN / 0xff on its robot's stance legs, its swing legs keep their forces, every other robot as without it
    assert st[b].any() and np.all(dev["flag"][b][st[b]] == 0xff) and np.isnan(dev["f"][b][st[b]]).all() and np.isnan(dev["tau"][b][st[b]]).all()
    assert np.array_equal(dev["f"][b][~st[b]], f_in[b][~st[b]]) and not np.any(dev["flag"][np.arange(B) != b] == 0xff)
    others = torch.ones(B, dtype=torch.bool, device="cuda")
    others[b] = False
    for k in ("f", "tau", "flag"):
        assert torch.equal(out[k][others], ref[k][others]), k
    assert not bool(torch.isnan(ref["f"][b]).any())


# ------------------------------------------------------------------------------------------------------ 2. the flat table is no table
def _track_ops(sol, s):
    import torch
    dt = sol.tdtype
    logs = {"actual": _t(s["actual"], dt), "forces": _t(s["forces"], dt), "feet_log": _t(s["feet_log"], dt),
            "contact_log": _t(s["contact_log"], torch.uint8)}
    return logs, _t(s["swing"], dt), _t(s["base_acc"], dt)


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_the_flat_table_is_no_table(io):
    import torch
    ops = _ops(io)
    sol, dt = ops.sol, ops.sol.tdtype
    c = dc.as_io(dc.clamp_draw(), np.float64 if io == "f64" else np.float32)
    x, f, feet, ground = (_t(c[k], dt) for k in ("x", "f", "feet", "ground"))
    contact = _t(c["contact"], torch.uint8)
    logs, swing, acc = _track_ops(sol, legsim_cases.turning_logs())
    vel, accf = swing[:, :, :, 1].contiguous(), swing[:, :, :, 2].contiguous()

    def run_all(table):
        """Every call that reads the table, each with a flat table of its own size set (table) or with none."""
        put = (lambda B: sol.set_actuators(actuators.actuator_rows(B))) if table else (lambda B: None)
        out = {}
        put(33)
        out["stance"] = sol.stance_drive(x, f, feet, contact, ground)
        put(2)
        state = torch.zeros((2, 4, 7), dtype=dt, device="cuda")
        out["track"] = dict(sol.swing_track(logs, swing, base_acc=acc, state=state), state=state)
        out["effort"] = sol.leg_effort(logs["actual"], logs["forces"], swing[:, :, :, 0].contiguous(), vel, accf, base_acc=acc)
        put(ROLL_B)
        a, b = ops.state(), ops.state()
        out["legs"] = dict(ops.legs(a, ROLL_T, "actual"), **a)
        out["drive"] = dict(ops.drive(b, ROLL_T, "rule", "limited", ops.ground), **b)
        torch.cuda.synchronize()
        return out

    ref = run_all(False)
    flat = run_all(True)
    sol.clear_actuators()
    sol.clear_actuators()                                                       # (twice: the second is a no-op)
    again = run_all(False)
    for name, other in (("flat table", flat), ("after clear_actuators", again)):
        for call in ref:
            assert set(ref[call]) == set(other[call])
            for k in ref[call]:
                assert _eq(ref[call][k], other[call][k]), (name, call, k)
    # not vacuous: the draw clamps about half its stance legs and the limited roll-out on slippery ground changes forces
    assert int(((ref["stance"]["flag"] & 2) != 0).sum()) >= 20 and not torch.equal(ref["drive"]["cmd"], ref["drive"]["forces"])
    assert int((ref["effort"]["limit"] != 0xff).sum()) > 0 and int(ref["drive"]["solved"].min()) > 0


# ---------------------------------------------------------------------------------------------------- 3. row by row, zero tolerance
def _mixed(io):
    """The roll-out under the four classes cycling through the robots, once per I/O dtype: (ops, final state, logs)."""
    import torch
    if ("mixed", io) not in _CACHE:
        ops = _ops(io)
        ops.sol.set_actuators(ac.rollout_rows())
        st = ops.state()
        logs = ops.drive(st, ROLL_T, "actual", "limited", None)
        torch.cuda.synchronize()
        ops.sol.clear_actuators()
        _CACHE[("mixed", io)] = (ops, st, logs)
    return _CACHE[("mixed", io)]


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_a_mixed_table_row_by_row(io):
    import torch
    ops, st, logs = _mixed(io)
    sol = ops.sol
    refs = {}
    for c, (scale, knee, free) in enumerate(ac.CLASSES):
        s = ops.state()
        if np.isinf(knee):                                                      # a flat class: no table, the inertia row with tau_max scaled
            out = ops.drive(s, ROLL_T, "actual", "limited", None, inertia=dc.weak_row(scale))
        else:                                                                   # a curved class: that one row tiled over the batch
            sol.set_actuators(ac.rows_of((ac.CLASSES[c],), ROLL_B))
            out = ops.drive(s, ROLL_T, "actual", "limited", None)
        torch.cuda.synchronize()
        sol.clear_actuators()
        refs[c] = (s, out)
    for b in range(ROLL_B):
        s, out = refs[b % 4]
        for k in STATE:
            assert _eq(st[k][b], s[k][b]), (b, k)
        for k in ALL_LOGS:
            assert _eq(logs[k][b], out[k][b]), (b, k)
    flag, stance = _np(logs["flag"]), _np(logs["contact_log"]) != 0
    cl = ((flag & 2) != 0) & (flag != 0xff)
    cls = np.arange(ROLL_B) % 4
    swing_rows, stance_rows = [int((cl & ~stance)[cls == c].sum()) for c in range(4)], [int((cl & stance)[cls == c].sum()) for c in range(4)]
    print(f"mixed roll-out {io}: clamped swing rows per class {swing_rows}, clamped stance rows {stance_rows}; solved {logs['solved'].tolist()}")
    assert swing_rows[2] > 0 and stance_rows[3] > 0 and swing_rows[0] == 0
    assert not _eq(refs[0][1]["q"], refs[2][1]["q"])                            # the curve changes what the legs do


# ------------------------------------------------------------------------------------------------------------------- 4. replay
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_the_logs_replay_with_the_table(io):
    import torch
    growth = max(1.0, ac.recorded_growth()["rollout"])
    ops, st, logs = _mixed(io)
    sol, B, T, dt = ops.sol, ROLL_B, ROLL_T, ops.sol.tdtype
    table = ac.rollout_rows()
    rows = B * T
    # (a) the stance rule on the logged rows, the table tiled
    sol.set_actuators(actuators.tile(table, T))
    rep = sol.stance_drive(logs["actual"].reshape(rows, 12), logs["cmd"].reshape(rows, 12), logs["feet_log"].reshape(rows, 4, 3),
                           logs["contact_log"].reshape(rows, 4), None)
    torch.cuda.synchronize()
    s = (logs["contact_log"] != 0).reshape(rows, 4)
    assert torch.equal(rep["f"], logs["forces"].reshape(rows, 12))
    assert torch.equal(rep["tau"][s], logs["tau"].reshape(rows, 4, 3)[s])
    assert torch.equal(rep["flag"][s] & dc.BITS, logs["flag"].reshape(rows, 4)[s] & dc.BITS)
    assert int(((rep["flag"][s] & 2) != 0).sum()) > 0 and not torch.equal(logs["cmd"], logs["forces"])
    # (b) the swing rows through swing_track on the roll-out's own logs, told the pushed right-hand side
    h = rl._host_logs(logs)
    wr = gaits.log_wrench(ops.rows["push"], ops.rows["push_ticks"], ops.pb["tick"], T)
    acc = lite3_model.plant_base_acc_host(h["actual"], h["forces"], h["feet_log"], ops.rows["body"], wrench=wr)
    if io == "f32":
        acc = _r32(acc)
    sol.set_actuators(table)
    state = torch.zeros((B, 4, 7), dtype=dt, device="cuda")
    out = sol.swing_track(logs, logs["swing"], base_acc=_t(acc, dt), state=state)
    torch.cuda.synchronize()
    host = lite3_model.swing_track_host(h["actual"], h["forces"], h["feet_log"], h["contact_log"], h["swing"], acc, delta=DELTA, actuators=table)
    near = legsim_cases.flag_margins(host)
    print(f"replay {io}: {int(near.sum())} of {near.size} (robot, tick, leg) within 1e-9 of a flag threshold")
    assert near.sum() <= 1e-3 * near.size
    up = h["contact_log"] == 0                                                  # (a stance row's tau and bits 2 / 16 / 32 are the rule's, (a))
    keep = ~near & up
    assert np.array_equal(_np(out["flag"])[keep], h["flag"][keep]) and np.array_equal(host["flag"][keep], h["flag"][keep])
    for k in ("q", "qd", "foot", "err"):
        for name, other in (("swing_track on the device", _np(out[k])), ("the host", host[k])):
            err, band = rl._error(_np(logs[k]), other, io)
            print(f"replay {io} {k}_log against {name}: err {err:.3e} band {band:.1e} x growth {growth:.1f}")
            assert err <= band * growth, (k, name, err)
    for name, other in (("swing_track on the device", _np(out["tau"])), ("the host", host["tau"])):
        err, band = rl._error(_np(logs["tau"])[up], other[up], io)
        print(f"replay {io} tau_log of the swing rows against {name}: err {err:.3e} band {band:.1e} x growth {growth:.1f}")
        assert err <= band * growth, (name, err)
    assert int((((h["flag"] & 2) != 0) & up).sum()) > 0
    # (c) two pieces are one call
    p = ops.state()
    p1 = ops.drive(p, 3, "actual", "limited", None)
    p2 = ops.drive(p, T - 3, "actual", "limited", None)
    torch.cuda.synchronize()
    sol.clear_actuators()
    for k in STATE:
        assert torch.equal(p[k], st[k]) or _eq(p[k], st[k]), k
    for k in ALL_LOGS:
        if k == "solved":
            assert torch.equal(p1[k] + p2[k], logs[k])
        else:
            assert _eq(torch.cat([p1[k], p2[k]], dim=1), logs[k]), k


# ---------------------------------------------------------------------------------------------------------------- 5. arguments
@pytest.mark.gpu
def test_arguments_the_gate_and_a_side_stream():
    import torch
    plib = mpcqp.product_library()
    assert plib.has_actuators and all(plib.calls[s][0] is not None for s in mpcqp._capi.ACTUATOR_SYMBOLS)
    io, B, T = "f32", 12, 6
    ops = _ops(io, B)
    sol = ops.sol
    c = dc.as_io(dc.clamp_draw(), np.float32)
    x, f, feet = (_t(c[k], sol.tdtype) for k in ("x", "f", "feet"))
    contact = _t(c["contact"], torch.uint8)
    sol.set_actuators(actuators.actuator_rows(B + 1))
    with pytest.raises(mpcqp.MpcQpError, match=rf"code -1: mpcqp_rollout_drive: batch size {B}, but the actuator table has {B + 1} rows"):
        ops.drive(ops.state(), T, "rule", "limited", None)
    with pytest.raises(mpcqp.MpcQpError, match=rf"code -1: mpcqp_rollout_legs: batch size {B}, but the actuator table has {B + 1} rows"):
        ops.legs(ops.state(), T)
    with pytest.raises(mpcqp.MpcQpError, match=rf"code -1: mpcqp_stance_drive: batch size 33, but the actuator table has {B + 1} rows"):
        sol.stance_drive(x, f, feet, contact, None)
    logs, swing, acc = _track_ops(sol, legsim_cases.turning_logs())
    with pytest.raises(mpcqp.MpcQpError, match=rf"code -1: mpcqp_swing_track: batch size 2, but the actuator table has {B + 1} rows"):
        sol.swing_track(logs, swing, base_acc=acc)
    with pytest.raises(mpcqp.MpcQpError, match=rf"code -1: mpcqp_leg_effort: batch size 2, but the actuator table has {B + 1} rows"):
        sol.leg_effort(logs["actual"], logs["forces"], swing[:, :, :, 0].contiguous(), base_acc=acc)
    sol.clear_actuators()
    rows = _t(actuators.actuator_rows(B), torch.float64)
    with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_set_actuators: null actuator table"):
        sol.engine.set_actuators_ptr(B, 0)
    for bad in (0, -3):
        with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_set_actuators: batch size out of range"):
            sol.engine.set_actuators_ptr(bad, rows.data_ptr())
    with pytest.raises(ValueError, match="operand mismatch: rows"):
        sol.set_actuators(np.zeros((B, 8)))
    with pytest.raises(ValueError, match="operand mismatch: rows"):
        sol.set_actuators(rows.to(torch.float32))
    ops.drive(ops.state(), 1, "rule", "limited", None)                          # none of the refused calls left a table behind
    # a table set on a side stream and a roll-out on that stream right behind it: no synchronisation in between
    table = ac.rows_of(ac.CLASSES, B)
    sol.set_actuators(table)
    a = ops.state()
    ref = ops.drive(a, T, "actual", "limited", None)
    torch.cuda.synchronize()
    sol.clear_actuators()
    side = torch.cuda.Stream()
    b = ops.state()
    dev_rows = _t(table, torch.float64)
    torch.cuda.synchronize()                                                    # (the operands above were made on the current stream)
    sol.set_actuators(dev_rows, stream=side)
    out = ops.drive(b, T, "actual", "limited", None, stream=side)
    side.synchronize()
    sol.clear_actuators()
    for k in STATE:
        assert _eq(a[k], b[k]), k
    for k in ALL_LOGS:
        assert _eq(ref[k], out[k]), k
    cl = (out["flag"] & 2) != 0
    assert int(cl[out["flag"] != 0xff].sum()) > 0
