"""Every reader of the actuator table with rows that differ per robot (include/mpcqp_actuators.h, mpcqp_set_actuators); the cases are in
tests/actuator_cases.py and their conditions are held on the CPU checker by tests/test_actuator_rows_host.py.

  1. leg_effort with one row per robot at T = 4 against lite3_model.leg_effort_host: the limit byte of every leg, byte for byte.
  2. The conversion kernel over three blocks (627 rows of stance_drive): every invalid kind, the valid edge rows, against the host.
  3. rollout_legs (land = rule and actual) with four classes of rows cycling through the robots, row by row against uniform runs; the
     ideal drive with the table.
  4. Model rows, actuator rows and ground rows in one rollout_drive: row by row, under permutations of the robots (B = 16 and the queued
     launch at B = 2560), and replayed through stance_drive and solve_batch_phase.
  5. An invalid row inside a roll-out, clause by clause, in the four modes of actuator_cases.LOOP_MODES, device against device.
  6. Table lifetime on one stream without synchronisation: a second table, a smaller table after a larger one, growth after use.

No tolerance is new: comparisons are bit for bit, or in the bands of tests/test_gpu_stance_drive.py times the growth recorded in
tests/golden/actuator_growth.npz, or (the replayed solves of 4) at the 1e-4 band of tests/batch_checks.py."""
import numpy as np
import pytest

import actuator_cases as ac
import drive_cases as dc
import legsim_cases
import models_rollout_cases as C
import mpcqp
import test_gpu_models_rollouts as mr
import test_gpu_stance_drive as sd
from legsim_cases import DELTA, ROLL_B, ROLL_T, STEP_HEIGHT
from mpcqp import actuators

_t, _np = sd._t, sd._np
_CACHE = {}
STATE, ALL_LOGS = sd.STATE, sd.ALL_LOGS + ("cmd",)
LEG_NAN_LOGS = ("q", "qd", "tau", "foot", "err")


def _ops(io, B=ROLL_B):
    """The operands of tests/test_gpu_stance_drive.py on an engine of this module's own: a table left behind reaches no other module."""
    if ("ops", io, B) not in _CACHE:
        _CACHE[("ops", io, B)] = sd._Ops(io, B)
    return _CACHE[("ops", io, B)]


def _eq(a, b):
    return np.array_equal(_np(a), _np(b), equal_nan=True)


def _same_robot(what, got, ref, b, keys):
    """Robot b of two results (device tensors or numpy arrays), bit for bit."""
    host = lambda a: _np(a) if hasattr(a, "cpu") else a
    for k in keys:
        assert np.array_equal(host(got[k][b]), host(ref[k][b]), equal_nan=True), (what, b, k)


# --------------------------------------------------------------------------------------------------- 1. leg_effort, one row per robot
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_leg_effort_with_one_row_per_robot_against_the_host(io):
    import torch
    s, rows = ac.effort_case(io)
    B, T = s["actual"].shape[:2]
    b = ac.INVALID_ROBOT
    sol = mpcqp.MPCBatch(io_dtype=io)
    d = {k: _t(s[k], sol.tdtype) for k in ac.EFFORT_IN}
    try:
        for what, drop in ac.EFFORT_VARIANTS:
            args = [None if k in drop else d[k] for k in ac.EFFORT_IN]
            plain = sol.leg_effort(*args)
            sol.set_actuators(rows)
            dev = sol.leg_effort(*args)
            sol.set_actuators(np.roll(rows, 1, axis=0))
            rolled = sol.leg_effort(*args)
            torch.cuda.synchronize()
            sol.clear_actuators()
            host = ac.effort_host(s, rows, drop)
            margin = ac.effort_margin(host, rows)
            assert (margin > legsim_cases.FLAG_MARGIN).all()                     # no leg is left out
            limit, host_rolled = _np(dev["limit"]), ac.effort_host(s, np.roll(rows, 1, axis=0), drop)["limit"]
            differ = int((limit != host["limit"]).sum())
            print(f"leg_effort with a table {io} {what}: {differ} of {limit.size} limit bytes differ from the host's; smallest margin {margin.min():.2e}")
            assert np.array_equal(limit, host["limit"]), what
            for k in ("qdd", "tau_dyn", "tau", "power"):                         # the table changes the limit byte only
                assert torch.equal(dev[k], plain[k]) or _eq(dev[k], plain[k]), (what, k)
            assert np.all(limit[b] == 0xff) and not np.any(limit[np.arange(B) != b] == 0xff) and not np.any(_np(plain["limit"]) == 0xff)
            assert np.array_equal(_np(rolled["limit"]), host_rolled), what
            moved_host = int((host_rolled != host["limit"]).any(axis=(1, 2)).sum())
            moved = int((_np(rolled["limit"]) != limit).any(axis=(1, 2)).sum())
            assert moved_host >= ac.EFFORT_ROBOTS_MOVED and moved >= ac.EFFORT_ROBOTS_MOVED   # (the floor is the host test's)
    finally:
        sol.clear_actuators()


# ------------------------------------------------------------------------------------------------------- 2. the conversion, 627 rows
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_the_conversion_kernel_across_blocks_every_invalid_kind_and_the_valid_edges(io):
    import torch
    growth = max(1.0, ac.recorded_growth()["draw"])
    case, mended, bad = ac.conversion_case()
    c = ac.as_io(case, np.float64 if io == "f64" else np.float32)
    host = ac.drive(c)
    n = c["x"].shape[0]
    sol = mpcqp.MPCBatch(io_dtype=io)
    dt = sol.tdtype
    x, f, feet, ground = (_t(c[k], dt) for k in ("x", "f", "feet", "ground"))
    contact = _t(c["contact"], torch.uint8)
    try:
        sol.set_actuators(c["rows"])
        out = sol.stance_drive(x, f, feet, contact, ground)
        sol.set_actuators(mended)
        ref = sol.stance_drive(x, f, feet, contact, ground)
        torch.cuda.synchronize()
    finally:
        sol.clear_actuators()
    dev = {"f": _np(out["f"]).reshape(-1, 4, 3), "tau": _np(out["tau"]), "flag": _np(out["flag"])}
    st = c["contact"] != 0
    near = dc.near_threshold(host)
    print(f"conversion case {io}: {int(near.sum())} of {near.size} legs within FLAG_MARGIN of a threshold")
    assert near.mean() <= dc.MARGIN_SHARE
    keep = ~near
    assert np.array_equal(dev["flag"][keep], host["flag"][keep])
    f_in, hf = _np(f).reshape(-1, 4, 3), host["f"].reshape(-1, 4, 3)
    free = keep & ((host["flag"] & 34) == 0)                                    # untouched forces keep their bits
    assert np.array_equal(dev["f"][free], f_in[free], equal_nan=True)
    rest = keep & ~free
    for k, dv, h in (("f_out", dev["f"], hf), ("tau", dev["tau"], host["tau"])):
        err, band = sd._error(dv[rest], h[rest], io)
        print(f"conversion case {io} {k}: err {err:.3e} band {band:.1e} x growth {growth:.1f} on {int(rest.sum())} legs")
        assert err <= band * growth, (k, err)
    err, band = sd._error(dev["tau"][free], host["tau"][free], io)
    assert err <= band
    # every invalid row, whatever its kind and wherever it sits in its block: NaN / 0xff on its stance legs, its swing legs' forces kept
    assert n == 627 and st[bad].any(axis=1).all() and (~st[bad]).any()
    for r in np.nonzero(bad)[0]:
        assert np.all(dev["flag"][r][st[r]] == 0xff) and np.isnan(dev["f"][r][st[r]]).all() and np.isnan(dev["tau"][r][st[r]]).all(), r
        assert np.array_equal(dev["f"][r][~st[r]], f_in[r][~st[r]]), r
    assert not np.any(dev["flag"][~bad] == 0xff)                                # the valid edge rows among them
    e = list(ac.CONV_EDGES)
    assert np.isfinite(dev["tau"][e]).all() and np.all((dev["flag"][e[0]] & 2) != 0)
    # with the ten rows mended every other row is what it was
    others = torch.as_tensor(~bad).cuda()
    for k in ("f", "tau", "flag"):
        assert torch.equal(out[k][others], ref[k][others]), k
    assert not bool((ref["flag"] == 0xff).any()) and not bool(torch.isnan(ref["f"]).any())


# ------------------------------------------------------------------------------------------------- 3. rollout_legs, row by row
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_rollout_legs_and_the_ideal_drive_row_by_row(io):
    import torch
    ops = _ops(io)
    sol = ops.sol
    table = ac.rollout_rows()
    cls = np.arange(ROLL_B) % 4
    try:
        for land in ("rule", "actual"):
            sol.set_actuators(table)
            st, sti = ops.state(), ops.state()
            logs = ops.legs(st, ROLL_T, land)
            ideal = ops.drive(sti, ROLL_T, land, "ideal", None)
            torch.cuda.synchronize()
            sol.clear_actuators()
            refs = {}
            for c, (scale, knee, free) in enumerate(ac.CLASSES):
                s = ops.state()
                if np.isinf(knee):                                              # a flat class: no table, the inertia row with tau_max scaled
                    out = ops.legs(s, ROLL_T, land, inertia=dc.weak_row(scale))
                else:                                                           # a curved class: that one row tiled over the batch
                    sol.set_actuators(ac.rows_of((ac.CLASSES[c],), ROLL_B))
                    out = ops.legs(s, ROLL_T, land)
                torch.cuda.synchronize()
                sol.clear_actuators()
                refs[c] = (s, out)
            for b in range(ROLL_B):
                s, out = refs[b % 4]
                _same_robot(f"rollout_legs({land}) state", st, s, b, STATE)
                _same_robot(f"rollout_legs({land}) logs", logs, out, b, sd.ALL_LOGS)
            # the ideal drive without a ground reads the table as rollout_legs does
            for k in STATE:
                assert _eq(st[k], sti[k]), (land, k)
            for k in sd.ALL_LOGS:
                assert _eq(logs[k], ideal[k]), (land, k)
            assert torch.equal(ideal["cmd"], ideal["forces"])
            flag, up = _np(logs["flag"]), _np(logs["contact_log"]) == 0
            cl = ((flag & 2) != 0) & (flag != 0xff)
            per = [int((cl & up)[cls == c].sum()) for c in range(4)]
            print(f"rollout_legs({land}) {io} with mixed rows: clamped swing rows per class {per}; solved {logs['solved'].tolist()}")
            assert per[2] > 0 and per[3] > 0 and per[0] == 0 and not (cl & ~up).any() and int(logs["solved"].min()) > 0
            assert not _eq(refs[0][1]["q"], refs[2][1]["q"])                    # the curve changes what the legs do
        # the ideal drive on slippery ground skips the stance clamp, not the swing one
        sol.set_actuators(table)
        a, b = ops.state(), ops.state()
        slip = ops.drive(a, ROLL_T, "rule", "ideal", ops.ground)
        torch.cuda.synchronize()
        sol.clear_actuators()
        plain = ops.drive(b, ROLL_T, "rule", "ideal", ops.ground)
        torch.cuda.synchronize()
        flag, up = _np(slip["flag"]), _np(slip["contact_log"]) == 0
        cl = ((flag & 2) != 0) & (flag != 0xff)
        assert not (cl & ~up).any() and (cl & up)[cls == 2].sum() > 0 and (((flag & 32) != 0) & ~up).sum() > 0
        for r in np.nonzero(cls == 0)[0]:                                       # a flat Lite3 row: no table
            _same_robot("ideal drive on slippery ground", slip, plain, r, ALL_LOGS)
        q, qp = _np(slip["q"]), _np(plain["q"])
        assert not np.array_equal(q[cls == 2][up[cls == 2]], qp[cls == 2][up[cls == 2]], equal_nan=True)
    finally:
        sol.clear_actuators()


# ------------------------------------------------------------------------------------- 4. models, actuators and ground in one call
DRIVE_KW = dict(land="actual", drive="limited")


def _three(sol, pb, pr, T, models, act, ground):
    """rollout_drive (limited, land = actual) with the three tables set; numpy logs and state as mr._run returns them."""
    sol.set_models(models)
    sol.set_actuators(act)
    return mr._run(sol, "drive", pb, pr, T, ground=ground, **DRIVE_KW)


def _combined():
    """The combined run, once: (engine, case, tables, result)."""
    if "combined" not in _CACHE:
        pb, pr, rows, T = C.legs_case()
        act, ground, acls = ac.combined_tables()
        sol = mr._engine()
        try:
            out = _three(sol, pb, pr, T, rows, act, ground)
        finally:
            sol.clear_actuators()
            sol.clear_models()
        _CACHE["combined"] = (sol, (pb, pr, rows, T), (act, ground, acls), out)
    return _CACHE["combined"]


def _permuted(d, perm):
    return {k: (v[perm] if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _tiled(d, reps):
    return {k: (np.tile(v, (reps,) + (1,) * (v.ndim - 1)) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


@pytest.mark.gpu
def test_three_tables_in_one_call_row_by_row():
    sol, (pb, pr, rows, T), (act, ground, acls), out = _combined()
    B = C.LEGS_B
    keys = mr.KEYS["drive"]
    try:
        for c in range(4):                                                      # the model table uniform at class c, the others as they are
            ref = _three(sol, pb, pr, T, np.tile(rows[c], (B, 1)), act, ground)
            for b in np.nonzero(np.arange(B) % 4 == c)[0]:
                _same_robot(f"uniform model class {c}", out, ref, b, keys)
            assert not np.array_equal(ref["forces"][(c + 1) % 4], out["forces"][(c + 1) % 4])
        for c in range(4):                                                      # the actuator table uniform at class c
            ref = _three(sol, pb, pr, T, rows, ac.rows_of((ac.CLASSES[c],), B), ground)
            for b in np.nonzero(acls == c)[0]:
                _same_robot(f"uniform actuator class {c}", out, ref, b, keys)
        assert any(not np.array_equal(ref["q"][b], out["q"][b], equal_nan=True) for b in np.nonzero(acls != 3)[0])   # (ref: the weak curve)
        for g, mine in ((dc.GROUND_MU, np.arange(B) % 2 == 0), (1e3, np.arange(B) % 2 == 1)):
            ref = _three(sol, pb, pr, T, rows, act, np.full(B, g))
            for b in np.nonzero(mine)[0]:
                _same_robot(f"uniform ground {g}", out, ref, b, keys)
            assert any(not np.array_equal(ref["forces"][b], out["forces"][b]) for b in np.nonzero(~mine)[0])
    finally:
        sol.clear_actuators()
        sol.clear_models()
    fl, st = out["flag"], out["contact_log"] != 0
    live = fl != 0xff
    cl = ((fl & 2) != 0) & live
    print(f"three tables: solved {out['solved'].tolist()}, lowest CoM {out['actual'][:, :, 5].min():.3f} m, swing rows clamped on "
          f"{int((cl & ~st).any(axis=(1, 2)).sum())} robots, stance rows on {int((cl & st).any(axis=(1, 2)).sum())}")
    assert np.all(out["solved"] == T) and live.all() and (cl & ~st).any() and (cl & st).any()
    assert np.array_equal((((fl & 32) != 0) & st).any(axis=(1, 2)), np.arange(B) % 2 == 0)


@pytest.mark.gpu
def test_three_tables_in_one_call_under_permutations():
    sol, (pb, pr, rows, T), (act, ground, _), out = _combined()
    B = C.LEGS_B
    keys = mr.KEYS["drive"]
    try:
        for name, perm in (("reversal", np.arange(B)[::-1].copy()), ("shuffle", np.random.default_rng(5).permutation(B))):
            got = _three(sol, _permuted(pb, perm), _permuted(pr, perm), T, rows[perm], act[perm], ground[perm])
            for k in keys:
                assert np.array_equal(got[k], out[k][perm], equal_nan=True), (name, k)
    finally:
        sol.clear_actuators()
        sol.clear_models()
    # the queued launch: the case tiled 160 times, resident workgroups take several robots each
    reps, T2 = 160, 2
    n = B * reps
    big = mr._engine(listed_max=-1)
    bp, br = _tiled(pb, reps), _tiled(pr, reps)
    tabs = [np.tile(t, (reps,) + (1,) * (t.ndim - 1)) for t in (rows, act, ground)]
    try:
        base = _three(big, bp, br, T2, *tabs)
        for k in keys:                                                          # every copy of the case is the case
            assert np.array_equal(base[k], np.tile(base[k][:B], (reps,) + (1,) * (base[k].ndim - 1)), equal_nan=True), k
        assert np.all(base["solved"] == T2)
        for name, perm in (("reversal", np.arange(n)[::-1].copy()), ("shuffle", np.random.default_rng(6).permutation(n))):
            got = _three(big, _permuted(bp, perm), _permuted(br, perm), T2, *[t[perm] for t in tabs])
            for k in keys:
                assert np.array_equal(got[k], base[k][perm], equal_nan=True), (name, n, k)
    finally:
        big.clear_actuators()
        big.clear_models()


@pytest.mark.gpu
def test_three_tables_in_one_call_replay():
    import torch
    sol, (pb, pr, rows, T), (act, ground, _), out = _combined()
    B = C.LEGS_B
    n = B * T
    try:                                                                        # the rule on the logged rows, actuator table and ground tiled
        sol.set_actuators(actuators.tile(act, T))
        rep = sol.stance_drive(_t(out["actual"].reshape(n, 12), sol.tdtype), _t(out["cmd"].reshape(n, 12), sol.tdtype),
                               _t(out["feet_log"].reshape(n, 4, 3), sol.tdtype), _t(out["contact_log"].reshape(n, 4), torch.uint8),
                               _t(np.repeat(ground, T), sol.tdtype))
        torch.cuda.synchronize()
    finally:
        sol.clear_actuators()
    stance = out["contact_log"].reshape(n, 4) != 0
    assert np.array_equal(rep["f"].cpu().numpy(), out["forces"].reshape(n, 12))
    assert np.array_equal(rep["tau"].cpu().numpy()[stance], out["tau"].reshape(n, 4, 3)[stance])
    assert np.array_equal(rep["flag"].cpu().numpy()[stance] & dc.BITS, out["flag"].reshape(n, 4)[stance] & dc.BITS)
    assert (out["cmd"] != out["forces"]).any()
    # the solves, with the model table tiled: bitwise against cmd on the device, and against the checker
    mr._replay("rollout_drive with three tables, commanded forces", out, pb, rows, T, cmd="cmd")


# ------------------------------------------------------------------------------------ 5. an invalid row inside a roll-out
class _LoopOps(sd._Ops):
    """sd._Ops on drive_cases.loop_batch() (8 robots, nobody pushed, the configuration's body)."""

    def __init__(self, io):
        import torch
        self.io, self.B = io, dc.LOOP_B
        self.pb, self.rows = ac.loop_pb(io), None
        self.sol = mpcqp.MPCBatch(N=10, delta=DELTA, io_dtype=io, precision="mixed")
        dt, pb = self.sol.tdtype, self.pb
        self.const = {"gait": _t(pb["gait"], torch.int32), "stand": _t(pb["stand"], dt), "gain": _t(pb["gain"], dt), "mu": _t(pb["mu"], dt),
                      "step_height": _t(np.full(self.B, STEP_HEIGHT), dt)}

    def _kw(self):
        return {}

    def run(self, st, mode, T=dc.LOOP_T):
        _, drive, land = ac.LOOP_MODES[mode]
        return self.legs(st, T, land) if drive is None else self.drive(st, T, land, drive, None)


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("mode", range(len(ac.LOOP_MODES)), ids=[m[0] for m in ac.LOOP_MODES])
def test_an_invalid_row_inside_a_rollout(oracle_lib, mode, io):
    import torch
    if ("loop", io) not in _CACHE:
        _CACHE[("loop", io)] = _LoopOps(io)
    ops = _CACHE[("loop", io)]
    sol = ops.sol
    name, drive, land = ac.LOOP_MODES[mode]
    v, T = ac.INVALID_IN_LOOP, dc.LOOP_T
    logs_of = sd.ALL_LOGS + (("cmd",) if drive is not None else ())
    try:
        sol.set_actuators(ac.loop_rows(True))
        sb = ops.state()
        bad = ops.run(sb, mode)
        sol.set_actuators(ac.loop_rows(False))
        sg = ops.state()
        good = ops.run(sg, mode)
        torch.cuda.synchronize()
    finally:
        sol.clear_actuators()
    # nobody else changes
    for b in range(dc.LOOP_B):
        if b != v:
            _same_robot(f"{name}: state next to an invalid row", sb, sg, b, STATE)
            _same_robot(f"{name}: logs next to an invalid row", bad, good, b, logs_of)
    assert int(good["solved"].min()) == T and not bool((good["flag"] == 0xff).any())
    B6 = {k: _np(bad[k][v]) for k in logs_of}
    G6 = {k: _np(good[k][v]) for k in logs_of}
    up, landing = ac.swing_and_landing_rows(G6["contact_log"])
    ff = B6["flag"] == 0xff
    for k in LEG_NAN_LOGS:                                                      # a row is NaN in all of a leg log's entries, or in none
        nan = np.isnan(B6[k]).reshape(T, 4, -1)
        assert np.array_equal(nan.all(axis=-1), ff) and np.array_equal(nan.any(axis=-1), ff), (name, k)
    first = ac.first_nonfinite_tick(B6["actual"])
    print(f"invalid row, {name} {io}: {int(ff.sum())} rows 0xff of {int(up.sum())} swing and {int(landing.sum())} landing rows, actual non-finite "
          f"from tick {first}, solved {int(B6['solved'])}")
    if land == "rule":
        for k in ("x", "ref", "feet", "tick"):
            assert _eq(sb[k][v], sg[k][v]), (name, k)
        for k in ("actual", "desired", "forces", "feet_log", "contact_log", "swing", "solved"):
            assert np.array_equal(B6[k], G6[k], equal_nan=True), (name, k)
        assert np.array_equal(ff, up | landing) and up.sum() >= 20 and landing.sum() >= 5
        assert np.array_equal(np.isnan(B6["miss"]), G6["miss"] != 0.0) and np.isnan(B6["miss"]).sum() >= 5
        for k in LEG_NAN_LOGS + ("flag",):
            assert np.array_equal(B6[k][~ff], G6[k][~ff], equal_nan=True), (name, k)
    elif drive == "limited":
        assert ff.all() and first == 1 and int(B6["solved"]) == 1 and np.isfinite(B6["cmd"][0]).all()
        assert not np.isfinite(B6["actual"][1:]).all(axis=-1).any()
    else:
        Th = ac.LOOP_HOST_T
        host = {k: h[0] for k, h in ac.loop_host(mode, True, Th, io).items()}
        hfirst = ac.first_nonfinite_tick(host["actual"])
        assert hfirst < Th - 1 and first == hfirst and int(B6["solved"]) == int(host["solved"])
        assert np.array_equal(ff[:Th], host["flag"] == 0xff)
        for k in LEG_NAN_LOGS + ("miss", "actual", "feet_log"):
            assert np.array_equal(np.isnan(B6[k][:Th]), np.isnan(host[k])), (name, k)
        assert ff[first:].all() and not np.isfinite(B6["actual"][first:]).all(axis=-1).any()      # (the host's full loop: the host test)
        assert np.array_equal(B6["contact_log"], G6["contact_log"])


# ------------------------------------------------------------------------------------------------------------- 6. table lifetime
def _alone(ops, table, T, land="actual"):
    """The reference of a lifetime case: one table, one limited roll-out, synchronised and cleared."""
    import torch
    ops.sol.set_actuators(table)
    st = ops.state()
    out = ops.drive(st, T, land, "limited", ops.ground)
    torch.cuda.synchronize()
    ops.sol.clear_actuators()
    return st, out


def _equal_run(what, st, out, rst, rout):
    for k in STATE:
        assert _eq(st[k], rst[k]), (what, k)
    for k in ALL_LOGS:
        assert _eq(out[k], rout[k]), (what, k)


@pytest.mark.gpu
def test_table_lifetime_on_one_stream():
    import torch
    io, T = "f32", ROLL_T
    ref16, ref8 = _ops(io), _ops(io, 8)
    A, Bt = ac.rollout_rows(), np.roll(ac.rollout_rows(), 1, axis=0)
    alone = {"A": _alone(ref16, A, T), "B": _alone(ref16, Bt, T), "A8": _alone(ref8, A[:8], T), "none": _alone(ref16, actuators.actuator_rows(ROLL_B), T)}
    assert not _eq(alone["A"][1]["q"], alone["B"][1]["q"]) and not _eq(alone["A"][1]["q"], alone["none"][1]["q"])
    assert not _eq(alone["A8"][1]["q"], alone["B"][1]["q"][:8])
    assert int(alone["A"][1]["solved"].min()) > 0
    dev = {k: _t(v, torch.float64) for k, v in (("A", A), ("B", Bt), ("A8", A[:8]))}

    def fresh():
        """Operands for 16 and for 8 robots on ONE new engine."""
        o16, o8 = sd._Ops(io), sd._Ops(io, 8)
        o8.sol = o16.sol
        return o16, o8

    # a second table on the same stream, nothing in between
    o16, o8 = fresh()
    try:
        s1, s2 = o16.state(), o16.state()
        torch.cuda.synchronize()
        o16.sol.set_actuators(dev["A"])
        r1 = o16.drive(s1, T, "actual", "limited", o16.ground)
        o16.sol.set_actuators(dev["B"])
        r2 = o16.drive(s2, T, "actual", "limited", o16.ground)
        torch.cuda.synchronize()
        _equal_run("first table", s1, r1, *alone["A"])
        _equal_run("second table", s2, r2, *alone["B"])
        # a smaller table after a larger one, and the larger one again (the engine above has used 16 rows)
        s1, s2, s3 = o16.state(), o8.state(), o16.state()
        torch.cuda.synchronize()
        o16.sol.set_actuators(dev["B"])
        r1 = o16.drive(s1, T, "actual", "limited", o16.ground)
        o16.sol.set_actuators(dev["A8"])
        r2 = o8.drive(s2, T, "actual", "limited", o8.ground)
        o16.sol.set_actuators(dev["A"])
        r3 = o16.drive(s3, T, "actual", "limited", o16.ground)
        torch.cuda.synchronize()
        _equal_run("16 rows", s1, r1, *alone["B"])
        _equal_run("8 rows after 16", s2, r2, *alone["A8"])
        _equal_run("16 rows again", s3, r3, *alone["A"])
    finally:
        o16.sol.clear_actuators()
    # growth after use: 8 rows set and used, then 16 rows -- larger than any before -- right behind it
    o16, o8 = fresh()
    try:
        s1, s2 = o8.state(), o16.state()
        torch.cuda.synchronize()
        o16.sol.set_actuators(dev["A8"])
        r1 = o8.drive(s1, T, "actual", "limited", o8.ground)
        o16.sol.set_actuators(dev["B"])
        r2 = o16.drive(s2, T, "actual", "limited", o16.ground)
        torch.cuda.synchronize()
        _equal_run("8 rows first", s1, r1, *alone["A8"])
        _equal_run("16 rows after growth", s2, r2, *alone["B"])
    finally:
        o16.sol.clear_actuators()
