"""The slip rule and its roll-out with per-robot model rows, actuator rows, ground rows, foot masses and a start slip state
(include/mpcqp_slip.h, mpcqp_stance_slip / mpcqp_rollout_slip); the cases are in tests/slip_rows_cases.py and their conditions are held
on the CPU checker by tests/test_slip_rows_host.py.

  a. stance_slip with a table and moving feet against lite3_model.stance_slip_host on the draw (33 robots, one actuator row each, an
     invalid one on robot 13, a third of the stance feet moving), both I/O dtypes; the device's own answer depends on s0.
  b. The combined roll-out row by row: model class, actuator class, ground, foot mass and start slip state made uniform in turn.
  c. Permutations of the robots at B = 16, and the case tiled 160 times on the queued launch (B = 2560, T = 2): the finish kernel and
     the rule's in-loop launch over many blocks.
  d. Replay of the combined run: the solves through solve_batch_phase and the tight checker, the rule through stance_slip with the
     tables tiled, the plant through plant_step, the slip-state chain, the foot-move identity, and stance_slip_host row by row.
  e. substeps = 4: the rule's n is the roll-out's.
  f. drive = ideal: rollout_drive's on ground 1e3; on the low-friction ground no stance clamp, and stance_slip_host(drive = ideal) row by
     row.  The device's stance_slip is always limited, so the ideal rule has no device replay: its rows are held against the host only.
  g. A slice of the robots with its slices of every table; a NaN mass in a model row, an invalid actuator row, a NaN slip entry on a
     swing leg.
  h. fp32 I/O: the rule replay and the host comparison of (d), the foot-move identity with the float32 cast.

No tolerance is new: comparisons are bit for bit, or in the bands of tests/test_gpu_slip.py times the growth recorded in
tests/golden/slip_rows_growth.npz (measured on the host), or (the replayed solves) at the 1e-4 band of tests/batch_checks.py.  Legs
within legsim_cases.FLAG_MARGIN of a deciding threshold are left out of a host comparison; that they are at most 2 % of the stance legs is
asserted on the device's own rows.  No closed-loop comparison against the host roll-out: stick and slide decisions make the slipping loop
discontinuous in its inputs; the row-by-row replays carry the comparison."""
import numpy as np
import pytest

import actuator_cases as ac
import drive_cases as dc
import models_rollout_cases as C
import mpcqp
import slip_cases as sc
import slip_rows_cases as rc
import test_gpu_models_rollouts as mr
import test_gpu_stance_drive as sd
from legsim_cases import DELTA
from mpcqp import actuators, gaits

pytestmark = pytest.mark.gpu

_t, _np = sd._t, sd._np
_CACHE = {}
KEYS = mr.KEYS["drive"] + ("slip", "slip_log", "disp")
PER_ROBOT = ("rows", "act", "acls", "ground", "foot_mass", "slip")


def _f64(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda().contiguous()


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _as_io(K, io):
    """The case as the I/O dtype holds its ground and foot masses (the tables and the slip state are fp64 whatever the dtype)."""
    return K if io == "f64" else dict(K, ground=_r32(K["ground"]), foot_mass=_r32(K["foot_mass"]))


def _run(sol, K, T=None, land="actual", drive="limited", **kw):
    """rollout_slip of a case on the device, the tables as the engine has them; numpy logs and the advanced state, "slip" included."""
    import torch
    d = mr._dev(sol, K["pb"])
    slip = _f64(K["slip"])
    out = sol.rollout_slip(*[d[k] for k in C.LEGS_ARGS], K["T"] if T is None else T, d["step_height"], _t(K["ground"], sol.tdtype),
                           _t(K["foot_mass"], sol.tdtype), slip, land, drive, **mr._plant(sol, K["pr"]), **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update({k: d[k].cpu().numpy() for k in ("x", "ref", "feet", "legs", "tick")})
    res["slip"] = slip.cpu().numpy()
    return res


def _five(sol, K, T=None, **kw):
    """rollout_slip with the model and the actuator table of the case set."""
    sol.set_models(K["rows"])
    sol.set_actuators(K["act"])
    return _run(sol, K, T, **kw)


def _clear(sol):
    sol.clear_actuators()
    sol.clear_models()


def _combined(io="f64", **kw):
    """The combined run, once per I/O dtype and variant: (engine, case, result)."""
    key = (io,) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        K = rc.combined_case()
        sol = mr._engine(io)
        try:
            out = _five(sol, K, **kw)
        finally:
            _clear(sol)
        _CACHE[key] = (sol, K, out)
    return _CACHE[key]


def _same_robot(what, got, ref, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(got[k][b], ref[k][b], equal_nan=True), (what, b, k)


def _permuted(K, perm):
    cut = lambda d: {k: (v[perm] if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    return dict(K, pb=cut(K["pb"]), pr=cut(K["pr"]), **{k: K[k][perm] for k in PER_ROBOT})


def _tiled(K, reps):
    rep = lambda v: np.tile(v, (reps,) + (1,) * (v.ndim - 1))
    cut = lambda d: {k: (rep(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    return dict(K, pb=cut(K["pb"]), pr=cut(K["pr"]), **{k: rep(K[k]) for k in PER_ROBOT})


def _rule(sol, K, out, substeps=10):
    """stance_slip on the logged rows of a roll-out of the case, the actuator table, ground, foot mass and slip_log tiled; numpy."""
    import torch
    x, f, feet, contact, ground, me, s0, act = rc.replay_operands(out, K)
    dt = sol.tdtype
    try:
        sol.set_actuators(act)
        rep = sol.stance_slip(_t(x, dt), _t(f, dt), _t(feet, dt), _t(contact, torch.uint8), _t(ground, dt), _t(me, dt), _f64(s0), substeps=substeps)
        torch.cuda.synchronize()
    finally:
        sol.clear_actuators()
    return {k: v.cpu().numpy() for k, v in rep.items()}


def _rows(a):
    return a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])


def _print_counts(tag, out, K):
    print(f"{tag}: solved {out['solved'].tolist()}, lowest CoM {np.nanmin(out['actual'][:, :, 5]):.3f} m, {rc.counts(out, K)}, largest |disp| "
          f"{np.nanmax(np.abs(out['disp'])):.4f} m")


def _rule_replay_and_host(io):
    """(d)'s rule replay and host comparison on the combined run of one I/O dtype.  Returns (case, run, replay)."""
    sol, K, out = _combined(io)
    K = _as_io(K, io)
    B, T = C.LEGS_B, K["T"]
    npdt = np.float64 if io == "f64" else np.float32
    _print_counts(f"combined slip run {io}", out, K)
    n = rc.counts(out, K)
    assert np.all(out["solved"] == T) and n["dead"] == 0 and n["clamped stance"] > 0 and n["clamped swing"] > 0 and n["sliding"] > 0
    assert n["sliding low-friction robots"] >= 6
    rep = _rule(sol, K, out)
    s = _rows(out["contact_log"]) != 0
    assert np.array_equal(rep["f"], _rows(out["forces"])) and np.array_equal(rep["disp"], _rows(out["disp"]))
    assert np.array_equal(rep["tau"][s], _rows(out["tau"])[s])
    # (bit 16 has a second source on a stance row: the legs step sets it where the held foot is out of reach, which a foot that slides
    #  without a reach stop can be; the rule's own bit 16 needs a clamped leg)
    dt = sol.tdtype
    far = _rows(sol.joint_log(_t(out["actual"], dt), _t(out["cmd"], dt), _t(out["feet_log"], dt))["reach"].cpu().numpy() == 0)
    flag = _rows(out["flag"])
    print(f"combined slip run {io}: {int((far & s).sum())} stance leg-rows out of reach")
    assert np.array_equal((rep["flag"][s] & sc.BITS) | (far[s] * 16).astype(np.uint8), flag[s] & sc.BITS)
    assert np.array_equal(rep["flag"][s & ~far] & sc.BITS, flag[s & ~far] & sc.BITS) and not rep["flag"][~s].any()
    # the slip state: the next row's s0 is this row's s_end where the leg did not touch down, 0 at a touchdown; a start entry on a swing
    # leg is logged as given and is 0 from the next row on until the leg has landed and slid
    gait, tick0 = K["pb"]["gait"], K["pb"]["tick"]
    end, slog = rep["slip"].reshape(B, T, 4, 2), out["slip_log"]
    on_swing = rc.start_on_swing(K, out["contact_log"])
    assert np.array_equal(slog[:, 0], K["slip"]) and on_swing.sum() >= 3 and not end[~(out["contact_log"] != 0)].any()
    for t in range(1, T + 1):
        td = gaits.touchdown_mask(gait, tick0 + t)
        nxt = slog[:, t] if t < T else out["slip"]
        assert np.array_equal(nxt[~td], end[:, t - 1][~td]) and not nxt[td].any(), t
    up = out["contact_log"] == 0
    for b, l in zip(*np.nonzero(on_swing)):
        first_down = int(np.argmax(~up[b, :, l])) if (~up[b, :, l]).any() else T
        assert first_down >= 1 and not slog[b, 1:first_down + 1, l].any(), (b, l)
    # the foot-move identity, on the logs in their own dtype
    assert sc.foot_move_holds(out["feet_log"], out["contact_log"], out["disp"], gait, tick0, cast=lambda a: a.astype(npdt))
    assert np.abs(out["disp"]).max() > 1e-4
    # row by row on the host, the margin share on the device's own rows
    o64 = {k: (v.astype(np.float64) if v.dtype.kind == "f" else v) for k, v in out.items()}
    host = rc.replay_host(o64, K)
    dev = {"f": _rows(o64["forces"]).reshape(-1, 4, 3), "tau": np.where(s[..., None], _rows(o64["tau"]), 0.0),
           "flag": np.where(s, rep["flag"] & (sc.BITS | 4), 0).astype(np.uint8), "slip": rep["slip"], "disp": _rows(o64["disp"])}
    worst = rc.compare_with_host(f"combined slip run, rows", io, dev, host, _rows(o64["cmd"]).reshape(-1, 4, 3), np.repeat(K["foot_mass"], T), s,
                                 rc.band_scale(), sd._error)
    x, f, feet, contact, ground, me, s0, act = rc.replay_operands(o64, K)
    moving = s0.any(axis=-1) & s
    sens = rc.s0_sensitive(host["tau_cmd"], host["rate"], rc.rest_rate(x, f, feet, contact, ground, act), act, moving)
    print(f"combined slip run {io}: {int(moving.sum())} moving stance leg-rows, {int(sens.sum())} s0-sensitive on the device's own rows; worst "
          f"error over band {max(worst.values()):.3e}")
    return K, out, rep


# ------------------------------------------------------------------------------------- a. stance_slip with a table and moving feet
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_stance_slip_with_a_table_and_moving_feet_against_the_host(io):
    import torch
    npdt = np.float64 if io == "f64" else np.float32
    c = rc.as_io(rc.rows_draw(), npdt)
    host, host0 = rc.slip(c), rc.slip(dict(c, slip=np.zeros_like(c["slip"])))
    b = ac.INVALID_ROBOT
    mended = c["rows"].copy()
    mended[b] = actuators.actuator_rows(1)[0]
    sol = mpcqp.MPCBatch(io_dtype=io)
    dt = sol.tdtype
    x, f, feet, ground, me = (_t(c[k], dt) for k in ("x", "f", "feet", "ground", "foot_mass"))
    contact, slip = _t(c["contact"], torch.uint8), _f64(c["slip"])
    try:
        sol.set_actuators(c["rows"])
        out = sol.stance_slip(x, f, feet, contact, ground, me, slip)
        out0 = sol.stance_slip(x, f, feet, contact, ground, me, torch.zeros_like(slip))
        sol.set_actuators(mended)
        ref = sol.stance_slip(x, f, feet, contact, ground, me, slip)
        torch.cuda.synchronize()
    finally:
        sol.clear_actuators()
    grab = lambda o: {"f": _np(o["f"]).reshape(-1, 4, 3), "tau": _np(o["tau"]), "flag": _np(o["flag"]), "slip": _np(o["slip"]), "disp": _np(o["disp"])}
    dev, dev0, good = grab(out), grab(out0), grab(ref)
    st = c["contact"] != 0
    f_in = _np(f).reshape(-1, 4, 3)
    worst = rc.compare_with_host("stance_slip with a table", io, dev, host, f_in, c["foot_mass"], st, rc.band_scale(), sd._error)
    print(f"stance_slip with a table {io}: worst error over band {max(worst.values()):.3e}")
    for k in ("tau", "flag", "slip", "disp"):
        assert not dev[k][~st].any(), k
    # robot 13: every stance leg poisoned, its swing legs' forces kept; with its row mended nobody else changes
    assert st[b].any() and (~st[b]).any() and np.all(dev["flag"][b][st[b]] == 0xff) and np.array_equal(dev["f"][b][~st[b]], f_in[b][~st[b]])
    for k in ("f", "tau", "slip", "disp"):
        assert np.isnan(dev[k][b][st[b]]).all(), k
    others = np.arange(c["x"].shape[0]) != b
    for k in dev:
        assert np.array_equal(dev[k][others], good[k][others], equal_nan=True), k
    assert not np.any(dev["flag"][others] == 0xff) and not np.any(good["flag"] == 0xff)
    # the device's own answer depends on s0: slip = 0 gives other torques on the legs where the host's differ, the same bits at rest
    moving = c["slip"].any(axis=-1) & st
    other = rc.tau_moves_without_s0(host, host0, moving)
    rest = rc.rest_rate(c["x"], c["f"], c["feet"], c["contact"], c["ground"], c["rows"])
    sens = rc.s0_sensitive(host["tau_cmd"], host["rate"], rest, c["rows"], moving)
    with np.errstate(invalid="ignore"):
        differ = (dev["tau"] != dev0["tau"]).any(axis=-1) & (dev["flag"] != 0xff)
        big = other & (np.abs(host["tau"] - host0["tau"]).max(axis=-1) > rc.S0_TORQUE)
    print(f"stance_slip with a table {io}: slip = 0 changes the torque of {int((differ & moving).sum())} moving legs on the device, of "
          f"{int(other.sum())} on the host ({int(big.sum())} by more than {rc.S0_TORQUE} N m, {int((other & sens).sum())} through the envelope)")
    assert (differ & moving).sum() >= other.sum() >= rc.S0_LEGS and differ[big].all() and (other & sens).sum() >= rc.S0_LEGS
    at_rest = ~c["slip"].any(axis=-1)
    for k in dev:
        assert np.array_equal(dev[k][at_rest], dev0[k][at_rest], equal_nan=True), k
    # ... and through the envelope: on the s0-sensitive legs the device is the rule's answer, not the one with s0 left out of the rate
    a = [c[k] for k in ("x", "f", "feet", "contact", "ground", "foot_mass", "slip", "rows")]
    mutant = rc.rule_with_rate(*a, rest, delta=DELTA)
    with np.errstate(invalid="ignore"):
        apart = sens & ~dc.near_threshold(host) & (np.abs(mutant["tau"] - host["tau"]).max(axis=-1) > rc.S0_TORQUE)
        closer = np.abs(dev["tau"] - host["tau"]).max(axis=-1) < 0.5 * np.abs(dev["tau"] - mutant["tau"]).max(axis=-1)
    assert apart.sum() >= rc.S0_LEGS and closer[apart].all()


# ----------------------------------------------------------------------------------------------- b. the combined roll-out, row by row
def test_five_per_robot_inputs_in_one_call_row_by_row():
    """Each input uniform in turn, the other four as they are: the robots whose own value that was are the combined run bit for bit,
    state and every log, and some other robot is not.  The model and actuator tables and the ground have four, four and two values; the
    foot mass and the start slip state have sixteen, of which those of robots 0, 5, 10 and 15 are taken (both grounds, every class)."""
    sol, K, out = _combined()
    B, T = C.LEGS_B, K["T"]
    every = np.arange(B)
    picks = (0, 5, 10, 15)                                                      # both grounds, every model and actuator class
    uniform = lambda v: np.tile(v[None], (B,) + (1,) * np.ndim(v))
    cases = [(f"model class {c}", {"rows": uniform(K["rows"][c])}, every % 4 == c) for c in range(4)]
    cases += [(f"actuator class {c}", {"act": ac.rows_of((ac.CLASSES[c],), B)}, K["acls"] == c) for c in range(4)]
    cases += [(f"ground {g}", {"ground": np.full(B, g)}, K["ground"] == g) for g in (rc.LOW_MU, 1e3)]
    cases += [(f"foot mass of robot {b}", {"foot_mass": np.full(B, K["foot_mass"][b])}, every == b) for b in picks]
    cases += [(f"start slip state of robot {b}", {"slip": uniform(K["slip"][b])}, every == b) for b in picks]
    try:
        for what, over, mine in cases:
            ref = _five(sol, dict(K, **over))
            assert mine.any() and not mine.all()
            for b in np.nonzero(mine)[0]:
                _same_robot(f"uniform {what}", out, ref, b)
            moved = [b for b in np.nonzero(~mine)[0] if not np.array_equal(ref["forces"][b], out["forces"][b], equal_nan=True)
                     or not np.array_equal(ref["disp"][b], out["disp"][b], equal_nan=True)]
            print(f"uniform {what}: {len(moved)} of {int((~mine).sum())} other robots differ")
            assert moved, what
    finally:
        _clear(sol)
    _print_counts("combined slip run f64", out, K)
    n = rc.counts(out, K)
    assert np.all(out["solved"] == T) and n["dead"] == 0 and n["clamped stance"] > 0 and n["clamped swing"] > 0
    assert n["sliding low-friction robots"] >= 6 and np.array_equal(out["slip_log"][:, 0], K["slip"])


# ----------------------------------------------------------------------------------------------------------------- c. permutations
def test_five_per_robot_inputs_under_permutations():
    sol, K, out = _combined()
    B = C.LEGS_B
    try:
        for name, perm in (("reversal", np.arange(B)[::-1].copy()), ("shuffle", np.random.default_rng(5).permutation(B))):
            got = _five(sol, _permuted(K, perm))
            for k in KEYS:
                assert np.array_equal(got[k], out[k][perm], equal_nan=True), (name, k)
    finally:
        _clear(sol)
    # the queued launch: the case tiled 160 times; the rule's in-loop launch and the finish kernel run over 40 blocks
    reps, T2 = 160, 2
    n = B * reps
    big = mr._engine(listed_max=-1)
    KT = _tiled(K, reps)
    try:
        base = _five(big, KT, T2)
        for k in KEYS:                                                          # every copy of the case is the case
            assert np.array_equal(base[k], np.tile(base[k][:B], (reps,) + (1,) * (base[k].ndim - 1)), equal_nan=True), k
        rep = _rule(big, KT, base)                                              # ... and its rows replay through the rule, 80 blocks
        assert np.array_equal(rep["f"], _rows(base["forces"])) and np.array_equal(rep["disp"], _rows(base["disp"]))
        assert np.all(base["solved"] == T2) and base["disp"].any() and (base["slip"] != KT["slip"]).any()
        assert (((base["flag"] & 128) != 0) & (base["contact_log"] != 0)).any() and (4 * n + 255) // 256 == 40
        for name, perm in (("reversal", np.arange(n)[::-1].copy()), ("shuffle", np.random.default_rng(6).permutation(n))):
            got = _five(big, _permuted(KT, perm), T2)
            for k in KEYS:
                assert np.array_equal(got[k], base[k][perm], equal_nan=True), (name, n, k)
    finally:
        _clear(big)


# ------------------------------------------------------------------------------------------------------------------------ d. replay
def _plant_replay(sol, K, out, substeps=10):
    """plant_step on the logged rows with each robot's body and push: actual[t + 1], numpy [B (T - 1), 12]."""
    import torch
    B, T = C.LEGS_B, K["T"]
    dt = sol.tdtype
    pb, pr = K["pb"], K["pr"]
    g = np.repeat(pb["x"][:, 12:13], T - 1, axis=0)
    x0 = np.concatenate([_rows(out["actual"][:, :-1]), g], axis=1)
    wr = _rows(gaits.log_wrench(pr["push"], pr["push_ticks"], pb["tick"], T)[:, :-1])
    nxt = sol.plant_step(_t(x0, dt), _t(_rows(out["forces"][:, :-1]), dt), _t(_rows(out["feet_log"][:, :-1]), dt),
                         _t(_rows(out["contact_log"][:, :-1]), torch.uint8), _t(np.repeat(pr["body"], T - 1, axis=0), dt), _t(wr, dt), substeps=substeps)
    torch.cuda.synchronize()
    return nxt.cpu().numpy()[:, :12]


def test_five_per_robot_inputs_replay():
    K, out, rep = _rule_replay_and_host("f64")
    sol = _CACHE[("f64",)][0]
    # the solves, with the model table tiled: bitwise against cmd on the device, and against the tight checker
    mr._replay("rollout_slip with five per-robot inputs, commanded forces", out, K["pb"], K["rows"], K["T"], cmd="cmd")
    # the plant received the applied forces, with its feet fixed over the tick, each robot's body and push
    assert np.any(K["pr"]["push"] != 0) and len(np.unique(K["pr"]["body"], axis=0)) == 4
    assert np.array_equal(_plant_replay(sol, K, out), _rows(out["actual"][:, 1:]))
    assert (out["cmd"] != out["forces"]).any()


# ------------------------------------------------------------------------------------------------------- e. another substep count
def test_the_rules_substeps_are_the_rollouts():
    n = rc.SECOND_SUBSTEPS
    sol, K, out = _combined(substeps=n)
    _print_counts(f"combined slip run, substeps {n}", out, K)
    assert np.all(out["solved"] == K["T"]) and rc.counts(out, K)["sliding"] > 0
    own, other = _rule(sol, K, out, substeps=n), _rule(sol, K, out)
    assert np.array_equal(own["f"], _rows(out["forces"])) and np.array_equal(own["disp"], _rows(out["disp"]))
    assert not np.array_equal(other["f"], _rows(out["forces"])) and not np.array_equal(other["disp"], _rows(out["disp"]))
    assert np.array_equal(_plant_replay(sol, K, out, substeps=n), _rows(out["actual"][:, 1:]))
    assert not np.array_equal(_plant_replay(sol, K, out), _rows(out["actual"][:, 1:]))
    assert not np.array_equal(out["forces"], _combined()[2]["forces"])


# --------------------------------------------------------------------------------------------------------------- f. the ideal drive
def test_the_ideal_drive_with_the_tables():
    """(The device's stance_slip is always limited: the ideal rule's rows have no device replay and are held against the host.)"""
    sol, K, _ = _combined()
    B, T = C.LEGS_B, K["T"]
    grip = dict(K, ground=np.full(B, 1e3), slip=np.zeros((B, 4, 2)))
    try:
        got = _five(sol, grip, drive="ideal")
        ref = mr._run(sol, "drive", K["pb"], K["pr"], T, land="actual", drive="ideal", ground=grip["ground"])
        ice = _five(sol, K, drive="ideal")
    finally:
        _clear(sol)
    for k in mr.KEYS["drive"]:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert not got["slip_log"].any() and not got["disp"].any() and not got["slip"].any() and np.all(got["solved"] == T)
    # on the low-friction ground: no stance clamp, the ground and the slide alone change the forces
    _print_counts("ideal drive on the low-friction ground", ice, K)
    fl, st = ice["flag"], ice["contact_log"] != 0
    live = fl != 0xff
    assert np.all(ice["solved"] == T) and live.all()
    assert not (((fl & 2) != 0) & st).any() and (((fl & 32) != 0) & st).any() and (((fl & 128) != 0) & st).any()
    assert (((fl & 2) != 0) & ~st).any()                                        # (the swing legs still clamp)
    mr._replay("rollout_slip(ideal) on the low-friction ground, commanded forces", ice, K["pb"], K["rows"], T, cmd="cmd")
    host = rc.replay_host(ice, K, drive="ideal")
    s = _rows(st)
    near = dc.near_threshold(host)
    keep = s & ~near
    scale = rc.band_scale()
    print(f"ideal drive: {int(near.sum())} of {int(s.sum())} stance leg-rows within FLAG_MARGIN of a threshold")
    assert near.sum() <= dc.MARGIN_SHARE * s.sum()
    assert np.array_equal(_rows(fl)[keep] & (2 | 32 | 128), host["flag"][keep] & (2 | 32 | 128))
    f_dev, f_host, f_in = (_rows(a).reshape(-1, 4, 3) for a in (ice["forces"], host["f"].reshape(B, T, 12), ice["cmd"]))
    free = keep & ((host["flag"] & (32 | 128)) == 0)
    assert np.array_equal(f_dev[free], f_in[free]) and np.array_equal(f_dev[~s], f_in[~s])
    err, band = sd._error(f_dev[keep], f_host[keep], "f64")
    bd = sc.state_bands(np.float64, f_host, f_in, np.repeat(K["foot_mass"], T))[1]
    derr = float((np.abs(_rows(ice["disp"]) - host["disp"]) / (bd * scale)[..., None])[keep].max())
    print(f"ideal drive: applied forces err {err:.3e} band {band:.1e} x {scale:.2f} on {int(keep.sum())} leg-rows; disp worst error over band {derr:.3e}")
    assert err <= band * scale and derr <= 1.0


# ------------------------------------------------------------------------------------------------------ g. slices and invalid rows
def test_a_slice_of_robots_with_its_slices_of_every_table():
    sol, K, out = _combined()
    sub = np.arange(4, 12)
    try:
        part = _five(sol, _permuted(K, sub))
    finally:
        _clear(sol)
    for k in KEYS:
        assert np.array_equal(part[k], out[k][sub], equal_nan=True), k


def test_invalid_rows_and_a_nan_on_a_swing_leg_inside_a_slip_rollout():
    sol, K, out = _combined()
    B, T = C.LEGS_B, K["T"]
    up0 = out["contact_log"][:, 0] == 0
    # a swing leg of the first tick on a low-friction robot: NaN there, against 0 there
    sb, sl = [(b, l) for b, l in zip(*np.nonzero(up0)) if b % 2 == 0][0]
    victim, weak = 5, 9
    bad_rows, bad_act, bad_slip = K["rows"].copy(), K["act"].copy(), K["slip"].copy()
    bad_rows[victim, 0] = np.nan
    assert np.isfinite(K["act"][weak, 3:6]).all()
    bad_act[weak, 6:9] = 0.5 * bad_act[weak, 3:6]
    bad_slip[sb, sl] = [0.0, np.nan]
    zero_slip = bad_slip.copy()
    zero_slip[sb, sl] = 0.0
    try:
        zero = _five(sol, dict(K, slip=zero_slip))
        model = _five(sol, dict(K, rows=bad_rows))
        act = _five(sol, dict(K, act=bad_act))
        swing = _five(sol, dict(K, slip=bad_slip))
    finally:
        _clear(sol)
    # a NaN mass in a model row: that robot solves nothing and is commanded zero force; nobody else changes
    assert model["solved"][victim] == 0 and not np.any(model["cmd"][victim])
    for b in range(B):
        if b != victim:
            _same_robot("next to an invalid model row", model, out, b)
    # an invalid actuator row: its legs are poisoned from the first row, its state from the second; nobody else changes
    ff = act["flag"][weak] == 0xff
    first = ac.first_nonfinite_tick(act["actual"][weak])
    print(f"invalid actuator row in a slip roll-out: {int(ff.sum())} of {ff.size} rows 0xff, actual non-finite from tick {first}, solved {int(act['solved'][weak])}")
    assert ff.all() and first == 1 and int(act["solved"][weak]) == 1 and np.isfinite(act["cmd"][weak, 0]).all()
    assert not np.isfinite(act["actual"][weak, 1:]).all(axis=-1).any()
    for b in range(B):
        if b != weak:
            _same_robot("next to an invalid actuator row", act, out, b)
    # a NaN slip entry on a swing leg: logged as given, no leg poisoned, every force and state that of the run with 0 there
    assert np.isnan(swing["slip_log"][sb, 0, sl, 1]) and swing["slip_log"][sb, 0, sl, 0] == 0.0 and not swing["slip_log"][sb, 1, sl].any()
    assert not np.any(swing["flag"] == 0xff) and np.isfinite(swing["slip"]).all() and np.isfinite(swing["forces"]).all()
    mended = dict(swing, slip_log=swing["slip_log"].copy())
    mended["slip_log"][sb, 0, sl, 1] = 0.0
    for k in KEYS:
        assert np.array_equal(mended[k], zero[k], equal_nan=True), k
    assert (((zero["flag"][sb] & 128) != 0) & (zero["contact_log"][sb] != 0)).any() and np.all(zero["solved"] == T)


# ---------------------------------------------------------------------------------------------------------------- h. fp32 I/O
def test_the_rule_replay_and_the_host_comparison_in_fp32():
    K, out, rep = _rule_replay_and_host("f32")
    assert out["forces"].dtype == np.float32 and out["disp"].dtype == np.float32 and out["slip_log"].dtype == np.float64
    assert rep["slip"].dtype == np.float64 and (out["cmd"] != out["forces"]).any()
