"""Stance feet that slide, on the device (include/mpcqp_slip.h, mpcqp_stance_slip / mpcqp_rollout_slip).

  1. stance_slip against lite3_model.stance_slip_host on slip_cases.slip_draw(): drive_cases.clamp_draw() (33 robots, a partial block)
     with a third of the stance feet moving at up to 1 m/s and a foot mass per robot in [0.15, 0.6]; both I/O dtypes.
  2. rollout_slip at ground 1e3 is rollout_drive at ground 1e3 under torch.equal, state and every log, on legsim_cases.rollout_batch().
  3. ground 0.3 under the even robots with tau_max x 0.5: the logs replay through stance_slip and plant_step on the device bit for bit,
     the slip state and the feet follow the rule's outputs, and stance_slip_host agrees row by row within the bands of 1.
  4. Pieces, NULL logs, land = actual, an actuator table with rows that differ per robot, poison, determinism, argument errors, T = 0
     and B = 0.

Bands: f and tau as tests/test_gpu_stance_drive.py holds them (drive_cases.band: 1e-9 for fp64 I/O, 2 float32 spacings against the
host value rounded once for fp32 I/O); the slip state s to band_f delta / m_e and the displacement d to band_f delta^2 / m_e, the
rule's own gain from a force to a velocity and to a displacement, with band_f the band at the leg's largest force component,
commanded or applied (on a pull the applied force is 0 and the whole commanded force drives the foot); d, which
is of the I/O dtype, against the host value rounded once.  Legs within legsim_cases.FLAG_MARGIN of a deciding threshold are left out;
that they are at most 2 % of the stance legs is asserted here and, for the draw, on the CPU (tests/test_slip_host.py).
The foot-move identity is held in its exact form, feet_log[t + 1].xy == T(feet_log[t].xy + disp[t])."""
import numpy as np
import pytest

import drive_cases as dc
import mpcqp
import slip_cases as sc
import test_gpu_stance_drive as drv
from legsim_cases import DELTA, ROLL_B, ROLL_T
from mpcqp import actuators, gaits, lite3_model

_t, _np, _error = drv._t, drv._np, drv._error
STATE = drv.STATE + ("slip",)
DRIVE_LOGS = drv.ALL_LOGS + ("cmd",)
ALL_LOGS = DRIVE_LOGS + ("slip_log", "disp")
_CACHE = {}


def _f64(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda().contiguous()


def _same(a, b):
    return np.array_equal(_np(a), _np(b), equal_nan=True)


def _compare_with_host(tag, io, dev, host, f_in, foot_mass, stance):
    """Flags equal; f_out bit-equal to f where the rule left the leg alone; elsewhere f_out and tau within the band; s and d within
    theirs.  dev = {"f" [n,4,3], "tau" [n,4,3], "flag" [n,4], "slip" [n,4,2], "disp" [n,4,2]} as numpy.  Returns the worst
    error / band ratios."""
    npdt = np.float64 if io == "f64" else np.float32
    near = dc.near_threshold(host)
    print(f"{tag} {io}: {int(near.sum())} of {int(stance.sum())} stance legs within FLAG_MARGIN of a threshold")
    assert near.sum() <= dc.MARGIN_SHARE * stance.sum()
    keep = ~near
    assert np.array_equal(dev["flag"][keep], host["flag"][keep])
    hf = host["f"].reshape(-1, 4, 3)
    free = keep & ((host["flag"] & (2 | 32 | 128)) == 0)
    assert np.array_equal(dev["f"][free], f_in[free], equal_nan=True)
    rest = keep & ~free
    worst = {}
    for k, d, h in (("f_out", dev["f"], hf), ("tau", dev["tau"], host["tau"])):
        err, band = _error(d[rest], h[rest], io)
        print(f"{tag} {io} {k}: err {err:.3e} band {band:.1e} on {int(rest.sum())} legs (max |{k}| {np.nanmax(np.abs(h[rest])):.1f})")
        assert err <= band, (k, err)
        worst[k] = err / band
    err, band = _error(dev["tau"][free], host["tau"][free], io)
    assert err <= band
    bs, bd = sc.state_bands(npdt, hf, f_in, foot_mass)
    for k, d, h, b in (("s", dev["slip"], host["slip"], bs), ("d", dev["disp"], host["disp"].astype(npdt).astype(np.float64), bd)):
        nan = np.isnan(h)
        assert np.array_equal(nan, np.isnan(d)), k
        ratio = np.where(nan, 0.0, np.abs(d - h) / b[..., None])[keep]
        worst[k] = float(ratio.max())
        print(f"{tag} {io} {k}: worst |dev - host| / band {worst[k]:.3e} (largest |{k}| {np.nanmax(np.abs(h)):.3f}, smallest band {b[keep].min():.2e})")
        assert worst[k] <= 1.0, (k, worst[k])
    return worst


# ----------------------------------------------------------------------------------------------------- 1. stance_slip against the host
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_stance_slip_against_the_host(io):
    import torch
    npdt = np.float64 if io == "f64" else np.float32
    c = sc.as_io(sc.slip_draw(), npdt)
    host = sc.slip(c)
    sol = mpcqp.MPCBatch(io_dtype=io)
    dt = sol.tdtype
    x, f, feet, ground, me = (_t(c[k], dt) for k in ("x", "f", "feet", "ground", "foot_mass"))
    contact, slip = _t(c["contact"], torch.uint8), _f64(c["slip"])
    out = sol.stance_slip(x, f, feet, contact, ground, me, slip)
    torch.cuda.synchronize()
    st = c["contact"] != 0
    fl = host["flag"]
    assert ((fl & 2) != 0)[st].sum() >= 20 and ((fl & 32) != 0)[st].sum() >= 20 and ((fl & 128) != 0)[st].sum() >= 20
    assert (~st).sum() >= 10 and not np.any(fl == 0xff) and torch.equal(slip, _f64(c["slip"]))
    dev = {"f": _np(out["f"]).reshape(-1, 4, 3), "tau": _np(out["tau"]), "flag": _np(out["flag"]), "slip": _np(out["slip"]),
           "disp": _np(out["disp"])}
    assert out["slip"].dtype == torch.float64 and out["disp"].dtype == dt
    _compare_with_host("stance_slip", io, dev, host, _np(f).reshape(-1, 4, 3), c["foot_mass"], st)
    for k in ("tau", "flag", "slip", "disp"):
        assert not dev[k][~st].any(), k
    # a foot that stuck is at rest exactly
    stopped = c["slip"].any(axis=-1) & ~host["slip"].any(axis=-1) & ~dc.near_threshold(host)
    assert stopped.sum() >= 3 and not dev["slip"][stopped].any()
    # slip_out may be slip_in; optional outputs; another substep count is another answer
    s2 = slip.clone()
    fo = torch.empty_like(f)
    sol.engine.stance_slip_ptr(33, x.data_ptr(), f.data_ptr(), feet.data_ptr(), contact.data_ptr(), ground.data_ptr(), me.data_ptr(),
                               s2.data_ptr(), fo.data_ptr(), slip_out=s2.data_ptr())
    fine = sol.stance_slip(x, f, feet, contact, ground, me, slip, substeps=40, want=())
    torch.cuda.synchronize()
    assert torch.equal(s2, out["slip"]) and torch.equal(fo, out["f"])
    assert fine["tau"] is None and fine["flag"] is None and not torch.equal(fine["disp"], out["disp"])
    hf = sc.slip(c, substeps=40)
    bs40 = sc.state_bands(npdt, hf["f"].reshape(-1, 4, 3), c["f"].reshape(-1, 4, 3), c["foot_mass"])[0]
    assert np.all((np.abs(_np(fine["slip"]) - hf["slip"]) <= bs40[..., None])[~dc.near_threshold(hf)])
    # poison: a NaN foot_mass row, a negative ground row and a NaN slip entry; nobody else changes
    mb, gb, sb = me.clone(), ground.clone(), slip.clone()
    mb[3] = float("nan"); gb[5] = -0.5
    l9 = int(np.nonzero(c["contact"][9])[0][0])
    sb[9, l9, 0] = float("nan")
    bad = sol.stance_slip(x, f, feet, contact, gb, mb, sb)
    sol.stance_slip(x[:0], f[:0], feet[:0], contact[:0], ground[:0], me[:0], slip[:0])     # the empty batch
    torch.cuda.synchronize()
    for b in (3, 5):
        assert bool((bad["flag"][b] == 0xff).all()) and all(bool(torch.isnan(bad[k][b]).all()) for k in ("f", "tau", "slip", "disp"))
    assert int(bad["flag"][9, l9]) == 0xff and all(bool(torch.isnan(bad[k][9, l9]).all()) for k in ("tau", "slip", "disp"))
    assert bool(torch.isnan(bad["f"][9, 3 * l9:3 * l9 + 3]).all())
    others = torch.ones((33, 4), dtype=torch.bool, device="cuda")
    others[3] = False; others[5] = False; others[9, l9] = False
    for k in ("tau", "flag", "slip", "disp"):
        assert torch.equal(bad[k][others], out[k][others]), k
    assert torch.equal(bad["f"].reshape(33, 4, 3)[others], out["f"].reshape(33, 4, 3)[others])


# ------------------------------------------------------------------------------------------------------------- the roll-out's operands
class _Ops:
    """drv._Ops' operands with the slip rule's: a foot mass per robot and a fresh slip state per run."""

    def __init__(self, io, B=ROLL_B):
        self.ops = drv._ops(io, B)
        self.io, self.B, self.sol = io, B, self.ops.sol
        self.ground, self.ground_np = self.ops.ground, self.ops.ground_np
        self.grip = _t(np.full(B, 1e3), self.sol.tdtype)
        self.me_np = np.full(B, lite3_model.foot_mass())
        self.me = _t(self.me_np, self.sol.tdtype)

    def state(self):
        import torch
        st = self.ops.state()
        st["slip"] = torch.zeros((self.B, 4, 2), dtype=torch.float64, device="cuda")
        return st

    def drive(self, st, T, land="rule", drive="limited", ground=None, **kw):
        return self.ops.drive(st, T, land, drive, ground, **kw)

    def slip(self, st, T, ground, land="rule", drive="limited", foot_mass=None, **kw):
        return self.sol.rollout_slip(*self.ops._args(st, T), ground, self.me if foot_mass is None else foot_mass, st["slip"], land, drive,
                                     **self.ops._kw(), **kw)


def _ops(io, B=ROLL_B):
    if ("ops", io, B) not in _CACHE:
        _CACHE[("ops", io, B)] = _Ops(io, B)
    return _CACHE[("ops", io, B)]


def _ice(io):
    """The roll-out of test 3, once per I/O dtype: ground 0.3 under the even robots, tau_max x 0.5."""
    import torch
    if ("ice", io) not in _CACHE:
        ops = _ops(io)
        st = ops.state()
        logs = ops.slip(st, ROLL_T, ops.ground, inertia=dc.weak_row(0.5))
        torch.cuda.synchronize()
        _CACHE[("ice", io)] = (ops, st, logs)
    return _CACHE[("ice", io)]


# ------------------------------------------------------------------------------------------------- 2. high friction is rollout_drive
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_high_friction_is_rollout_drive(io):
    import torch
    ops = _ops(io)
    a, b = ops.state(), ops.state()
    ref = ops.drive(a, ROLL_T, "rule", "limited", ops.grip)
    out = ops.slip(b, ROLL_T, ops.grip)
    torch.cuda.synchronize()
    for k in drv.STATE:
        assert torch.equal(a[k], b[k]), k
    for k in DRIVE_LOGS:
        assert torch.equal(ref[k], out[k]) or (bool(torch.isnan(ref[k]).any()) and _same(ref[k], out[k])), k
    assert set(out) == set(ref) | {"slip_log", "disp"}
    assert not bool(out["slip_log"].any()) and not bool(out["disp"].any()) and not bool(b["slip"].any())
    assert int(out["solved"].min()) > 0 and bool((b["tick"] == ROLL_T).all())
    assert not bool((((out["flag"] & 128) != 0) & (out["flag"] != 0xff)).any())


# ------------------------------------------------------------------------------------------------------ 3. replay on slippery ground
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_replay_on_slippery_ground(io):
    import torch
    ops, st, logs = _ice(io)
    sol, B, T = ops.sol, ROLL_B, ROLL_T
    npdt = np.float64 if io == "f64" else np.float32
    weak = dc.weak_row(0.5)
    flag, stance = logs["flag"], logs["contact_log"] != 0
    live = flag != 0xff
    # (a) not vacuous
    n = {bit: int(((flag & bit) != 0)[stance & live].sum()) for bit in (2, 32, 128)}
    print(f"slip roll-out {io}: {n[2]} clamped, {n[32]} ground-limited and {n[128]} sliding stance leg-rows of {int(stance.sum())}; "
          f"largest |disp| {float(logs['disp'].abs().max()):.4f} m; solved {logs['solved'].tolist()}")
    assert n[2] > 0 and n[32] > 0 and n[128] > 0 and bool(live.all())
    assert not bool(((flag & 128) != 0)[~stance].any())
    # (b) device against device: the rule on the logged rows gives the applied forces, the stance torques, the bits and the displacements
    rows = B * T
    rep = sol.stance_slip(logs["actual"].reshape(rows, 12), logs["cmd"].reshape(rows, 12), logs["feet_log"].reshape(rows, 4, 3),
                          logs["contact_log"].reshape(rows, 4), ops.ground.repeat_interleave(T).contiguous(),
                          ops.me.repeat_interleave(T).contiguous(), logs["slip_log"].reshape(rows, 4, 2), inertia=weak)
    torch.cuda.synchronize()
    s = stance.reshape(rows, 4)
    assert torch.equal(rep["f"], logs["forces"].reshape(rows, 12))
    assert torch.equal(rep["tau"][s], logs["tau"].reshape(rows, 4, 3)[s])
    # (bit 16 has a second source on a stance row: the legs step sets it where the held foot is out of reach, which a foot that slides
    #  without a reach stop can be; the rule's own bit 16 needs a clamped leg)
    far = (sol.joint_log(logs["actual"], logs["cmd"], logs["feet_log"])["reach"] == 0).reshape(rows, 4)
    torch.cuda.synchronize()
    print(f"slip roll-out {io}: {int((far & s).sum())} stance leg-rows out of reach")
    assert torch.equal((rep["flag"][s] & sc.BITS) | (far[s] * 16).to(torch.uint8), flag.reshape(rows, 4)[s] & sc.BITS)
    assert torch.equal(rep["flag"][s & ~far] & sc.BITS, flag.reshape(rows, 4)[s & ~far] & sc.BITS)
    assert not bool((rep["flag"][~s] != 0).any())
    assert torch.equal(rep["disp"], logs["disp"].reshape(rows, 4, 2))
    # the slip state: the next row's s0 is this row's s_end where the leg did not touch down (it was then in stance or in swing:
    # 0 after a swing row), 0 at a touchdown; the state left behind is the last row's
    gait, tick0 = ops.ops.pb["gait"], ops.ops.pb["tick"]
    end, slog = _np(rep["slip"]).reshape(B, T, 4, 2), _np(logs["slip_log"])
    assert not end[~_np(stance).astype(bool)].any() and not slog[:, 0].any()
    for t in range(1, T + 1):
        td = gaits.touchdown_mask(gait, tick0 + t)
        nxt = slog[:, t] if t < T else _np(st["slip"])
        assert np.array_equal(nxt[~td], end[:, t - 1][~td]) and not nxt[td].any(), t
    # (c) device against device: the plant received the applied forces, with its feet fixed over the tick
    g = _t(np.repeat(ops.ops.pb["x"][:, 12:13], T - 1, axis=0), sol.tdtype)
    x0 = torch.cat([logs["actual"][:, :-1].reshape(-1, 12), g], dim=1).contiguous()
    wr = _t(gaits.log_wrench(ops.ops.rows["push"], ops.ops.rows["push_ticks"], tick0, T)[:, :-1].reshape(-1, 6), sol.tdtype)
    body = ops.ops.const["body"].repeat_interleave(T - 1, dim=0).contiguous()
    nxt = sol.plant_step(x0, logs["forces"][:, :-1].reshape(-1, 12).contiguous(), logs["feet_log"][:, :-1].reshape(-1, 4, 3).contiguous(),
                         logs["contact_log"][:, :-1].reshape(-1, 4).contiguous(), body, wr)
    torch.cuda.synchronize()
    assert torch.equal(nxt[:, :12], logs["actual"][:, 1:].reshape(-1, 12))
    # the foot-move identity, on the logs in their own dtype
    raw = lambda k: logs[k].cpu().numpy()
    assert sc.foot_move_holds(raw("feet_log"), raw("contact_log"), raw("disp"), gait, tick0, cast=lambda a: a.astype(npdt))
    assert float(logs["disp"].abs().max()) > 1e-4
    # (d) row by row on the host
    h = {k: _np(logs[k]) for k in ("actual", "cmd", "feet_log", "contact_log", "forces", "tau", "flag", "disp")}
    host = lite3_model.stance_slip_host(h["actual"].reshape(rows, 12), h["cmd"].reshape(rows, 12), h["feet_log"].reshape(rows, 4, 3),
                                        h["contact_log"].reshape(rows, 4), np.repeat(_np(ops.ground), T), np.repeat(_np(ops.me), T),
                                        slog.reshape(rows, 4, 2), inertia=weak, delta=DELTA)
    sn = s.cpu().numpy()
    dev = {"f": h["forces"].reshape(rows, 4, 3), "tau": np.where(sn[..., None], h["tau"].reshape(rows, 4, 3), 0.0),
           "flag": np.where(sn, _np(rep["flag"]) & (sc.BITS | 4), 0), "slip": end.reshape(rows, 4, 2), "disp": h["disp"].reshape(rows, 4, 2)}
    _compare_with_host("slip roll-out", io, dev, host, h["cmd"].reshape(rows, 4, 3), np.repeat(_np(ops.me), T), sn)


# ------------------------------------------------------------------------------------------------ 4. composition and edge cases
@pytest.mark.gpu
def test_pieces_null_logs_land_actual_and_determinism():
    import torch
    io, B, T = "f32", 12, 8
    ops = _ops(io, B)
    weak = dc.weak_row(0.5)
    run = lambda st, n, land="rule", ground=ops.ground, **kw: ops.slip(st, n, ground, land, inertia=weak, **kw)
    whole_st = ops.state()
    whole = run(whole_st, T)
    # two pieces are one call, the slip state included
    st = ops.state()
    p1 = run(st, 3)
    p2 = run(st, T - 3)
    # the same call twice gives the same bits
    again_st = ops.state()
    again = run(again_st, T)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(st[k], whole_st[k]) and torch.equal(again_st[k], whole_st[k]), k
    for k in ALL_LOGS:
        if k == "solved":
            assert torch.equal(p1[k] + p2[k], whole[k]) and torch.equal(again[k], whole[k])
        else:
            assert _same(torch.cat([p1[k], p2[k]], dim=1), whole[k]) and _same(again[k], whole[k]), k
    assert int(((whole["flag"] & 128) != 0)[whole["contact_log"] != 0].sum()) > 0 and bool(whole_st["slip"].any() or whole["slip_log"].any())
    # NULL logs: the same closed loop
    quiet_st = ops.state()
    quiet = run(quiet_st, T, log=False)
    torch.cuda.synchronize()
    assert all(quiet[k] is None for k in ALL_LOGS if k != "solved") and torch.equal(quiet["solved"], whole["solved"])
    for k in STATE:
        assert torch.equal(quiet_st[k], whole_st[k]), k
    # land = actual composes: at ground 1e3 it is rollout_drive's land = actual, and on ice the logs still replay
    a, b, c = ops.state(), ops.state(), ops.state()
    ref = ops.drive(a, T, "actual", "limited", ops.grip, inertia=weak)
    grip = run(b, T, "actual", ops.grip)
    ice = run(c, T, "actual")
    torch.cuda.synchronize()
    for k in drv.STATE:
        assert torch.equal(a[k], b[k]), k
    for k in DRIVE_LOGS:
        assert _same(ref[k], grip[k]), k
    assert bool(torch.isfinite(c["x"]).all()) and bool(torch.isfinite(c["feet"]).all()) and not torch.equal(c["feet"], a["feet"])
    rep = ops.sol.stance_slip(ice["actual"].reshape(B * T, 12), ice["cmd"].reshape(B * T, 12), ice["feet_log"].reshape(B * T, 4, 3),
                              ice["contact_log"].reshape(B * T, 4), ops.ground.repeat_interleave(T).contiguous(),
                              ops.me.repeat_interleave(T).contiguous(), ice["slip_log"].reshape(B * T, 4, 2), inertia=weak, want=())
    torch.cuda.synchronize()
    assert torch.equal(rep["f"], ice["forces"].reshape(B * T, 12)) and torch.equal(rep["disp"], ice["disp"].reshape(B * T, 4, 2))
    assert sc.foot_move_holds(ice["feet_log"].cpu().numpy(), ice["contact_log"].cpu().numpy(), ice["disp"].cpu().numpy(), ops.ops.pb["gait"],
                              ops.ops.pb["tick"], cast=lambda v: v.astype(np.float32))


@pytest.mark.gpu
def test_actuator_rows_that_differ_per_robot():
    import torch
    io, B, T = "f32", 12, 8
    ops = _ops(io, B)
    sol = ops.sol
    tmax = lite3_model.leg_inertia()["tau_max"]
    scale = np.linspace(0.35, 1.0, B)
    table = np.concatenate([tmax[None] * scale[:, None], np.tile([6.0, 6.0, 4.0], (B, 1)) * scale[:, None] + 2.0,
                            np.tile([14.0, 14.0, 10.0], (B, 1)) + 4.0 * scale[:, None]], axis=1)
    assert actuators.valid_rows(table).all() and len({tuple(r) for r in table}) == B
    plain_st = ops.state()
    plain = ops.slip(plain_st, T, ops.ground)
    try:
        sol.set_actuators(table)
        st = ops.state()
        out = ops.slip(st, T, ops.ground)
        sol.set_actuators(actuators.tile(table, T))
        rep = sol.stance_slip(out["actual"].reshape(B * T, 12), out["cmd"].reshape(B * T, 12), out["feet_log"].reshape(B * T, 4, 3),
                              out["contact_log"].reshape(B * T, 4), ops.ground.repeat_interleave(T).contiguous(),
                              ops.me.repeat_interleave(T).contiguous(), out["slip_log"].reshape(B * T, 4, 2))
        torch.cuda.synchronize()
    finally:
        sol.clear_actuators()
    s = (out["contact_log"] != 0).reshape(B * T, 4)
    assert torch.equal(rep["f"], out["forces"].reshape(B * T, 12)) and torch.equal(rep["disp"], out["disp"].reshape(B * T, 4, 2))
    assert torch.equal(rep["tau"][s], out["tau"].reshape(B * T, 4, 3)[s])
    assert torch.equal(rep["flag"][s] & (sc.BITS ^ 16), out["flag"].reshape(B * T, 4)[s] & (sc.BITS ^ 16))   # (16: see test 3)
    assert bool((out["flag"] != 0xff).all()) and int(((out["flag"] & 2) != 0)[out["contact_log"] != 0].sum()) > 0
    assert not torch.equal(out["forces"], plain["forces"])                      # the weak rows clamp where the inertia row does not
    # row by row on the host, with the rate of the moving foot in the envelope
    h = {k: _np(out[k]) for k in ("actual", "cmd", "feet_log", "contact_log", "slip_log", "forces", "flag")}
    host = lite3_model.stance_slip_host(h["actual"].reshape(B * T, 12), h["cmd"].reshape(B * T, 12), h["feet_log"].reshape(B * T, 4, 3),
                                        h["contact_log"].reshape(B * T, 4), np.repeat(_np(ops.ground), T), np.repeat(_np(ops.me), T),
                                        h["slip_log"].reshape(B * T, 4, 2), actuators=actuators.tile(table, T), delta=DELTA)
    keep = ~dc.near_threshold(host) & s.cpu().numpy()
    assert (~keep & s.cpu().numpy()).sum() <= dc.MARGIN_SHARE * s.sum().item()
    assert np.array_equal((_np(rep["flag"]) & sc.BITS)[keep], (host["flag"] & sc.BITS)[keep])
    err, band = _error(h["forces"].reshape(B * T, 4, 3)[keep], host["f"].reshape(B * T, 4, 3)[keep], io)
    print(f"actuator rows {io}: f_out err {err:.3e} band {band:.1e}")
    assert err <= band


@pytest.mark.gpu
def test_poison_arguments_and_empty_calls():
    import torch
    io, B, T = "f32", 12, 8
    ops = _ops(io, B)
    weak = dc.weak_row(0.5)
    run = lambda st, n, land="rule", ground=ops.ground, **kw: ops.slip(st, n, ground, land, inertia=weak, **kw)
    whole_st = ops.state()
    whole = run(whole_st, T)
    # a NaN foot_mass row poisons its robot from the first tick; a NaN slip entry its leg, and through the foot its robot; nobody else
    mbad = ops.me.clone()
    mbad[2] = float("nan")
    nst = ops.state()
    l7 = int(np.nonzero(_np(whole["contact_log"][7, 0]))[0][0])
    nst["slip"][7, l7, 1] = float("nan")
    nan = run(nst, T, foot_mass=mbad)
    torch.cuda.synchronize()
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[2] = False; keep[7] = False
    assert bool(torch.isnan(nst["x"][2, :12]).all()) and int(nan["solved"][2]) <= 1
    assert bool((nan["flag"][2, 0][nan["contact_log"][2, 0] != 0] == 0xff).all()) and bool(torch.isnan(nan["actual"][2, 1:]).all())
    assert bool(torch.isfinite(nan["cmd"][2, 0]).all())
    assert int(nan["flag"][7, 0, l7]) == 0xff and bool(torch.isnan(nan["forces"][7, 0, 3 * l7:3 * l7 + 3]).all())
    other_legs = [l for l in range(4) if l != l7]
    assert torch.equal(nan["forces"][7, 0].reshape(4, 3)[other_legs], whole["forces"][7, 0].reshape(4, 3)[other_legs])
    for k in STATE:
        assert torch.equal(nst[k][keep], whole_st[k][keep]), k
    for k in ALL_LOGS:
        assert _same(nan[k][keep], whole[k][keep]), k
    # argument errors, by message
    for bad in ("strong", None):                                               # (None is a wrong mode too, not "no mode")
        with pytest.raises(ValueError, match=f"drive must be 'ideal' or 'limited', got {bad!r}"):
            run(ops.state(), 1, drive=bad)
    with pytest.raises(ValueError, match="land must be"):
        run(ops.state(), 1, land="soft")
    for bad in (2, -1):
        with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_slip: drive is neither MPCQP_DRIVE_IDEAL nor MPCQP_DRIVE_LIMITED"):
            run(ops.state(), 1, drive=bad)
    with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_rollout_slip: substeps out of range \[0, 1000\]"):
        run(ops.state(), 1, substeps=1001)
    with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_rollout_slip: leg_substeps out of range \[0, 1000\]"):
        run(ops.state(), 1, leg_substeps=-1)
    for miss in ("ground", "foot_mass", "slip"):
        with pytest.raises(ValueError, match=f"operand mismatch: {miss} expected"):
            st = ops.state()
            kw = {"ground": ops.ground, "foot_mass": ops.me, "slip": st["slip"]}
            kw[miss] = None
            ops.sol.rollout_slip(*ops.ops._args(st, 1), kw["ground"], kw["foot_mass"], kw["slip"], **ops.ops._kw())
    # ... and at the C-ABI: ground, foot_mass and slip are required there too
    st = ops.state()
    c = ops.ops.const
    p = lambda t: t.data_ptr()
    head = [B, 1, p(st["x"]), p(st["ref"]), p(st["feet"]), p(st["legs"]), p(c["gait"]), p(c["stand"]), p(c["gain"]), p(st["tick"]), p(c["mu"]),
            0, 0, 0, 10, p(c["step_height"]), 0, 0, 0, 1]
    for trio in ((0, p(ops.me), p(st["slip"])), (p(ops.ground), 0, p(st["slip"])), (p(ops.ground), p(ops.me), 0)):
        with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_slip: null buffer"):
            ops.sol.engine.rollout_slip_ptr(*head, *trio, *([0] * 17))
    x13 = torch.cat([whole["actual"][:, 0], torch.zeros((B, 1), dtype=ops.sol.tdtype, device="cuda")], dim=1).contiguous()
    row = [B, p(x13), p(whole["cmd"][:, 0].contiguous()), p(whole["feet_log"][:, 0].contiguous()), p(whole["contact_log"][:, 0].contiguous())]
    fo = torch.empty((B, 12), dtype=ops.sol.tdtype, device="cuda")
    for trio in ((0, p(ops.me), p(st["slip"])), (p(ops.ground), 0, p(st["slip"])), (p(ops.ground), p(ops.me), 0)):
        with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_stance_slip: null buffer"):
            ops.sol.engine.stance_slip_ptr(*row, *trio, p(fo))
    with pytest.raises(mpcqp.MpcQpError, match=r"code -1: mpcqp_stance_slip: substeps out of range \[0, 1000\]"):
        ops.sol.engine.stance_slip_ptr(*row, p(ops.ground), p(ops.me), p(st["slip"]), p(fo), substeps=-3)
    with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_stance_slip: batch size out of range"):
        ops.sol.engine.stance_slip_ptr(-1, *row[1:], p(ops.ground), p(ops.me), p(st["slip"]), p(fo))
    # T = 0 and B = 0 are no-ops
    zst = ops.state()
    zero = run(zst, 0)
    torch.cuda.synchronize()
    fresh = ops.state()
    for k in STATE:
        assert torch.equal(zst[k], fresh[k]), k
    assert zero["actual"].shape == (B, 0, 12) and zero["slip_log"].shape == (B, 0, 4, 2) and not bool(zero["solved"].any())
    ops.sol.engine.rollout_slip_ptr(0, 4, *([0] * 9), 0, 0, 0, 10, 0, 0, 0, 0, 1, 0, 0, 0, *([0] * 17))
    ops.sol.engine.stance_slip_ptr(0, 0, 0, 0, 0, 0, 0, 0, 0)


@pytest.mark.gpu
def test_the_gate():
    plib = mpcqp.product_library()
    assert plib.has_slip and all(plib.calls[s][0] is not None for s in mpcqp._capi.SLIP_SYMBOLS)
