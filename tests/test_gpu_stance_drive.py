"""The stance drive on the device (include/mpcqp_sim.h, mpcqp_stance_drive / mpcqp_rollout_drive).

  1. stance_drive against lite3_model.stance_drive_host on drive_cases.clamp_draw(): 33 robots (132 legs, a partial block), about
     half the stance legs clamped, swing legs, pulling legs, slippery ground under the even robots; both I/O dtypes.
  2. drive = ideal with ground = None is rollout_legs, bit for bit, on legsim_cases.rollout_batch().
  3. drive = limited in the loop (tau_max x 0.5, ground 0.3 under the even robots): the logs replay through stance_drive and
     plant_step on the device bit for bit, and through stance_drive_host within the band of 1.
  4. Pieces, land = actual, NULL logs, the drive argument, a NaN ground row.

The band is that of tests/test_gpu_joint_rates.py for the same J and the same cofactor solve on the same joint box: 1e-9 for fp64 I/O,
2 float32 spacings against the host value rounded once for fp32 I/O.  Legs within legsim_cases.FLAG_MARGIN of a threshold that decides
a bit or a branch are left out of the comparison; that they are at most 2 % of the legs is asserted here and, for the draw, on the CPU
(tests/test_stance_drive_host.py)."""
import numpy as np
import pytest

import drive_cases as dc
import mpcqp
from legsim_cases import DELTA, ROLL_B, ROLL_T, STEP_HEIGHT, rollout_batch
from mpcqp import gaits, lite3_model

_CACHE = {}
LEG_LOGS = ("swing", "q", "qd", "tau", "foot", "err", "flag", "miss")
ALL_LOGS = ("actual", "desired", "forces", "feet_log", "contact_log", "solved") + LEG_LOGS
STATE = ("x", "ref", "feet", "legs", "tick")


def _t(a, dt):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _np(t):
    a = t.cpu().numpy()
    return a.astype(np.float64) if a.dtype.kind == "f" else a


def _ulps32(dev, host64):
    """fp32 device values against the fp64 host values rounded once, in float32 spacings (floor 2^-20); NaN must match NaN."""
    ref = np.asarray(host64, np.float64).astype(np.float32)
    dev = np.asarray(dev, np.float32)
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(dev))
    sp = np.spacing(np.maximum(np.abs(ref[~nan]), np.float32(2.0 ** -20)))
    err = np.abs(dev[~nan].astype(np.float64) - ref[~nan].astype(np.float64)) / sp
    return float(err.max()) if err.size else 0.0


def _error(dev, host, io):
    """(error, band): fp64 |dev - host| against 1e-9, fp32 float32 spacings against 2; the NaN pattern must match."""
    if io == "f32":
        return _ulps32(dev, host), dc.F32_SPACINGS
    dev, host = np.asarray(dev, np.float64), np.asarray(host, np.float64)
    nan = np.isnan(host)
    assert np.array_equal(nan, np.isnan(dev))
    return (float(np.abs(dev[~nan] - host[~nan]).max()) if (~nan).any() else 0.0), dc.F64_BAND


def _compare_with_host(tag, io, dev, host, f_in, contact):
    """The comparison of tests 1 and 3 (d): flags equal; f_out bit-equal to f where the leg is neither clamped nor limited by the
    ground; elsewhere f_out and tau within the band.  dev = {"f" [n,4,3], "tau" [n,4,3], "flag" [n,4]} as numpy, f_in [n,4,3]."""
    near = dc.near_threshold(host)
    print(f"{tag} {io}: {int(near.sum())} of {near.size} legs within FLAG_MARGIN of a threshold")
    assert near.mean() <= dc.MARGIN_SHARE
    keep = ~near
    assert np.array_equal(dev["flag"][keep], host["flag"][keep])
    hf = host["f"].reshape(-1, 4, 3)
    free = keep & ((host["flag"] & 34) == 0)
    assert np.array_equal(dev["f"][free], f_in[free], equal_nan=True)
    rest = keep & ~free
    for k, d, h in (("f_out", dev["f"], hf), ("tau", dev["tau"], host["tau"])):
        err, band = _error(d[rest], h[rest], io)
        print(f"{tag} {io} {k}: err {err:.3e} band {band:.1e} on {int(rest.sum())} legs (max |{k}| {np.nanmax(np.abs(h[rest])):.1f})")
        assert err <= band, (k, err)
    err, band = _error(dev["tau"][free], host["tau"][free], io)
    print(f"{tag} {io} tau of the free legs: err {err:.3e} band {band:.1e}")
    assert err <= band


# ---------------------------------------------------------------------------------------------------- 1. stance_drive against the host
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_stance_drive_against_the_host(io):
    import torch
    npdt = np.float64 if io == "f64" else np.float32
    c = dc.as_io(dc.clamp_draw(), npdt)
    host = dc.drive(c)
    moved = dc.drive(dc.as_io(dc.clamp_draw(dq=1e-12), npdt))
    ok = (host["flag"] != 0xff) & (moved["flag"] == host["flag"])
    print(f"host's own sensitivity, q moved by 1e-12: f_out {np.abs(moved['f'] - host['f']).reshape(-1, 4, 3)[ok].max():.3e}, "
          f"tau {np.abs(moved['tau'] - host['tau'])[ok].max():.3e}")
    sol = mpcqp.MPCBatch(io_dtype=io)
    dt = sol.tdtype
    x, f, feet, ground = (_t(c[k], dt) for k in ("x", "f", "feet", "ground"))
    contact = _t(c["contact"], torch.uint8)
    out = sol.stance_drive(x, f, feet, contact, ground)
    torch.cuda.synchronize()
    st = c["contact"] != 0
    fl = host["flag"]
    assert ((fl & 2) != 0)[st].sum() >= 20 and ((fl & 32) != 0)[st].sum() >= 20 and (~st).sum() >= 10 and not np.any(fl == 0xff)
    dev = {"f": _np(out["f"]).reshape(-1, 4, 3), "tau": _np(out["tau"]), "flag": _np(out["flag"])}
    _compare_with_host("stance_drive", io, dev, host, _np(f).reshape(-1, 4, 3), c["contact"])
    assert not dev["tau"][~st].any() and not dev["flag"][~st].any()
    # ground = None skips only the cone; in place; optional outputs
    none = sol.stance_drive(x, f, feet, contact, None, want=())
    hn = lite3_model.stance_drive_host(c["x"], c["f"], c["feet"], c["contact"], None)
    fin = f.clone()
    sol.engine.stance_drive_ptr(33, x.data_ptr(), fin.data_ptr(), feet.data_ptr(), contact.data_ptr(), 0, fin.data_ptr())
    torch.cuda.synchronize()
    assert none["tau"] is None and none["flag"] is None and torch.equal(fin, none["f"])
    free = (hn["flag"] & 34) == 0
    assert np.array_equal(_np(none["f"]).reshape(-1, 4, 3)[free], _np(f).reshape(-1, 4, 3)[free])
    err, band = _error(_np(none["f"]).reshape(-1, 4, 3)[~free], hn["f"].reshape(-1, 4, 3)[~free], io)
    assert err <= band
    # a poisoned robot and a poisoned leg; nobody else changes
    xb, gb, fb = x.clone(), ground.clone(), f.clone()
    xb[3, 1] = float("nan"); gb[5] = -0.5
    l9 = int(np.nonzero(c["contact"][9])[0][0])
    fb[9, 3 * l9 + 2] = float("inf")
    bad = sol.stance_drive(xb, fb, feet, contact, gb)
    sol.stance_drive(x[:0], f[:0], feet[:0], contact[:0], None)                 # the empty batch
    torch.cuda.synchronize()
    for b in (3, 5):
        assert bool((bad["flag"][b] == 0xff).all()) and bool(torch.isnan(bad["f"][b]).all()) and bool(torch.isnan(bad["tau"][b]).all())
    assert int(bad["flag"][9, l9]) == 0xff and bool(torch.isnan(bad["tau"][9, l9]).all()) and bool(torch.isnan(bad["f"][9, 3 * l9:3 * l9 + 3]).all())
    others = torch.ones((33, 4), dtype=torch.bool, device="cuda")
    others[3] = False; others[5] = False; others[9, l9] = False
    for k in ("tau", "flag"):
        assert torch.equal(bad[k][others], out[k][others]), k
    assert torch.equal(bad["f"].reshape(33, 4, 3)[others], out["f"].reshape(33, 4, 3)[others])


# ------------------------------------------------------------------------------------------------------------- the roll-out's operands
def _case(io, B=ROLL_B):
    pb, rows = rollout_batch()
    if io == "f32":
        pb = {k: (_r32(v) if k in ("x", "ref", "feet", "stand", "gain", "mu") else v) for k, v in pb.items()}
        rows = dict(rows, body=_r32(rows["body"]), push=_r32(rows["push"]))
    if B != ROLL_B:
        pb = {k: v[:B] for k, v in pb.items()}
        rows = {k: v[:B] for k, v in rows.items()}
    return pb, rows


class _Ops:
    """The device operands of one batch: the constant rows once, a fresh copy of the state per run."""

    def __init__(self, io, B=ROLL_B):
        import torch
        self.io, self.B = io, B
        self.pb, self.rows = _case(io, B)
        self.sol = mpcqp.MPCBatch(N=10, delta=DELTA, io_dtype=io, precision="mixed")
        dt, pb, rows = self.sol.tdtype, self.pb, self.rows
        self.const = {"gait": _t(pb["gait"], torch.int32), "stand": _t(pb["stand"], dt), "gain": _t(pb["gain"], dt), "mu": _t(pb["mu"], dt),
                      "body": _t(rows["body"], dt), "push": _t(rows["push"], dt), "push_ticks": _t(rows["push_ticks"], torch.int32),
                      "step_height": _t(np.full(B, STEP_HEIGHT), dt)}
        self.ground_np = np.where(np.arange(B) % 2 == 0, dc.GROUND_MU, 1e3)
        self.ground = _t(self.ground_np, dt)

    def state(self):
        import torch
        dt = self.sol.tdtype
        return {"x": _t(self.pb["x"], dt), "ref": _t(self.pb["ref"], dt), "feet": _t(self.pb["feet"], dt),
                "legs": torch.zeros((self.B, 4, 7), dtype=torch.float64, device="cuda"), "tick": _t(self.pb["tick"], torch.int32)}

    def _args(self, st, T):
        c = self.const
        return (st["x"], st["ref"], st["feet"], st["legs"], c["gait"], c["stand"], c["gain"], st["tick"], c["mu"], T, c["step_height"])

    def _kw(self):
        c = self.const
        return {"body": c["body"], "push": c["push"], "push_ticks": c["push_ticks"]}

    def legs(self, st, T, land="rule", **kw):
        return self.sol.rollout_legs(*self._args(st, T), land, **self._kw(), **kw)

    def drive(self, st, T, land="rule", drive="limited", ground=None, **kw):
        return self.sol.rollout_drive(*self._args(st, T), land, drive, ground, **self._kw(), **kw)


def _ops(io, B=ROLL_B):
    if ("ops", io, B) not in _CACHE:
        _CACHE[("ops", io, B)] = _Ops(io, B)
    return _CACHE[("ops", io, B)]


def _limited(io):
    """The limited roll-out of test 3, once per I/O dtype: tau_max x 0.5, ground 0.3 under the even robots."""
    import torch
    if ("limited", io) not in _CACHE:
        ops = _ops(io)
        st = ops.state()
        logs = ops.drive(st, ROLL_T, "rule", "limited", ops.ground, inertia=dc.weak_row(0.5))
        torch.cuda.synchronize()
        _CACHE[("limited", io)] = (ops, st, logs)
    return _CACHE[("limited", io)]


# -------------------------------------------------------------------------------------------------------- 2. ideal is rollout_legs
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_ideal_drive_is_rollout_legs(io):
    import torch
    ops = _ops(io)
    a, b = ops.state(), ops.state()
    ref = ops.legs(a, ROLL_T)
    out = ops.drive(b, ROLL_T, "rule", "ideal", None)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(a[k], b[k]), k
    for k in ALL_LOGS:
        assert torch.equal(ref[k], out[k]) or (bool(torch.isnan(ref[k]).any()) and np.array_equal(_np(ref[k]), _np(out[k]), equal_nan=True)), k
    assert torch.equal(out["cmd"], out["forces"]) and int(out["solved"].min()) > 0 and bool((b["tick"] == ROLL_T).all())
    assert set(out) == set(ref) | {"cmd"}


# ------------------------------------------------------------------------------------------------------ 3. limited, in the loop
@pytest.mark.gpu
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_limited_drive_in_the_loop(io):
    import torch
    ops, st, logs = _limited(io)
    sol, B, T = ops.sol, ROLL_B, ROLL_T
    weak = dc.weak_row(0.5)
    flag, stance = logs["flag"], logs["contact_log"] != 0
    live = flag != 0xff
    # (a) not vacuous
    n2, n32 = int(((flag & 2) != 0)[stance & live].sum()), int(((flag & 32) != 0)[stance & live].sum())
    print(f"limited roll-out {io}: {n2} clamped and {n32} ground-limited stance leg-rows of {int(stance.sum())}; solved {logs['solved'].tolist()}")
    assert n2 > 0 and n32 > 0 and bool(live.all())
    # (b) device against device: the rule on the logged rows gives the applied forces, the stance torques and the bits
    rows = B * T
    ground_rows = ops.ground.repeat_interleave(T).contiguous()
    rep = sol.stance_drive(logs["actual"].reshape(rows, 12), logs["cmd"].reshape(rows, 12), logs["feet_log"].reshape(rows, 4, 3),
                           logs["contact_log"].reshape(rows, 4), ground_rows, inertia=weak)
    torch.cuda.synchronize()
    s = stance.reshape(rows, 4)
    assert torch.equal(rep["f"], logs["forces"].reshape(rows, 12))
    assert torch.equal(rep["tau"][s], logs["tau"].reshape(rows, 4, 3)[s])
    assert torch.equal(rep["flag"][s] & dc.BITS, flag.reshape(rows, 4)[s] & dc.BITS)
    assert not bool((rep["flag"][~s] != 0).any())
    changed = (logs["cmd"] != logs["forces"]).reshape(B, T, 4, 3).any(dim=-1)
    assert int(changed.sum()) > 0 and not bool((changed & ~(stance & ((flag & 34) != 0))).any())
    # (c) device against device: the plant received the applied forces
    g = _t(np.repeat(ops.pb["x"][:, 12:13], T - 1, axis=0), sol.tdtype)
    x0 = torch.cat([logs["actual"][:, :-1].reshape(-1, 12), g], dim=1).contiguous()
    wr = _t(gaits.log_wrench(ops.rows["push"], ops.rows["push_ticks"], ops.pb["tick"], T)[:, :-1].reshape(-1, 6), sol.tdtype)
    body = ops.const["body"].repeat_interleave(T - 1, dim=0).contiguous()
    nxt = sol.plant_step(x0, logs["forces"][:, :-1].reshape(-1, 12).contiguous(), logs["feet_log"][:, :-1].reshape(-1, 4, 3).contiguous(),
                         logs["contact_log"][:, :-1].reshape(-1, 4).contiguous(), body, wr)
    torch.cuda.synchronize()
    assert torch.equal(nxt[:, :12], logs["actual"][:, 1:].reshape(-1, 12))
    assert bool((wr != 0).any())
    # (d) row by row on the host
    h = {k: _np(logs[k]) for k in ("actual", "cmd", "feet_log", "contact_log", "forces", "tau", "flag")}
    host = lite3_model.stance_drive_host(h["actual"].reshape(rows, 12), h["cmd"].reshape(rows, 12), h["feet_log"].reshape(rows, 4, 3),
                                         h["contact_log"].reshape(rows, 4), np.repeat(_np(ops.ground), T), inertia=weak)
    dev = {"f": h["forces"].reshape(rows, 4, 3), "tau": np.where(s.cpu().numpy()[..., None], h["tau"].reshape(rows, 4, 3), 0.0),
           "flag": np.where(s.cpu().numpy(), h["flag"].reshape(rows, 4) & (dc.BITS | 4), 0)}
    _compare_with_host("limited roll-out", io, dev, host, h["cmd"].reshape(rows, 4, 3), h["contact_log"].reshape(rows, 4))


# ------------------------------------------------------------------------------------------------ 4. composition and edge cases
@pytest.mark.gpu
def test_pieces_land_actual_null_logs_and_arguments():
    import torch
    io, B, T = "f32", 12, 8
    ops = _ops(io, B)
    weak = dc.weak_row(0.5)
    run = lambda st, n, land="rule", drive="limited", ground=ops.ground, **kw: ops.drive(st, n, land, drive, ground, inertia=weak, **kw)
    whole_st = ops.state()
    whole = run(whole_st, T)
    # two pieces are one call
    st = ops.state()
    p1 = run(st, 3)
    p2 = run(st, T - 3)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(st[k], whole_st[k]), k
    for k in ALL_LOGS + ("cmd",):
        if k == "solved":
            assert torch.equal(p1[k] + p2[k], whole[k])
        else:
            assert np.array_equal(_np(torch.cat([p1[k], p2[k]], dim=1)), _np(whole[k]), equal_nan=True), k
    assert int(((whole["flag"] & 34) != 0)[whole["contact_log"] != 0].sum()) > 0
    # NULL logs: the same closed loop
    quiet_st = ops.state()
    quiet = run(quiet_st, T, log=False)
    torch.cuda.synchronize()
    assert all(quiet[k] is None for k in ALL_LOGS + ("cmd",) if k != "solved") and torch.equal(quiet["solved"], whole["solved"])
    for k in STATE:
        assert torch.equal(quiet_st[k], whole_st[k]), k
    # land = actual composes with the drive: ideal / None is rollout_legs' land = actual, and the limited one lands elsewhere
    a, b, c = ops.state(), ops.state(), ops.state()
    ref = ops.legs(a, T, "actual")
    idl = ops.drive(b, T, "actual", "ideal", None)
    lim = run(c, T, "actual")
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(a[k], b[k]), k
    for k in ALL_LOGS:
        assert np.array_equal(_np(ref[k]), _np(idl[k]), equal_nan=True), k
    assert bool(torch.isfinite(c["x"]).all()) and bool(torch.isfinite(c["feet"]).all())
    rep = ops.sol.stance_drive(lim["actual"].reshape(B * T, 12), lim["cmd"].reshape(B * T, 12), lim["feet_log"].reshape(B * T, 4, 3),
                               lim["contact_log"].reshape(B * T, 4), ops.ground.repeat_interleave(T).contiguous(), inertia=weak, want=())
    torch.cuda.synchronize()
    assert torch.equal(rep["f"], lim["forces"].reshape(B * T, 12))
    # the drive argument
    for bad in ("strong", None):                                               # (None is a wrong mode too, not "no mode")
        with pytest.raises(ValueError, match=f"drive must be 'ideal' or 'limited', got {bad!r}"):
            run(ops.state(), 1, drive=bad)
    for bad in (2, -1):
        with pytest.raises(mpcqp.MpcQpError, match="code -1: mpcqp_rollout_drive: drive is neither MPCQP_DRIVE_IDEAL nor MPCQP_DRIVE_LIMITED"):
            run(ops.state(), 1, drive=bad)
    with pytest.raises(ValueError, match="land must be"):
        run(ops.state(), 1, land="soft")
    run(ops.state(), 0)                                                        # T = 0 is a no-op
    # a NaN ground row: that robot's solves report NONFINITE from the next tick, nobody else changes
    gbad = ops.ground.clone()
    gbad[2] = float("nan")
    nst = ops.state()
    nan = run(nst, T, ground=gbad)
    torch.cuda.synchronize()
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[2] = False
    assert bool(torch.isnan(nst["x"][2, :12]).all()) and int(nan["solved"][2]) <= 1 and bool((nan["flag"][2, 0][nan["contact_log"][2, 0] != 0] == 0xff).all())
    assert bool(torch.isnan(nan["actual"][2, 1:]).all()) and bool(torch.isfinite(nan["cmd"][2, 0]).all())
    for k in STATE:
        assert torch.equal(nst[k][keep], whole_st[k][keep]), k
    for k in ALL_LOGS + ("cmd",):
        assert np.array_equal(_np(nan[k][keep]), _np(whole[k][keep]), equal_nan=True), k


@pytest.mark.gpu
def test_the_gate():
    plib = mpcqp.product_library()
    assert plib.has_sim and plib.has_drive and all(plib.calls[s][0] is not None for s in mpcqp._capi.DRIVE_SYMBOLS)
