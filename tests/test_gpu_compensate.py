"""mpcqp_rollout_observe_compensated on the device (include/mpcqp_compensate.h): the wrench observer and the table update inside the
tick loop of rollout_observe.  The cases are in tests/compensate_cases.py: the pushed trot robots of tests/disturbance_cases.py as a
leg roll-out, tiled to B robots, N = 10, period 12, T <= 24.

  1. The twin, bit for bit: the call against disturbance.compensated_rollout composed on the same device of set_disturbance,
     rollout_observe, disturbance_track and set_disturbance, for both sources, two holds, both I/O types and four batch sizes, with
     the closing update of a T that is no multiple of hold; once with the gated, aided estimator in the feedback and a model table.
  2. Pieces that are multiples of hold are the uncut call.
  3. Without a gain nothing moves; compensate=None is today's call.
  4. The host twin, in the bands of tests/test_gpu_disturbance.py's compensated roll-out.
  5. It estimates the push and an untold payload.
  6. It helps the pushed robots.
  7. Poison, argument errors, the table that stays.

Equality is of values (np.array_equal with equal NaNs): -0 and +0 may differ."""
import functools

import numpy as np
import pytest

import compensate_cases as K
import disturbance_cases as C
import mpcqp
from mpcqp import disturbance

pytestmark = pytest.mark.gpu
STATE = ("x", "ref", "feet", "legs", "tick", "slip", "est")
OBSERVER_OUT = ("dist", "resid")


def _t(a, dt):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _np(v):
    return v.cpu().numpy().copy() if hasattr(v, "cpu") else v


def _host(d):
    import torch
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in d.items() if v is not None}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


class _Ops:
    """The device operands of the fixture tiled to B robots: the constant rows once, a fresh copy of the state per run."""

    def __init__(self, io, B):
        import torch
        self.io, self.B, self.pb = io, B, K.batch(B)
        cap = 10 * mpcqp.product_library().default_config(N=10).max_iter      # (tests/test_gpu_disturbance.py's solver)
        self.sol = mpcqp.MPCBatch(N=10, delta=C.DELTA, io_dtype=io, precision="mixed", max_iter=cap)
        pb, dt = self.pb, self.sol.tdtype
        self.c = {k: _t(pb[k], dt) for k in ("stand", "gain", "mu", "step_height", "ground", "foot_mass", "height", "est_init", "push",
                                             "model_body", "heavy_body")}
        self.c["gait"], self.c["push_ticks"] = _t(pb["gait"], torch.int32), _t(pb["push_ticks"], torch.int32)

    def state(self):
        import torch
        dt, z = self.sol.tdtype, lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
        return {"x": _t(self.pb["x"], dt), "ref": _t(self.pb["ref"], dt), "feet": _t(self.pb["feet"], dt), "legs": z(self.B, 4, 7),
                "tick": _t(self.pb["tick"], torch.int32), "slip": z(self.B, 4, 2), "est": z(self.B, 131), "dist": z(self.B, 40)}

    def observe(self, st, T, feed="truth", heavy=True, **kw):
        """rollout_observe on the carried state, under the push and (heavy) the payload; with compensate= the state's observer rides along."""
        c = self.c
        if kw.get("compensate") is not None:
            kw["dist_state"] = st["dist"]
        if kw.get("attitude") is not None:
            kw["att_state"] = st.setdefault("att", _t(np.zeros((self.B, 8)), st["est"].dtype))
        return self.sol.rollout_observe(st["x"], st["ref"], st["feet"], st["legs"], c["gait"], c["stand"], c["gain"], st["tick"], c["mu"], T,
                                        c["step_height"], c["ground"], c["foot_mass"], st["slip"], st["est"], feed, est_init=c["est_init"],
                                        height=c["height"], push=c["push"], push_ticks=c["push_ticks"],
                                        body=c["heavy_body"] if heavy else None, **kw)


@functools.lru_cache(maxsize=None)
def _ops(io, B):
    return _Ops(io, B)


def _composed(ops, T, hold, source, feed="truth", heavy=True, observer=None, st=None, **kw):
    """disturbance.compensated_rollout at piece = hold on the device -> (the final state, the joined logs), as numpy."""
    import torch
    sol = ops.sol
    st = ops.state() if st is None else st
    pieces = []
    view = disturbance.sensed_logs if source == "sensed" else (lambda logs: logs)

    def step(n):
        pieces.append(ops.observe(st, n, feed, heavy, **kw))
        return pieces[-1]

    sol.set_disturbance(st["dist"][:, :6].contiguous())
    out = disturbance.compensated_rollout(step, T, hold, lambda logs, s: sol.disturbance_track(view(logs), observer=observer, state=s),
                                          sol.set_disturbance, st["dist"])
    logs = {k: (sum(p[k] for p in pieces[1:]) + pieces[0][k]) if k == "solved" else
            (pieces[-1][k] if k == "att_state" else torch.cat([p[k] for p in pieces], dim=1)) for k in pieces[0]}
    return _host(st), _host({**logs, "dist": out["dist"], "resid": out["resid"]})


def _new(ops, T, hold, source, feed="truth", heavy=True, observer=None, st=None, **kw):
    st = ops.state() if st is None else st
    out = ops.observe(st, T, feed, heavy, compensate={"source": source, "hold": hold, **(observer or {})}, **kw)
    return _host(st), _host(out)


def _assert_twin(got, want, what):
    (gs, gl), (ws, wl) = got, want
    for k in ws:
        assert _same(gs[k], ws[k]), (what, "state", k)
    assert set(gl) == set(wl) | {"dist_state"}, (what, set(gl) ^ set(wl))
    for k in wl:
        assert _same(gl[k], wl[k]), (what, k)
    assert _same(gl["dist_state"], ws["dist"])


# ----------------------------------------------------------------------------------------------------------- 1. the twin, bit for bit
@pytest.mark.parametrize("B", [1, 63, 65, 257])
@pytest.mark.parametrize("io", ["f32", "f64"])
@pytest.mark.parametrize("hold", [1, 3])
@pytest.mark.parametrize("source", ["truth", "sensed"])
def test_the_call_is_the_composed_loop(source, hold, io, B):
    ops = _ops(io, B)
    try:
        for T, h in ((12, hold), (11, 3)):                                       # (11 at hold 3: the closing update on the last tick)
            got, want = _new(ops, T, h, source), _composed(ops, T, h, source)
            _assert_twin(got, want, (T, h))
            assert np.isfinite(got[1]["dist"]).all() and got[1]["dist"].shape == (B, T, 6)
        if B > 1:                                                                # the pushed robots' estimates moved, so the table did
            assert np.abs(got[1]["dist"][1, -1, 0]) > 1.0
    finally:
        ops.sol.clear_disturbance()


@pytest.mark.parametrize("source", ["truth", "sensed"])
def test_the_call_is_the_composed_loop_with_the_estimate_fed_back(source):
    """feed="estimate" with the gate and the aided rule, under a model table whose rows differ: 65 robots."""
    ops = _ops("f64", 65)
    B, sol = ops.B, ops.sol
    scale = np.linspace(0.9, 1.2, B)
    models = np.stack([sol.cfg.m * scale, 0.24 * scale, 1.0 * scale, 1.0 * scale, np.full(B, sol.cfg.f_min), sol.cfg.f_max * np.linspace(0.8, 1.0, B)],
                      axis=1)
    kw = dict(feed="estimate", gate={}, attitude={})
    try:
        sol.set_models(models)
        got, want = _new(ops, 12, 3, source, **kw), _composed(ops, 12, 3, source, **kw)
        _assert_twin(got, want, source)
        assert {"trust", "gyro_bias", "att_state"} <= set(got[1])
        plain = _new(ops, 12, 3, source, feed="estimate")                        # the plain estimator is another run
        assert "trust" not in plain[1] and "gyro_bias" not in plain[1] and not _same(plain[1]["est"], got[1]["est"])
    finally:
        sol.clear_disturbance()
        sol.clear_models()


# ------------------------------------------------------------------------------------------------------------------------ 2. pieces
@pytest.mark.parametrize("hold", [1, 3])
@pytest.mark.parametrize("source", ["truth", "sensed"])
def test_pieces_are_the_uncut_call(source, hold):
    ops = _ops("f32", 65)
    try:
        whole_st, whole = _new(ops, 12, hold, source)
        st = ops.state()
        _, p1 = _new(ops, 6, hold, source, st=st)
        cut_st, p2 = _new(ops, 6, hold, source, st=st)
    finally:
        ops.sol.clear_disturbance()
    for k in whole_st:
        assert _same(cut_st[k], whole_st[k]), k
    for k in whole:
        if k == "solved":
            assert np.array_equal(p1[k] + p2[k], whole[k])
        elif k == "dist_state":
            assert _same(p2[k], whole[k])
        else:
            assert _same(np.concatenate([p1[k], p2[k]], axis=1), whole[k]), k


# ------------------------------------------------------------------------------------------------- 3. without the observer nothing moves
@pytest.mark.parametrize("io", ["f32", "f64"])
def test_without_a_gain_it_is_rollout_observe_under_zero_rows(io):
    ops = _ops(io, 65)
    try:
        got_st, got = _new(ops, 12, 1, "truth", observer={"kappa": 0.0})
        st = ops.state()
        ops.sol.set_disturbance(disturbance.wrench_rows(ops.B))
        want = _host(ops.observe(st, 12))
        want_st = _host(st)
    finally:
        ops.sol.clear_disturbance()
    assert "dist" not in want and "resid" not in want and "dist_state" not in want     # compensate=None: today's call, today's keys
    for k in STATE:
        assert _same(got_st[k], want_st[k]), k
    for k in want:
        assert _same(got[k], want[k]), k
    assert not got["dist"].any() and np.abs(got["resid"][1, 1:, 0]).min() > 1.0


# ------------------------------------------------------------------------------------------------------------------- 4. the host twin
def test_the_host_twin():
    """Source truth, feed truth, hold 1, 12 ticks of the four fixture robots without the payload, against rollout_compensated_host in
    the bands of tests/test_gpu_disturbance.py's compensated roll-out: forces 1e-4 of their scale, states 1e-5, and the estimates by
    its formula."""
    T = 12
    ops = _ops("f64", C.B_FIX)
    try:
        _, dev = _new(ops, T, 1, "truth", heavy=False)
    finally:
        ops.sol.clear_disturbance()
    host = K.host_run("truth", 1, T)
    assert np.all(dev["solved"] == T) and np.all(host["solved"] == T)
    sc = max(1.0, np.abs(host["forces"]).max())
    ef, ea = np.abs(dev["forces"] - host["forces"]).max(), np.abs(dev["actual"] - host["actual"]).max()
    ed = np.abs(dev["dist"] - host["dist"])
    bf, bt = C.checker().cfg.m * 2e-5 / C.DELTA + 4e-4 * sc, 2e-5 / C.DELTA + 4.0 * (0.5e-4 * sc + 2e-5 * sc)
    print(f"compensated roll-out vs its host twin: forces {ef:.3e} (band {1e-4 * sc:.3e}), states {ea:.3e} (band 1e-5), "
          f"estimates {ed[..., :3].max():.3e} N (band {bf:.3e}), {ed[..., 3:].max():.3e} N m (band {bt:.3e})")
    assert ef <= 1e-4 * sc and ea <= 1e-5
    assert ed[..., :3].max() <= bf and ed[..., 3:].max() <= bt


# ------------------------------------------------------------------------------------------------------- 5. it estimates what is there
def test_it_estimates_the_push_and_the_payload():
    T = 24
    ops = _ops("f64", C.B_FIX)
    try:
        _, told = _new(ops, T, 1, "truth", heavy=False)
        _, heavy = _new(ops, T, 1, "truth", heavy=True)                           # obs_body = None: the observer believes the model
    finally:
        ops.sol.clear_disturbance()
    F = C.PUSH[:, :3]
    sc = max(1.0, np.abs(told["forces"]).max())
    bf = C.checker().cfg.m * 2e-5 / C.DELTA + 4e-4 * sc
    err = np.abs(told["dist"][:, -1, :3] - F)
    print("estimate after 24 ticks", np.round(told["dist"][:, -1, :3], 4).tolist(), "error - band, worst", (err - (0.8 ** 23 * np.abs(F) + bf)).max())
    assert np.all(err <= 0.8 ** 23 * np.abs(F) + bf)                               # d^ = (1 - 0.8^n) res after n = 23 live rows
    fz = float(heavy["resid"][:, 1:, 2].mean())
    print("payload: mean F_z residual", fz, "against", -K.PAYLOAD * 9.81)
    assert abs(fz + K.PAYLOAD * 9.81) < 0.5


# ------------------------------------------------------------------------------------------------------------------------- 6. it helps
def test_it_helps_the_pushed_robots():
    """On the host (rollout_compensated_host, 24 ticks, every tick solved): final CoM error of the pushed robots 4.8, 4.8 and 28.0 mm
    with the observer against 13.6, 33.8 and 73.7 mm without a gain."""
    T = 24
    ops = _ops("f64", 2 * C.B_FIX)
    try:
        _, on = _new(ops, T, 1, "truth", heavy=False)
        _, off = _new(ops, T, 1, "truth", heavy=False, observer={"kappa": 0.0})
    finally:
        ops.sol.clear_disturbance()
    assert np.all(on["solved"] == T) and np.all(off["solved"] == T)
    pushed = np.arange(ops.B) % C.B_FIX != 0
    e_on, e_off = C.final_xy_error(on)[pushed], C.final_xy_error(off)[pushed]
    print("final CoM error [mm]: observer", np.round(1e3 * e_on, 2).tolist(), "no gain", np.round(1e3 * e_off, 2).tolist())
    assert np.all(e_on < e_off)


# ----------------------------------------------------------------------------------------------------------- 7. poison and arguments
@pytest.mark.parametrize("what", ["dist_state", "obs_body"])
def test_poison(what):
    import torch
    T, bad = 6, 2
    ops = _ops("f64", 5)
    keep = np.arange(ops.B) != bad
    try:
        clean_st, clean = _new(ops, T, 1, "truth")
        st, kw = ops.state(), {}
        if what == "dist_state":
            st["dist"][bad, 10] = float("nan")                                   # (not in d^: the table of tick 0 is finite)
        else:
            body = ops.c["model_body"].clone()
            body[bad, 2] = float("nan")
            kw = {"observer": {"body": body}}
        got_st, got = _new(ops, T, 1, "truth", st=st, **kw)
    finally:
        ops.sol.clear_disturbance()
    for k in OBSERVER_OUT:
        assert np.isnan(got[k][bad]).all(), k
    assert np.isnan(got["dist_state"][bad]).all() and np.isnan(got_st["dist"][bad]).all()
    assert int(got["solved"][bad]) == 1 and np.all(got["solved"][keep] == T)     # tick 0 solves, every later QP is NONFINITE
    assert not got["cmd"][bad, 1:].any() and got["cmd"][bad, 0].any()
    for k in clean_st:
        assert _same(got_st[k][keep], clean_st[k][keep]), k
    for k in clean:
        assert _same(got[k][keep], clean[k][keep]), k


def test_arguments_and_the_table_that_stays():
    import torch
    ops = _ops("f64", 5)
    sol, lib, who = ops.sol, ops.sol.engine.library, "code -1: mpcqp_rollout_observe_compensated: "
    run = lambda comp, st=None, T=1: ops.observe(ops.state() if st is None else st, T, compensate=comp)
    cases = ((lambda p: setattr(p, "source", 2), "compensate: source is neither MPCQP_WRENCH_TRUTH nor MPCQP_WRENCH_SENSED"),
             (lambda p: setattr(p, "hold", 0), "compensate: hold must be at least 1"),
             (lambda p: setattr(p, "size", 8), "compensate struct size mismatch"),
             (lambda p: setattr(p, "flags", 4), "compensate: flags has a bit other than"),
             (lambda p: setattr(p.observer, "size", 8), "wrench observer struct size mismatch"),
             (lambda p: setattr(p.observer, "gravity", 1.0), "wrench observer: gravity"),
             (lambda p: setattr(p.observer, "kappa", 1.5), "wrench observer: kappa"),
             (lambda p: setattr(p.observer, "f_lim", -1.0), "wrench observer: f_lim"),
             (lambda p: setattr(p.observer, "t_lim", float("nan")), "wrench observer: f_lim and t_lim"))
    try:
        for spoil, said in cases:
            par = lib.default_compensate()
            spoil(par)
            with pytest.raises(mpcqp.MpcQpError, match=who + said):
                run(par)
        with pytest.raises(ValueError, match="hold must be"):
            run({"hold": 0})
        with pytest.raises(ValueError, match="source must be"):
            run({"source": "both"})
        with pytest.raises(ValueError, match="dist_state needs compensate"):
            ops.observe(ops.state(), 1, dist_state=ops.state()["dist"])
        # at the C-ABI dist_state is required
        st, c, p = ops.state(), ops.c, (lambda t: t.data_ptr())
        head = [ops.B, 1, p(st["x"]), p(st["ref"]), p(st["feet"]), p(st["legs"]), p(c["gait"]), p(c["stand"]), p(c["gain"]), p(st["tick"]),
                p(c["mu"]), 0, 0, 0, 10, p(c["step_height"]), 0, 0, 0, 1, p(c["ground"]), p(c["foot_mass"]), p(st["slip"])]
        with pytest.raises(mpcqp.MpcQpError, match=who + "null dist_state buffer"):
            sol.engine.rollout_observe_compensated_ptr(*head, *([0] * 28), 0, p(st["est"]))
        assert sol.engine.library.calls["mpcqp_set_disturbance"][0] is not None
        # B = 0 and T = 0 are no-ops: no table is set
        sol.engine.rollout_observe_compensated_ptr(0, 4, *([0] * 21), *([0] * 28), 0, 0)
        zst, fresh = ops.state(), _host(ops.state())
        zero = _host(run({}, zst, 0))
        assert zero["dist"].shape == (ops.B, 0, 6) and all(_same(v, fresh[k]) for k, v in _host(zst).items())
        pb8 = _ops("f64", 8)
        x8 = pb8.state()                                                          # (eight robots' operands for this handle)
        solve8 = lambda: sol.solve_batch_phase(x8["x"], x8["ref"], x8["feet"], pb8.c["gait"], x8["tick"], pb8.c["stand"], pb8.c["gain"], pb8.c["mu"])
        solve8()                                                                  # no table yet: 8 robots solve
        # after a call a table of B rows is set: a solve at another B is refused, and clear_disturbance takes the table back
        run({}, T=2)
        with pytest.raises(mpcqp.MpcQpError, match=rf"mpcqp_solve_batch_phase: batch size 8, but the disturbance table has {ops.B} rows"):
            solve8()
        sol.clear_disturbance()
        solve8()
        torch.cuda.synchronize()
    finally:
        sol.clear_disturbance()
