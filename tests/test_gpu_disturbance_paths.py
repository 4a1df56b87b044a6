"""The disturbance table (include/mpcqp_disturb.h) on every path its header promises, with wrench rows that differ per robot; the
cases, and the conditions they meet on the CPU, are in tests/disturbance_path_cases.py and tests/test_disturbance_paths_host.py.

  1. A table is exactly "shift, solve, add back": over the grid of engines, horizons, I/O types and discretisations, with and without a
     model table, the solve with the table equals -- bit for bit -- the table-less solve of the shifted tuple, and its X is that solve's
     X plus s, rounded once.
  2. Against the checker with both tables (models.grouped_host + DisturbedEngine), at the bands of tests/batch_checks.py.
  3. The ordered launch scores the shifted xdes: against one workgroup per QP in batch order, bitwise, with non-finite and huge rows.
  4. Lifecycle: want_X=False, a table replaced without a clear, growth of the table, warm-started engines, a side stream.
  5. Every roll-out reads row b for robot b, against its host twin through DisturbedEngine.
  6. The size mismatch names the entry point.

Bands.  Single QPs: 1e-4 relative on forces, 1e-4 absolute on states (tests/batch_checks.py).  The shift: estimate_cases.error.  Closed
loops: forces within 1e-4 of their scale and states within 1e-5, what tests/test_rollout.py, test_gpu_plant.py, test_gpu_gaits.py and
test_gpu_disturbance.py's _rollout_band hold for the table-less loops (disturbance_path_cases.loop_band)."""
import functools

import numpy as np
import pytest

import disturbance_path_cases as P
import drive_cases as dc
import mpcqp
from batch_checks import check_batch
from conftest import rel_err
from mpcqp import disturbance

pytestmark = pytest.mark.gpu
D, MR = P.D, P.MR
KEYS = ("u", "X", "status", "iters", "res")
SENTINEL = -7777
GRID_IDS = [g[0] for g in P.GRID]


def _t(a, dt):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().copy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def _flags(engine):
    return mpcqp.FLAG_POLISH | (mpcqp.FLAG_STAGE_KERNEL if engine == "stage_flag" else 0)


def _cap(N, flags=mpcqp.FLAG_POLISH):
    return 10 * mpcqp.product_library().default_config(N=N, flags=flags).max_iter


def _make(N, io, precision="mixed", engine="dense", disc="euler", **kw):
    flags = kw.pop("flags", _flags(engine))
    return mpcqp.MPCBatch(N=N, delta=P.DELTA, io_dtype=io, precision=precision, flags=flags, max_iter=_cap(N, flags),
                          **P.engine_overrides(engine, disc), **kw)


def _solve(sol, dev, want_X=True, **kw):
    return _host(sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=want_X, **kw))


def _bits(a, b):
    """Bit for bit, NaN payloads and the sign of zero included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------- 1. a table is shift, solve, add back
@pytest.mark.parametrize("models", [False, True], ids=["config-model", "model-table"])
@pytest.mark.parametrize("point", P.GRID, ids=GRID_IDS)
def test_a_table_is_shift_solve_add_back(point, models):
    import torch
    name, N, B, io, precision, engine, disc = point
    b, rows, mod, nan_row = P.solve_case(N, B, io=io)
    mod = mod if models else None
    sol = _make(N, io, precision, engine, disc)
    dev = sol.upload(b)
    # s in fp64: the shift of a zero xdes on a handle of the same configuration with fp64 I/O, negated.  (The arithmetic of the two
    # kernels is fp64 whatever the I/O type; an fp32 handle would return s rounded, and X + s is rounded once, not twice.)
    wide = sol if io == "f64" else _make(N, "f64", precision, engine, disc)
    if mod is not None:
        sol.set_models(mod)
        wide.set_models(mod)
    sol.set_disturbance(rows)
    table = _solve(sol, dev)
    xs = sol.disturbance_shift(dev["x0"], dev["xdes"])
    if wide is not sol:
        wide.set_disturbance(rows)
    x0w = dev["x0"].double()
    s = -_host({"s": wide.disturbance_shift(x0w, torch.zeros((B, N + 1, 13), dtype=torch.float64, device="cuda"))})["s"]
    sol.clear_disturbance()                                                            # (the model table stays)
    plain = _solve(sol, dict(dev, xdes=xs))
    hit = np.arange(B) == nan_row
    # the shift kernel against the host, in its own band
    s_host, fin = disturbance.offsets_host(b["x0"], rows, sol.cfg, mod)
    assert np.array_equal(~fin, hit)
    for what, d, h, dt in (("s", s, np.where(fin[:, None, None], s_host, np.nan), "f64"),
                           ("xdes - s", _host({"x": xs})["x"], disturbance.shift_host(b["x0"], b["xdes"], rows, sol.cfg, mod), io)):
        err, band = D.error(d, h, dt)
        print(f"{name} models={'yes' if models else 'no'} {what}: error {err:.3e}, band {band:.3e}")
        assert err <= band, what
    assert np.abs(s[~hit]).max() > 1e-2                                                # not vacuous
    # the solve never knew: everything but X is the table-less solve of the shifted tuple, bit for bit
    for k in ("u", "status", "iters", "res"):
        assert _bits(table[k], plain[k]), (name, k)
    # ... and X is that solve's X plus s, rounded once into the I/O type
    want = (plain["X"].astype(np.float64) + np.where(hit[:, None, None], 0.0, s)).astype(table["X"].dtype)
    assert np.array_equal(table["X"], want), (name, np.abs(table["X"].astype(np.float64) - want).max())
    assert np.abs(table["X"].astype(np.float64) - plain["X"])[~hit].max() > 1e-2
    # the robot with the NaN row fails alone
    st = table["status"]
    assert st[nan_row] == -1 and not np.any(table["u"][nan_row]) and not np.any(table["X"][nan_row])
    assert np.isin(st[~hit], (1, 2)).all(), st


# ------------------------------------------------------------------------------------------- 2. against the checker, with both tables
@pytest.mark.parametrize("point", [P.GRID[0], P.GRID[2], P.GRID[4]], ids=[GRID_IDS[0], GRID_IDS[2], GRID_IDS[4]])
def test_both_tables_against_the_checker(point):
    """allowed = 0 on seed 0 of disturbance_cases.shift_case at every point."""
    name, N, B, io, precision, engine, disc = point
    b, rows, mod, nan_row = P.solve_case(N, B, io=io)
    ref = P.solve_reference(b, rows, mod, N, P.engine_overrides(engine, disc))
    assert np.all(np.delete(ref["status"], nan_row) == 1)
    sol = _make(N, io, precision, engine, disc)
    sol.set_models(mod)
    sol.set_disturbance(rows)
    out = _solve(sol, sol.upload(b))
    shifted = P.shifted_tuple(b, rows, sol.cfg, mod)                                   # its finite-input accounting sees the NaN row
    ok = check_batch(out, shifted, ref, max_iter=_cap(N, _flags(engine)), allowed=0, tol=1e-4, x_tol=1e-4, what=f"{name} with both tables")
    print(f"{name} with both tables: worst force error {rel_err(out['u'], ref['u'])[ok].max():.3e} (band 1e-4), "
          f"worst state error {np.abs(out['X'].astype(np.float64) - ref['X'])[ok].max():.3e} (band 1e-4)")
    assert ok.sum() == B - 1


# ----------------------------------------------------------------------------------------------- 3. the ordered launch with a table
def _ordered(batch, rows, mod, N, io, flags):
    import torch
    sol = mpcqp.MPCBatch(N=N, delta=0.03, io_dtype=io, precision="mixed", flags=flags)
    dev = sol.upload(batch)
    B = len(batch["mu"])
    sol.set_models(mod)
    sol.set_disturbance(rows)
    pre = sol._outputs(B, True, None)                                                  # the buffers the solve will write: sentinel first
    pre["status"].fill_(SENTINEL); pre["iters"].fill_(SENTINEL)
    out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True)
    torch.cuda.synchronize()
    assert out["status"].data_ptr() == pre["status"].data_ptr()
    res = {k: out[k].cpu().numpy().copy() for k in KEYS}
    sol.engine.close()
    return res


@pytest.mark.parametrize("B,N,io,seed", P.ORDER_SIZES, ids=[f"B{s[0]}-n{s[1]}-{s[2]}" for s in P.ORDER_SIZES])
def test_ordered_launch_with_a_table_is_a_reordering(B, N, io, seed):
    batch, rows, mod, bad, huge = P.order_case(B, N, seed)
    ordered = _ordered(batch, rows, mod, N, io, mpcqp.FLAG_POLISH)
    natural = _ordered(batch, rows, mod, N, io, mpcqp.FLAG_POLISH | mpcqp.FLAG_NATURAL_ORDER)
    for name, o in (("ordered", ordered), ("natural", natural)):
        left = np.nonzero((o["status"] == SENTINEL) | (o["iters"] == SENTINEL))[0]
        assert left.size == 0, f"{name}: QPs {left[:8].tolist()} were never solved"
    for k in KEYS:
        assert ordered[k].dtype == natural[k].dtype and ordered[k].shape == natural[k].shape, k
        diff = np.nonzero((ordered[k].reshape(B, -1).view(np.uint8) != natural[k].reshape(B, -1).view(np.uint8)).any(axis=1))[0]
        assert diff.size == 0, f"{k}: rows {diff[:8].tolist()} differ between the ordered and the plain launch"
    st = ordered["status"]
    hit = np.zeros(B, bool); hit[bad] = True
    assert np.array_equal(st == -1, hit), (np.nonzero(st == -1)[0].tolist(), sorted(bad.tolist()))
    plain = np.setdiff1d(np.arange(B), np.concatenate([bad, huge]))
    share = float(np.isin(st[plain], (1, 2)).mean())
    print(f"ordered launch with a table B={B} N={N} {io}: {100 * share:.2f} % of the plain rows solved")
    assert share >= 0.99


# --------------------------------------------------------------------------------------------------------------------- 4. lifecycle
def test_want_x_false_skips_the_add_back_and_changes_nothing_else():
    b, rows, _, _ = P.solve_case(10, 24)
    sol = _make(10, "f64")
    dev = sol.upload(b)
    sol.set_disturbance(rows)
    with_x, without = _solve(sol, dev, True), _solve(sol, dev, False)
    assert without["X"] is None
    for k in ("u", "status", "iters"):
        assert _bits(with_x[k], without[k]), k


def test_a_table_replaced_without_a_clear_and_a_table_that_grows():
    b40, rows40, _, _ = P.solve_case(10, 40, seed=3)
    b16 = {k: v[:16] for k, v in b40.items()}
    rows_a, rows_b = P.wrench_rows(16, seed=4), P.wrench_rows(16, seed=5)
    fresh = lambda b, rows: (lambda s: (s.set_disturbance(rows), _solve(s, s.upload(b)))[1])(_make(10, "f64"))
    sol = _make(10, "f64")
    d16, d40 = sol.upload(b16), sol.upload(b40)
    sol.set_disturbance(rows_a)
    first = _solve(sol, d16)
    sol.set_disturbance(rows_b)                                                        # (b) replaced, never cleared
    second = _solve(sol, d16)
    sol.set_disturbance(rows40)                                                        # (c) the table and the shifted-xdes buffer grow
    grown = _solve(sol, d40)
    sol.set_disturbance(rows_a)
    again = _solve(sol, d16)
    want_b, want_40 = fresh(b16, rows_b), fresh(b40, rows40)
    for k in KEYS:
        assert _bits(second[k], want_b[k]), ("replaced", k)
        assert _bits(grown[k], want_40[k]), ("grown", k)
        assert _bits(again[k], first[k]), ("back at 16", k)
    assert not _bits(first["u"], second["u"])


@pytest.mark.parametrize("shift", [False, True], ids=["warm", "warm-shift"])
def test_a_warm_started_engine_with_the_table(shift):
    """Two consecutive solves of one tuple with the table on a warm-started engine, each held against the checker in the band of test 2;
    the second starts from the first's optimum and reports fewer ADMM iterations in total than a cold solve."""
    b, rows, _, nan_row = P.solve_case(10, 24, nan=False)
    ref = P.solve_reference(b, rows, None, 10)
    assert np.all(ref["status"] == 1) and nan_row is None
    cold_sol = _make(10, "f64")
    cold_sol.set_disturbance(rows)
    cold = _solve(cold_sol, cold_sol.upload(b))
    sol = _make(10, "f64", warm_start=True, warm_shift=shift)
    sol.set_disturbance(rows)
    dev = sol.upload(b)
    shifted = P.shifted_tuple(b, rows, sol.cfg)
    total = []
    for i in range(2):
        out = _solve(sol, dev)
        check_batch(out, shifted, ref, max_iter=_cap(10), allowed=0, tol=1e-4, x_tol=1e-4, what=f"warm solve {i} with a table")
        total.append(int(mpcqp.split_iters(out["iters"])[0].sum()))
    n_cold = int(mpcqp.split_iters(cold["iters"])[0].sum())
    print(f"warm engine (warm_shift={shift}) with a table: ADMM iterations cold {n_cold}, first {total[0]}, second {total[1]}")
    assert total[1] < n_cold


def test_a_side_stream():
    import torch
    b, rows, mod, _ = P.solve_case(10, 24)
    sol = _make(10, "f64")
    sol.set_models(mod)
    sol.set_disturbance(rows)
    want = _solve(sol, sol.upload(b))
    other = _make(10, "f64")
    dev, side = other.upload(b), torch.cuda.Stream()
    torch.cuda.synchronize()                                                           # the uploads, before the side stream reads them
    other.set_models(mod, stream=side)
    other.set_disturbance(rows, stream=side)
    got = _solve(other, dev, stream=side)
    for k in KEYS:
        assert _bits(got[k], want[k]), k


# --------------------------------------------------------------------------------------------- 5. every roll-out reads the table
def _hold(what, out, ref, T):
    """Device logs against the host twin's in the closed loops' band; prints every figure before it asserts."""
    fb, sb = P.loop_band(ref)
    figures = {"commanded forces": (np.abs(P.commanded(out) - P.commanded(ref)).max(), fb), "actual": (np.abs(out["actual"] - ref["actual"]).max(), sb),
               "desired": (np.abs(out["desired"] - ref["desired"]).max(), 1e-12)}
    for k, (err, band) in figures.items():
        print(f"{what} with a disturbance table vs its host twin: {k} err {err:.3e} band {band:.3e}")
    assert np.all(out["solved"] == T) and np.all(ref["solved"] == T), (what, out["solved"])
    for k, (err, band) in figures.items():
        assert err <= band, (what, k, err, band)


@functools.lru_cache(maxsize=None)
def _loop_solver():
    return mpcqp.MPCBatch(N=10, delta=P.DELTA, io_dtype="f64", precision="mixed")


def _plan_call(sol, kind, T=None):
    """rollout (kind "plan") or rollout_plant on the plan-table case, in the engine's current table state."""
    import torch
    rb, rows, T0 = P.plan_case()
    T, dt = T0 if T is None else T, sol.tdtype
    d = {k: _t(rb[k], dt) for k in ("x", "ref", "plan_pos", "mu")}
    d.update(plan_feet_id=_t(rb["plan_feet_id"], torch.uint8), plan_meta=_t(rb["plan_meta"], torch.int32), tick=_t(rb["tick"], torch.int32))
    a = [d[k] for k in P.PLAN_ARGS]
    if kind == "plan":
        out = _host(sol.rollout(*a, T))
    else:
        out = _host(sol.rollout_plant(*a, T, push=_t(rows, dt), push_ticks=_t(P.plan_ticks(), torch.int32)))
    out.update(x=d["x"].cpu().numpy(), ref=d["ref"].cpu().numpy(), tick=d["tick"].cpu().numpy())
    return out, T


def _plan_run(sol, kind, rows):
    try:
        sol.set_disturbance(rows)
        return _plan_call(sol, kind)
    finally:
        sol.clear_disturbance()


@pytest.mark.parametrize("kind", ["plan", "plant"])
def test_rollout_and_rollout_plant_read_the_table(kind):
    """mpcqp_rollout is the roll-out whose next state is X[:,1]: the add-back is in its closed loop."""
    out, T = _plan_run(_loop_solver(), kind, P.plan_case()[1])
    ref = P.host_loop(kind)
    _hold("rollout" if kind == "plan" else "rollout_plant", out, ref, T)
    assert np.abs(out["x"] - ref["x"]).max() <= 1e-5 and np.abs(out["ref"] - ref["ref"]).max() <= 1e-12 and np.all(out["tick"] == T)


def _phase_run(sol, rows, models=None, body=None):
    import torch
    pb, _, idx, T = P.phase_case()
    dt = sol.tdtype
    st = {k: _t(pb[k][idx], dt) for k in ("x", "ref", "feet")}
    st["tick"] = _t(pb["tick"][idx], torch.int32)
    try:
        if models is not None:
            sol.set_models(models)
        sol.set_disturbance(rows)
        out = _host(sol.rollout_phase(st["x"], st["ref"], st["feet"], _t(pb["gait"][idx], torch.int32), _t(pb["stand"][idx], dt), _t(pb["gain"][idx], dt),
                                      st["tick"], _t(pb["mu"][idx], dt), T, body=_t(body, dt), push=_t(D.PUSH[idx], dt),
                                      push_ticks=_t(D.PUSH_TICKS[idx], torch.int32)))
    finally:
        sol.clear_disturbance()
        sol.clear_models()
    return out, T


def test_rollout_phase_reads_both_tables():
    ref, mod, body = P.host_loop_models("phase")
    out, T = _phase_run(_loop_solver(), P.phase_case()[1], mod, body)
    _hold("rollout_phase with a model table", out, ref, T)


class _Legs:
    """The device operands of the legs family on the case of disturbance_path_cases.legs_case (tests/test_gpu_rollout_observe.py's
    pattern): the constant rows once, a fresh copy of the state per run."""

    def __init__(self, yaw=False):
        import torch
        self.pb, self.pr, self.rows, self.T = P.legs_case(yaw)
        self.sol = _loop_solver()
        pb, dt, B = self.pb, self.sol.tdtype, P.LEGS_B
        self.B = B
        self.const = {k: _t(pb[k], dt) for k in ("stand", "gain", "mu", "step_height", "ground", "foot_mass", "height", "bias", "noise", "enc_noise",
                                                 "est_init")}
        self.const["gait"] = _t(pb["gait"], torch.int32)
        self.plant = lambda body=None: {"body": _t(self.pr["body"] if body is None else body, dt), "push": _t(self.pr["push"], dt),
                                        "push_ticks": _t(self.pr["push_ticks"], torch.int32)}

    def state(self):
        import torch
        dt, z = self.sol.tdtype, lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
        return {"x": _t(self.pb["x"], dt), "ref": _t(self.pb["ref"], dt), "feet": _t(self.pb["feet"], dt), "legs": z(self.B, 4, 7),
                "tick": _t(self.pb["tick"], torch.int32), "slip": z(self.B, 4, 2), "est": z(self.B, 131)}

    def run(self, kind, T=None, body=None):
        """One roll-out of `kind` (disturbance_path_cases.LOOPS) from a fresh state, in the engine's current table state."""
        c, st, T = self.const, self.state(), self.T if T is None else T
        a = (st["x"], st["ref"], st["feet"], st["legs"], c["gait"], c["stand"], c["gain"], st["tick"], c["mu"], T, c["step_height"])
        weak = dict(inertia=dc.weak_row(0.5), **self.plant(body))
        if kind == "legs":
            out = self.sol.rollout_legs(*a, "rule", **self.plant(body))
        elif kind == "drive":
            out = self.sol.rollout_drive(*a, "rule", "limited", c["ground"], **weak)
        elif kind == "slip":
            out = self.sol.rollout_slip(*a, c["ground"], c["foot_mass"], st["slip"], **weak)
        else:
            out = self.sol.rollout_observe(*a, c["ground"], c["foot_mass"], st["slip"], st["est"], est_init=c["est_init"], height=c["height"],
                                           bias=c["bias"], noise=c["noise"][:, :T].contiguous(), enc_noise=c["enc_noise"][:, :T].contiguous(),
                                           **P.OBSERVE[kind], **weak)
        out = _host({k: v for k, v in out.items() if v is not None})
        used = ("x", "ref", "feet", "legs", "tick") + (() if kind in ("legs", "drive") else ("slip",) if kind == "slip" else ("slip", "est"))
        out.update({k: st[k].cpu().numpy() for k in used})                             # the state the call advanced in place
        return out

    def told(self, kind, rows=None, models=None, body=None):
        try:
            if models is not None:
                self.sol.set_models(models)
            self.sol.set_disturbance(self.rows if rows is None else rows)
            return self.run(kind, body=body)
        finally:
            self.sol.clear_disturbance()
            self.sol.clear_models()


@functools.lru_cache(maxsize=None)
def _legs(yaw=False):
    return _Legs(yaw)


@functools.lru_cache(maxsize=None)
def _told(kind):
    """The device roll-out `kind` under the case's rows, once per process; shared, not to be altered."""
    return _legs(kind == "observe_yaw").told(kind)


@pytest.mark.parametrize("kind", [k for k in P.LOOPS if k not in ("plan", "plant", "phase")])
def test_the_legs_family_reads_the_table(kind):
    """rollout_legs (land = rule), the limited rollout_drive, rollout_slip, and rollout_observe on both feeds, gated, aided, and with an
    estimate whose yaw is 0.3 rad off on the odd robots: there the shift's Rz must be the estimate's, not the plant's."""
    out = _told(kind)
    _hold(kind, out, P.host_loop(kind), P.LEGS_T)


def test_truth_feed_with_a_table_is_rollout_slip_with_that_table():
    a, b = _told("observe_truth"), _told("slip")
    for k in b:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert set(a) > set(b)


def test_rollout_legs_reads_both_tables():
    ref, mod, body = P.host_loop_models("legs")
    out = _legs().told("legs", models=mod, body=body)
    _hold("rollout_legs with a model table", out, ref, P.LEGS_T)


def test_a_nan_row_fails_alone_in_rollout_slip():
    ops, good = _legs(), _told("slip")
    rows = ops.rows.copy()
    rows[3, 1] = np.nan
    bad = ops.told("slip", rows)
    keep = np.arange(ops.B) != 3
    assert bad["solved"][3] == 0 and not np.any(bad["cmd"][3]) and np.all(bad["solved"][keep] == P.LEGS_T)
    for k in good:
        assert np.array_equal(bad[k][keep], good[k][keep], equal_nan=True), k


# ------------------------------------------------------------------------------------------ 6. the size mismatch names the entry point
def test_a_wrong_batch_size_names_every_entry_point():
    import torch
    ops = _legs()
    sol, B = ops.sol, ops.B                                                            # 8 robots against a table of 16 rows
    g = mpcqp.synth.make_gait_batch(B, N=10)
    gd = sol.upload_gait(g)
    pb = ops.pb
    calls = {
        "mpcqp_solve_batch_gait(_steps)?": lambda: sol.solve_batch_gait(gd["x0"], gd["ref"], gd["feet0"], gd["footholds"], gd["gait"], gd["feet_id"], gd["mu"]),
        "mpcqp_solve_batch_phase": lambda: sol.solve_batch_phase(_t(pb["x"], sol.tdtype), _t(pb["ref"], sol.tdtype), _t(pb["feet"], sol.tdtype),
                                                                 ops.const["gait"], _t(pb["tick"], torch.int32), ops.const["stand"], ops.const["gain"],
                                                                 ops.const["mu"]),
        "mpcqp_rollout": lambda: _plan_call(sol, "plan", 1), "mpcqp_rollout_plant": lambda: _plan_call(sol, "plant", 1),
        "mpcqp_rollout_legs": lambda: ops.run("legs", 1), "mpcqp_rollout_drive": lambda: ops.run("drive", 1),
        "mpcqp_rollout_slip": lambda: ops.run("slip", 1), "mpcqp_rollout_observe": lambda: ops.run("observe_estimate", 1),
        "mpcqp_rollout_observe_gated": lambda: ops.run("observe_gated", 1), "mpcqp_rollout_observe_aided": lambda: ops.run("observe_aided", 1)}
    try:
        sol.set_disturbance(np.ones((16, 6)))
        for name, call in calls.items():
            with pytest.raises(mpcqp.MpcQpError, match=rf"(?s){name}: batch size {B}\b.*disturbance.*\b16\b"):
                call()
    finally:
        sol.clear_disturbance()
    for call in calls.values():                                                        # without a table the same calls run
        call()
    torch.cuda.synchronize()
