"""Cases shared by tests/test_rollout_legs_host.py and tests/test_gpu_rollout_legs.py (include/mpcqp_sim.h, mpcqp_rollout_legs): the
end-to-end roll-out of legsim_cases.rollout_batch() with the swing legs inside it, on the CPU checker; the one-row replay of a
roll-out's leg logs on the host; the growth of one row, which the replay test's band is multiplied by (recorded in
tests/golden/rollout_legs_growth.npz); and the 60-tick report of `solved` counts and height error per named gait."""
import functools
import os

import numpy as np

from conftest import ORACLE_SO                                                  # (first: it puts the repository on the path)
import mpcqp
from legsim_cases import DELTA, ROLL_B, ROLL_T, STEP_HEIGHT, rollout_batch
from mpcqp import gaits, lite3_model, synth

ROW_GROWTH_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_legs_growth.npz")
STATE = ("x", "ref", "feet", "legs", "tick")                                   # what a roll-out carries from call to call
PHASE_LOGS = ("actual", "desired", "forces", "feet_log", "contact_log", "solved")
LEG_LOGS = gaits.LEGS_LOGS                                                        # swing, q, qd, tau, foot, err, flag, miss
REPORT_T = 60


def checker_engine():
    lib = mpcqp.Library(ORACLE_SO)
    return lib, mpcqp.Engine(lib, lib.default_config(N=10, delta=DELTA, max_iter=4000))


@functools.lru_cache(maxsize=None)
def host_loop(land, T=ROLL_T):
    """rollout_legs_host on rollout_batch(): (pb, rows, result)."""
    pb, rows = rollout_batch()
    lib, eng = checker_engine()
    o = gaits.rollout_legs_host(eng, pb["x"], pb["ref"], pb["feet"], np.zeros((ROLL_B, 4, 7)), pb["gait"], pb["stand"], pb["gain"], pb["tick"],
                                pb["mu"], T, np.full(ROLL_B, STEP_HEIGHT), land, rows["body"], rows["push"], rows["push_ticks"])
    return pb, rows, o


def landings(contact_log):
    """bool [B,T,4]: leg l touches down at the tick after row t (swing at t, stance at t + 1); the last row is never one."""
    up = np.asarray(contact_log) == 0
    out = np.zeros_like(up)
    out[:, :-1] = up[:, :-1] & ~up[:, 1:]
    return out


def replay_rows(logs, pb, rows, tick0, step_height=STEP_HEIGHT, state=None, **kw):
    """The host's one-row step from every row t of a roll-out's logs (fp64 arrays): the row's operands (actual, desired, forces,
    feet_log), the leg state the row started from (q_log, qd_log, live where the row is a swing row) -> the state after the row,
    [B,T,4,7], and the host's result for the rows.  Each row is a robot of its own to the host calls, so nothing is carried here.
    `state` [B,T,4,7] replaces the logged start state (the growth measurement perturbs it)."""
    B, T = logs["actual"].shape[:2]
    rep = lambda a: np.repeat(np.asarray(a), T, axis=0)                         # robot-major, like the logs flattened
    flat = lambda a: np.asarray(a).reshape((B * T, 1) + np.asarray(a).shape[2:])
    tick = (np.asarray(tick0, np.int64)[:, None] + np.arange(T)[None, :]).reshape(-1).astype(np.int32)
    sw = gaits.phase_swing_host(flat(logs["actual"]), flat(logs["desired"]), flat(logs["feet_log"]), rep(pb["gait"]), tick, rep(pb["stand"]),
                                rep(pb["gain"]), np.full(B * T, step_height), DELTA)["swing"]
    wr = gaits.log_wrench(rows["push"], rows["push_ticks"], tick0, T)
    acc = lite3_model.plant_base_acc_host(flat(logs["actual"]), flat(logs["forces"]), flat(logs["feet_log"]), rep(rows["body"]), wrench=flat(wr))
    if state is None:
        live = (np.asarray(logs["contact_log"]) == 0).astype(np.float64)
        state = np.concatenate([logs["q"], logs["qd"], live[..., None]], axis=-1)
    out = lite3_model.swing_track_host(flat(logs["actual"]), flat(logs["forces"]), flat(logs["feet_log"]), flat(logs["contact_log"]), sw, acc,
                                       state=np.nan_to_num(state.reshape(B * T, 4, 7)), delta=DELTA, **kw)
    return out["state"].reshape(B, T, 4, 7), out


def row_growth(logs, pb, rows, tick0, eps=1e-10, seed=9):
    """The largest ratio of the change of a swing row's end state (q, qd) to a perturbation eps of its start state, over the rows of
    these logs: what one row of the tracker does to a rounding difference in the state it is handed."""
    live = (np.asarray(logs["contact_log"]) == 0).astype(np.float64)
    st = np.concatenate([logs["q"], logs["qd"], live[..., None]], axis=-1)
    st2 = st.copy()
    st2[..., :6] += eps * np.random.default_rng(seed).choice([-1.0, 1.0], st[..., :6].shape)
    a, _ = replay_rows(logs, pb, rows, tick0, state=st)
    b, _ = replay_rows(logs, pb, rows, tick0, state=st2)
    up = live != 0
    d = np.abs(a[..., :6] - b[..., :6])[up]
    return float(np.nanmax(d)) / eps


def measure_row_growth():
    pb, rows, o = host_loop("actual")
    return row_growth(o, pb, rows, pb["tick"])


@functools.lru_cache(maxsize=None)
def gait_report(tau_scale=1.0, T=REPORT_T):
    """One robot per named gait, T ticks, land = rule and land = actual on the same robots with tau_max scaled: per gait the `solved`
    count, the worst and the RMS |z - H_COM|, the worst landing miss and the number of swing rows with a clamped torque,
    {land: {name: (solved, worst height error, RMS height error, miss, clamped rows)}}."""
    names = tuple(gaits.GAITS)
    pb = gaits.make_phase_batch(len(names), names, 12, seed=6)
    B = len(names)
    inr = lite3_model.leg_inertia()
    inr = dict(inr, tau_max=np.asarray(inr["tau_max"]) * tau_scale)
    lib, eng = checker_engine()
    out = {}
    for land in ("rule", "actual"):
        o = gaits.rollout_legs_host(eng, pb["x"], pb["ref"], pb["feet"], np.zeros((B, 4, 7)), pb["gait"], pb["stand"], pb["gain"], pb["tick"],
                                    pb["mu"], T, np.full(B, STEP_HEIGHT), land, inertia=inr)
        with np.errstate(invalid="ignore"):
            dz = o["actual"][:, :, 5] - synth.H_COM
            herr, hrms = np.abs(dz).max(axis=1), np.sqrt((dz * dz).mean(axis=1))
        out[land] = {n: (int(o["solved"][b]), float(herr[b]), float(hrms[b]), float(np.nan_to_num(o["miss"][b], nan=np.inf).max()),
                         int((((o["flag"][b] & 2) != 0) & (o["flag"][b] != 0xff)).sum())) for b, n in enumerate(names)}
    return out


def report_lines(rep, tau_scale):
    lines = [f"tau_max x {tau_scale:g}, {REPORT_T} ticks: gait | solved rule / actual | height error worst, RMS rule / worst, RMS actual [mm] | worst "
             f"landing miss rule / actual [mm] | swing rows with a clamped torque rule / actual"]
    for n in rep["rule"]:
        r, a = rep["rule"][n], rep["actual"][n]
        lines.append(f"  {n:12s} | {r[0]:3d} / {a[0]:3d} | {r[1] * 1e3:7.2f}, {r[2] * 1e3:7.3f} / {a[1] * 1e3:7.2f}, {a[2] * 1e3:7.3f} | {r[3] * 1e3:6.2f} / {a[3] * 1e3:6.2f} | "
                     f"{r[4]:3d} / {a[4]:3d}")
    return lines


if __name__ == "__main__":                                                      # regenerate tests/golden/rollout_legs_growth.npz
    g = measure_row_growth()
    np.savez(ROW_GROWTH_NPZ, growth=np.float64(g), eps=np.float64(1e-10))
    print("one-row growth", g)
