"""Cases shared by tests/test_disturbance_host.py and tests/test_gpu_disturbance.py (include/mpcqp_disturb.h):

  fixture    four trot robots (gaits.make_phase_batch(4, ("trot",), 12, seed=31)) under constant pushes F = (0,0) / (5,0) / (10,5) /
             (15,-10) N, plus 1 N m of yaw torque on robot 3, for 36 ticks of gaits.rollout_phase_host on the CPU checker: not told,
             told the true push through DisturbedEngine, and under compensated_rollout at piece = 1 with the default observer.
  shift      random QPs of mpcqp.synth.config3 with wrench rows of up to 20 N and 3 N m.
  track      the fixture's truth logs tiled to B robots and cut to T rows.

and two recorded numbers in tests/golden/disturbance_fixture.npz (`python tests/disturbance_cases.py` regenerates it; the project's own
host code produces both):
  tau_err    the worst error of the observer's torque residual against the push's torque on the fixture's live rows, with the lever
             arms at the midpoint of the two CoMs (the rule).  The force residual is exact to rounding; the torque residual is not,
             because the arms move during the tick.
  growth     the worst change of an observer output over the fixture's 36 rows, relative to max(1, |output|), under perturbations of
             1e-10 of the start state and of every operand, divided by 1e-10 (estimate_cases.measure_growth's definition).
The band is the project's (estimate_cases.error): fp64 I/O 1e-9 relative, fp32 I/O two float32 spacings against the host rounded once."""
import functools
import os

import numpy as np

from conftest import ORACLE_SO                                                  # noqa: F401  (first: it puts the repository on the path)
import mpcqp
from estimate_cases import error, r32                                           # noqa: F401  (the band, shared with the GPU tests)
from mpcqp import disturbance, gaits

FIXTURE_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disturbance_fixture.npz")
B_FIX, T_FIX, DELTA, N_FIX = 4, 36, 0.03, 10
PUSH = np.array([[0.0, 0.0, 0, 0, 0, 0], [5.0, 0.0, 0, 0, 0, 0], [10.0, 5.0, 0, 0, 0, 0], [15.0, -10.0, 0, 0, 0, 1.0]])
PUSH_TICKS = np.tile(np.array([[0, 1 << 20]], np.int32), (B_FIX, 1))
CHECKER = dict(N=N_FIX, delta=DELTA, max_iter=4000)


def checker(**kw):
    lib = mpcqp.Library(ORACLE_SO)
    return mpcqp.Engine(lib, lib.default_config(**{**CHECKER, **kw}))


def fixture_batch():
    return gaits.make_phase_batch(B_FIX, ("trot",), 12, seed=31)


def _roll(eng, pb, st, n):
    """n ticks of rollout_phase_host from the carried state st (x, ref, feet, tick), which is advanced."""
    o = gaits.rollout_phase_host(eng, st["x"], st["ref"], st["feet"], pb["gait"], pb["stand"], pb["gain"], st["tick"], pb["mu"], n,
                                 push=PUSH, push_ticks=PUSH_TICKS)
    st.update({k: o[k] for k in ("x", "ref", "feet", "tick")})
    return o


@functools.lru_cache(maxsize=None)
def fixture_run(kind, T=T_FIX, piece=1):
    """The fixture's closed loop: kind "untold" (no table), "told" (the true push as the table) or "observer" (compensated_rollout at
    `piece` with the default observer on the truth logs).  Returns the logs of the T ticks (and "dist", "resid", "state" for the observer)."""
    pb = fixture_batch()
    st = {k: pb[k].copy() for k in ("x", "ref", "feet", "tick")}
    eng = disturbance.DisturbedEngine(checker(), PUSH if kind == "told" else None)
    if kind != "observer":
        return _roll(eng, pb, st, T)
    out = disturbance.compensated_rollout(lambda n: _roll(eng, pb, st, n), T, piece,
                                          lambda logs, state: disturbance.disturbance_track_host(logs, eng.cfg, state=state), eng.set_rows)
    return {**out["logs"], "x": st["x"], "dist": out["dist"], "resid": out["resid"], "state": out["state"]}


def final_xy_error(run):
    """|CoM xy - reference xy| of every robot on the last logged row."""
    return np.linalg.norm(run["actual"][:, -1, 3:5] - run["desired"][:, -1, 3:5], axis=1)


def truth_logs():
    run = fixture_run("untold")
    return {k: run[k] for k in ("actual", "forces", "feet_log")}


def track_case(B, T):
    """The fixture's truth logs tiled to B robots (robot b is fixture robot b mod 4) and cut to T rows."""
    logs = truth_logs()
    idx = np.arange(B) % B_FIX
    return {k: np.ascontiguousarray(v[idx, :T]) for k, v in logs.items()}


def as_io(logs, io):
    return logs if io == "f64" else {k: r32(v) for k, v in logs.items()}


@functools.lru_cache(maxsize=None)
def host_track(B, T, io):
    return disturbance.disturbance_track_host(as_io(track_case(B, T), io), checker().cfg)


POISON_B, POISON_T = 6, 12


def poison_case():
    """Six robots over 12 rows of the fixture's logs: robot 0 a NaN foot on a swing leg (not read: clean), robot 1 a NaN in row 5 of
    `actual`, robot 2 an infinite force in row 3, robot 3 a NaN foot on a stance leg, robot 4 an invalid body row, robot 5 clean.
    Returns (logs, body, the first poisoned row of each robot or None)."""
    logs = {k: v.copy() for k, v in track_case(POISON_B, POISON_T).items()}
    sw = np.argwhere((logs["forces"][0].reshape(POISON_T, 4, 3) == 0).all(axis=2))
    assert len(sw) > 0                                                          # the trot has swing legs
    t_sw, l_sw = sw[len(sw) // 2]
    logs["feet_log"][0, t_sw, l_sw] = np.nan
    logs["actual"][1, 5, 7] = np.nan
    logs["forces"][2, 3, 4] = np.inf
    st_t, st_l = np.argwhere((logs["forces"][3].reshape(POISON_T, 4, 3) != 0).any(axis=2))[7]
    logs["feet_log"][3, st_t, st_l, 1] = np.nan
    cfg = checker().cfg
    body = mpcqp.plant.model_body(cfg.m, list(cfg.Ibody_inv), POISON_B)
    body[4, 0] = -1.0
    return logs, body, {0: None, 1: 5, 2: 3, 3: int(st_t), 4: 0, 5: None}


def measure_tau_err():
    out = disturbance.disturbance_track_host(truth_logs(), checker().cfg)
    return float(np.abs(out["resid"][:, 1:, 3:6] - PUSH[:, None, 3:6]).max())


def measure_growth(eps=1e-10, seed=11):
    logs, cfg = truth_logs(), checker().cfg
    rng = np.random.default_rng(seed)
    pert = {k: v + eps * rng.choice([-1.0, 1.0], v.shape) for k, v in logs.items()}
    st, stp = np.zeros((B_FIX, disturbance.STATE)), np.zeros((B_FIX, disturbance.STATE))
    stp[:, :6] = eps                                                            # (a fresh start: d^ is all of the state that is read)
    a, b = disturbance.disturbance_track_host(logs, cfg, state=st), disturbance.disturbance_track_host(pert, cfg, state=stp)
    return max(float((np.abs(a[k] - b[k]) / np.maximum(1.0, np.abs(a[k]))).max()) for k in disturbance.OUT) / eps


def recorded():
    z = np.load(FIXTURE_NPZ)
    return float(z["tau_err"]), float(z["growth"])


def shift_case(B, N=10, seed=0, models=False):
    """x0, xdes of a synthetic batch (their yaw is uniform in [-pi, pi]), wrench rows of up to 20 N and 3 N m and, with `models`,
    model rows that differ per robot."""
    b = mpcqp.synth.make_batch(B, N=N, delta=DELTA, seed=20251021 + seed, gait_names=("trot", "pronk", "amble", "gallop"), mus=(0.3, 0.5, 0.7, 1.0))
    rng = np.random.default_rng(977 + B + N + seed)
    rows = np.concatenate([rng.uniform(-20.0, 20.0, (B, 3)), rng.uniform(-3.0, 3.0, (B, 3))], axis=1)
    mod = None
    if models:
        mod = np.stack([rng.uniform(7.0, 14.0, B), rng.uniform(0.15, 0.4, B), rng.uniform(0.7, 1.5, B), rng.uniform(0.7, 1.5, B),
                        np.full(B, 3.0), np.full(B, 100.0)], axis=1)
    return b, rows, mod


if __name__ == "__main__":                                                      # regenerate tests/golden/disturbance_fixture.npz
    tau, g = measure_tau_err(), measure_growth()
    np.savez(FIXTURE_NPZ, tau_err=np.float64(tau), growth=np.float64(g), eps=np.float64(1e-10))
    print("worst torque residual error on the fixture [N m]", tau, " growth over its 36 rows", g)
