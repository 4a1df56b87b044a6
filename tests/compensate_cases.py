"""Cases shared by tests/test_compensate_host.py and tests/test_gpu_compensate.py (include/mpcqp_compensate.h,
mpcqp_rollout_observe_compensated): the pushed trot robots of tests/disturbance_cases.py with what the leg roll-out of
tests/observe_cases.py needs besides (a leg state, step heights, a ground that never limits, the feet's mass, height rows and an exact
est_init), tiled to B robots, and the host runs of that fixture, each made once."""
import functools

import numpy as np

import disturbance_cases as C
import observe_cases as oc
import mpcqp
from mpcqp import disturbance, gaits, lite3_model

T_FIX, PAYLOAD = 12, 2.0
STATE = ("x", "ref", "feet", "legs", "tick", "slip", "est_state")


def batch(B=C.B_FIX):
    """Robot b is fixture robot b mod 4: its state, its push over the whole run, the plant's body with PAYLOAD kg nobody is told of."""
    pb, idx = C.fixture_batch(), np.arange(B) % C.B_FIX
    pb = {k: np.ascontiguousarray(v[idx]) for k, v in pb.items()}
    cfg = C.checker().cfg
    pb["legs"] = np.zeros((B, 4, 7))
    pb["step_height"] = np.full(B, 0.06)
    pb["ground"] = np.full(B, 1e3)
    pb["foot_mass"] = np.full(B, lite3_model.foot_mass())
    pb["height"] = pb["stand"][:, :, 2].copy()
    pb["est_init"] = pb["x"][:, :12].copy()
    pb["push"], pb["push_ticks"] = C.PUSH[idx].copy(), C.PUSH_TICKS[idx].copy()
    pb["model_body"] = mpcqp.plant.model_body(cfg.m, list(cfg.Ibody_inv), B)
    pb["heavy_body"] = pb["model_body"].copy()
    pb["heavy_body"][:, 0] += PAYLOAD
    return pb


def host_args(pb):
    return (pb["x"], pb["ref"], pb["feet"], pb["legs"], pb["gait"], pb["stand"], pb["gain"], pb["tick"], pb["mu"])


def host_kw(pb, heavy=False, feed="truth"):
    return dict(feed=feed, est_init=pb["est_init"], height=pb["height"], push=pb["push"], push_ticks=pb["push_ticks"],
                body=pb["heavy_body"] if heavy else None)


@functools.lru_cache(maxsize=None)
def host_run(source="truth", hold=1, T=T_FIX, kappa=0.2, heavy=False, feed="truth"):
    """rollout_compensated_host on the four fixture robots."""
    pb = batch()
    return disturbance.rollout_compensated_host(C.checker(), *host_args(pb), T, pb["step_height"], pb["ground"], pb["foot_mass"],
                                                compensate={"source": source, "hold": hold, "kappa": kappa}, **host_kw(pb, heavy, feed))


@functools.lru_cache(maxsize=None)
def host_observe(T=T_FIX, rows=None, feed="truth"):
    """gaits.rollout_observe_host on the four fixture robots: under no table (rows = None) or under zero rows ("zero")."""
    pb = batch()
    eng = disturbance.DisturbedEngine(C.checker(), None if rows is None else disturbance.wrench_rows(C.B_FIX))
    return gaits.rollout_observe_host(eng, *host_args(pb), T, pb["step_height"], pb["ground"], pb["foot_mass"], **host_kw(pb, False, feed))


FIXTURE_NPZ = C.os.path.join(C.os.path.dirname(C.os.path.abspath(__file__)), "golden", "compensate_fixture.npz")
SENSED_T = 24


def sensed_figures():
    """On ground 1e3 without noise and with an exact est_init, 24 ticks at hold = 1, feed "truth": the sensed observer's force estimate
    against the truth observer's of the same robots -> (the worst difference [N], the worst error of the estimator's velocity [m/s],
    the worst difference between commanded and applied forces [N])."""
    s, t = host_run("sensed", 1, SENSED_T), host_run("truth", 1, SENSED_T)
    return (float(np.abs(s["dist"][..., :3] - t["dist"][..., :3]).max()), float(np.abs(s["est"][..., 9:12] - s["actual"][..., 9:12]).max()),
            float(np.abs(s["cmd"] - s["forces"]).max()))


def recorded():
    return float(np.load(FIXTURE_NPZ)["sensed_force_err"])


if __name__ == "__main__":                                                      # regenerate tests/golden/compensate_fixture.npz
    err, ev, df = sensed_figures()
    np.savez(FIXTURE_NPZ, sensed_force_err=np.float64(err), est_v_err=np.float64(ev), cmd_err=np.float64(df))
    print("sensed against truth estimate [N]", err, " estimator velocity error [m/s]", ev, " commanded against applied [N]", df)
