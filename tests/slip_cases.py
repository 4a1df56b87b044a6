"""Cases shared by tests/test_slip_host.py and tests/test_gpu_slip.py (include/mpcqp_slip.h, mpcqp_stance_slip / mpcqp_rollout_slip):
the draw of the rule's comparison -- drive_cases.clamp_draw() with a foot-velocity draw and a foot mass per robot --, the bands of the
slip state and the displacement, and the closed-loop runs."""
import numpy as np

import drive_cases as dc
from legsim_cases import DELTA
from mpcqp import gaits, lite3_model

SLIP_SEED = 5                      # the draw of s0 and foot_mass; chosen so that the margin share holds in both I/O roundings
S_MAX = 1.0                        # a moving foot's speed is at most this [m/s]
MASS_LO, MASS_HI = 0.15, 0.6       # the foot mass per robot [kg]
SLIDING = 128
BITS = dc.BITS | SLIDING           # what the rule adds to a stance row's flag
ICE = 0.3                          # the slippery ground of the loop tests


def slip_draw(seed=SLIP_SEED):
    """drive_cases.clamp_draw() -- 33 robots, ground 0.3 under the even ones and 1e3 under the odd ones -- plus "slip" [33,4,2]: a third
    of the stance feet moving at up to S_MAX in a random direction, every other foot at rest, and "foot_mass" [33] in [MASS_LO, MASS_HI]."""
    c = dc.clamp_draw()
    B = c["x"].shape[0]
    rng = np.random.default_rng(seed)
    moving = (rng.uniform(size=(B, 4)) < 1.0 / 3.0) & (c["contact"] != 0)
    ang, speed = rng.uniform(0.0, 2.0 * np.pi, (B, 4)), rng.uniform(0.0, S_MAX, (B, 4))
    c["slip"] = np.where(moving[..., None], np.stack([speed * np.cos(ang), speed * np.sin(ang)], axis=-1), 0.0)
    c["foot_mass"] = rng.uniform(MASS_LO, MASS_HI, B)
    return c


def as_io(case, dtype):
    """The operands as the I/O dtype holds them, back in float64 (the slip state is fp64 whatever the I/O dtype)."""
    out = dc.as_io({k: v for k, v in case.items() if k != "slip"}, dtype)
    out["slip"] = case["slip"]
    return out


def slip(case, **kw):
    kw.setdefault("delta", DELTA)
    return lite3_model.stance_slip_host(case["x"], case["f"], case["feet"], case["contact"], case["ground"], case["foot_mass"], case["slip"],
                                        **kw)


def force_band(dtype, f_out, f_in):
    """band_f per leg: drive_cases.band at the leg's largest force component, commanded or applied (floor 2^-20), [n,4].  The commanded
    force counts because it is f1, not the applied force, that drives the foot: on a pull the applied force is 0 and the foot coasts
    under the whole of f1."""
    top = lambda f: np.nanmax(np.abs(np.where(np.isfinite(f), f, 0.0)), axis=-1)
    return dc.band(dtype, np.maximum(np.maximum(top(f_out), top(f_in)), 2.0 ** -20))


def state_bands(dtype, f_out, f_in, foot_mass, delta=DELTA):
    """(band of s, band of d) per leg: band_f delta / m_e and band_f delta^2 / m_e, the rule's own gain from a force to the velocity
    and to the displacement at the end of the tick.  f_out, f_in [n,4,3], foot_mass [n]."""
    bf = force_band(dtype, f_out, f_in)
    me = np.asarray(foot_mass, dtype=np.float64)[:, None]
    return bf * delta / me, bf * delta * delta / me


def run_slip(engine, pb, ground, T=dc.LOOP_T, foot_mass=None, **kw):
    """gaits.rollout_slip_host on a batch as drive_cases.loop_batch returns it."""
    a = [pb[k] for k in ("x", "ref", "feet", "legs", "gait", "stand", "gain", "tick", "mu")]
    B = pb["x"].shape[0]
    me = lite3_model.foot_mass() if foot_mass is None else foot_mass
    return gaits.rollout_slip_host(engine, *a, T, pb["step_height"], np.broadcast_to(np.asarray(ground, dtype=np.float64), (B,)).copy(), me, **kw)


def foot_move_holds(feet_log, contact_log, disp, gait, tick0, cast=lambda a: a):
    """The foot-move identity on a roll-out's logs (numpy; float64 or the float32 of the logs): between the rows t and t + 1 a leg in
    stance on row t that does not touch down on row t + 1 has feet_log[t + 1].xy == cast(feet_log[t].xy + disp[t]); every other leg
    that does not touch down keeps its foot and has disp[t] == 0; z changes at touchdowns only."""
    B, T = contact_log.shape[:2]
    ok = True
    for t in range(T - 1):
        td = gaits.touchdown_mask(gait, np.asarray(tick0) + t + 1)
        move = (contact_log[:, t] != 0) & ~td
        a, b = feet_log[:, t], feet_log[:, t + 1]
        want = cast(a[..., :2].astype(np.float64) + disp[:, t].astype(np.float64))
        ok &= np.array_equal(b[..., :2][move], want[move])
        rest = ~move & ~td
        ok &= np.array_equal(b[rest], a[rest]) and not disp[:, t][~move].any()
        ok &= np.array_equal(b[..., 2][~td], a[..., 2][~td])
    return bool(ok)
