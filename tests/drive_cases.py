"""Cases shared by tests/test_stance_drive_host.py and tests/test_gpu_stance_drive.py (include/mpcqp_sim.h, mpcqp_stance_drive /
mpcqp_rollout_drive): the clamp draw on the joint box of tests/legsim_cases.py, the closed-loop batch of the eight named gaits and the
bands of the comparisons."""
import numpy as np

import legsim_cases
from mpcqp import gaits, lite3_model

CLAMP_SEED = 17
F_MAX = 150.0                      # the draw keeps |f| <= 150 N
GROUND_MU = 0.3                    # the slippery ground of the ground cases
LOOP_B, LOOP_T, LOOP_PERIOD, LOOP_SEED = 8, 36, 12, 6
BITS = 2 | 16 | 32                 # what the rule adds to a stance row's flag
# The band of tests/test_gpu_joint_rates.py for the same J and the same cofactor solve on the same joint box
F64_BAND, F32_SPACINGS = 1e-9, 2.0
MARGIN_SHARE = 0.02                # at most this share of the legs may sit within FLAG_MARGIN of a deciding threshold


def clamp_draw(seed=CLAMP_SEED, ground=True, dq=0.0):
    """33 robots (132 legs, not a full block) whose legs stand on `legsim_cases.box_rows()` joints: random torso rotations (robot 0:
    |theta| < 1e-6), feet from the forward kinematics, forces of at most F_MAX scaled so that roughly half the stance legs exceed the
    Lite3's tau_max, a fifth of the legs in swing, a tenth of the legs pulling (f_z < 0), and -- with `ground` -- GROUND_MU under the
    even robots and a ground that never limits (mu_g = 1e3) under the odd ones.  `dq` moves every joint angle the feet are made from
    (the forces stay): the host's own sensitivity to its operands.  Returns the operands of stance_drive_host."""
    from scipy.spatial.transform import Rotation
    q, _ = legsim_cases.box_rows()
    B = q.shape[0]
    rng = np.random.default_rng(seed)
    rv = rng.normal(0.0, 0.15, (B, 3))
    rv[0] = rv[0] / np.linalg.norm(rv[0]) * 5e-7
    R = Rotation.from_rotvec(rv).as_matrix()
    x = np.zeros((B, 13))
    x[:, 0:3] = rv
    x[:, 3:6] = np.array([0.0, 0.0, 0.3]) + rng.normal(0.0, 0.05, (B, 3))
    x[:, 6:12] = rng.normal(0.0, 0.1, (B, 6))
    x[:, 12] = -9.81
    feet = np.zeros((B, 4, 3))
    for b in range(B):
        for l in range(4):
            feet[b, l] = x[b, 3:6] + R[b] @ lite3_model.leg_fk_jac(l, q[b, l])[0]
    f = np.concatenate([rng.normal(0.0, 0.6, (B, 4, 2)), rng.uniform(0.3, 1.0, (B, 4, 1))], axis=-1)
    f[..., 2] = np.where(rng.uniform(size=(B, 4)) < 0.1, -f[..., 2], f[..., 2])
    f = f / np.linalg.norm(f, axis=-1, keepdims=True) * rng.uniform(0.7, 1.0, (B, 4, 1))      # inside the unit ball ...
    contact = (rng.uniform(size=(B, 4)) >= 0.2).astype(np.uint8)
    # ... and scaled so that the median stance leg sits at its torque limit, but never beyond F_MAX
    tau1 = lite3_model.joint_log_host(x[:, None, :12], f.reshape(B, 1, 12), feet[:, None])[1][:, 0]
    use = np.abs(tau1) / lite3_model.leg_inertia()["tau_max"]
    scale = min(F_MAX, 1.0 / np.median(use.max(axis=-1)[contact != 0]))
    f = f * scale
    if dq:
        for b in range(B):
            for l in range(4):
                feet[b, l] = x[b, 3:6] + R[b] @ lite3_model.leg_fk_jac(l, q[b, l] + dq)[0]
    mu_g = np.where(np.arange(B) % 2 == 0, GROUND_MU, 1e3) if ground else None
    return {"x": x, "f": f.reshape(B, 12), "feet": feet, "contact": contact, "ground": mu_g, "scale": scale}


def as_io(case, dtype):
    """The operands as the I/O dtype holds them, back in float64: what the host is fed next to a device run in that dtype."""
    return {k: (v if v is None or k in ("contact", "scale") else np.asarray(v, dtype=dtype).astype(np.float64)) for k, v in case.items()}


def drive(case, **kw):
    return lite3_model.stance_drive_host(case["x"], case["f"], case["feet"], case["contact"], case["ground"], **kw)


def near_threshold(host):
    """True where a stance leg of the host's result came within legsim_cases.FLAG_MARGIN of a threshold that decides a bit or a branch:
    there device and host may differ.  A condition of the comparison, held to MARGIN_SHARE on the CPU."""
    return (host["margin"] <= legsim_cases.FLAG_MARGIN) & (host["flag"] != 0xff)


def band(dtype, ref):
    """The comparison band at the reference values `ref`: F64_BAND absolute in fp64, F32_SPACINGS float32 spacings in fp32."""
    if np.dtype(dtype) == np.float64:
        return np.full(np.shape(ref), F64_BAND)
    return F32_SPACINGS * np.spacing(np.abs(np.asarray(ref, dtype=np.float32))).astype(np.float64)


def loop_batch():
    """The closed-loop case of the issue's prototype: the eight named gaits at period 12, seed 6, with a leg state and step heights."""
    pb = gaits.make_phase_batch(LOOP_B, tuple(gaits.GAITS), LOOP_PERIOD, seed=LOOP_SEED)
    pb["legs"] = np.zeros((LOOP_B, 4, 7))
    pb["step_height"] = np.full(LOOP_B, legsim_cases.STEP_HEIGHT)
    pb["names"] = [tuple(gaits.GAITS)[b % len(gaits.GAITS)] for b in range(LOOP_B)]
    return pb


def weak_row(factor):
    """The Lite3's inertia row with tau_max scaled."""
    row = lite3_model.leg_inertia()
    row["tau_max"] = row["tau_max"] * factor
    return row


def run_loop(engine, pb, T=LOOP_T, **kw):
    """gaits.rollout_drive_host (or, with drive=None, rollout_legs_host) on a batch as loop_batch returns it."""
    a = [pb[k] for k in ("x", "ref", "feet", "legs", "gait", "stand", "gain", "tick", "mu")]
    if kw.get("drive", "limited") is None:
        kw.pop("drive")
        kw.pop("ground", None)
        return gaits.rollout_legs_host(engine, *a, T, pb["step_height"], **kw)
    return gaits.rollout_drive_host(engine, *a, T, pb["step_height"], **kw)
