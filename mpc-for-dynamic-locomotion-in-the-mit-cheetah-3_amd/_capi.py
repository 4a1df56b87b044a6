"""ctypes binding of the C-ABI declared in include/mpcqp.h and its product-only extensions include/mpcqp_plan.h, mpcqp_sim.h, mpcqp_model.h,
mpcqp_joints.h, mpcqp_actuators.h, mpcqp_slip.h, mpcqp_estimate.h, mpcqp_observe.h, mpcqp_gate.h, mpcqp_attitude.h, mpcqp_disturb.h and
mpcqp_compensate.h.

The product path loads ``csrc/libmpcqp.so`` (hand-written HIP for gfx950) and nothing else: if that library is
missing or cannot be loaded, importing the engine raises -- there is no CPU fallback.  The binding itself is
generic over the library path because the CPU checker under ``oracle/`` exports the same symbols with host
pointers; only tests / smoke / bench's cpu_baseline leg ever pass that path in.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_void_p

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(_PKG_DIR, "csrc", "libmpcqp.so")

# include/mpcqp.h constants
STATUS_UNSOLVED, STATUS_SOLVED_POLISHED, STATUS_SOLVED_ADMM, STATUS_MAX_ITER, STATUS_NONFINITE = 0, 1, 2, 3, -1
DISC_EULER, DISC_ZOH = 0, 1
DTYPE_F32, DTYPE_F64 = 0, 1
PREC_F32, PREC_MIXED, PREC_F64 = 0, 1, 2
FLAG_POLISH, FLAG_WARM_START, FLAG_GENERAL_KERNEL, FLAG_NATURAL_ORDER, FLAG_WARM_SHIFT, FLAG_TILE_KERNEL, FLAG_NO_TIMING = 1, 2, 4, 8, 16, 32, 64
FLAG_STAGE_KERNEL = 128
ITERS_WIDE, ITERS_POLISH_MAX = 1000000, 2145


def split_iters(iters):
    """Decode the ``iters`` output (include/mpcqp.h, MPCQP_ITERS) into ``(admm, polish)``: ADMM iterations and polish
    refinement steps.  Values below 1e6 are ``admm + 1000 * polish``; larger ones ``1e6 * (polish + 1) + admm`` (polish
    clamped at 2145).  Takes an int or an integer array / tensor (any shape); returns ints or numpy arrays."""
    if hasattr(iters, "cpu"):   # torch tensor (any device)
        iters = iters.cpu().numpy()
    if isinstance(iters, (int, np.integer)):
        v = int(iters)
        return (v % 1000, v // 1000) if v < ITERS_WIDE else (v % ITERS_WIDE, v // ITERS_WIDE - 1)
    v = np.asarray(iters).astype(np.int64)
    wide = v >= ITERS_WIDE
    admm = np.where(wide, v % ITERS_WIDE, v % 1000)
    polish = np.where(wide, v // ITERS_WIDE - 1, v // 1000)
    return admm, polish

class MpcQpLegGeometry(ctypes.Structure):
    """Mirror of struct MpcQpLegGeometry (include/mpcqp.h)."""
    _fields_ = [("size", c_uint32), ("reserved", c_uint32), ("hip_x", c_double * 3 * 4), ("hip_y", c_double * 3 * 4),
                ("knee", c_double * 3), ("foot", c_double * 3), ("axis_x", c_double * 3), ("axis_y", c_double * 3)]


class MpcQpLegInertia(ctypes.Structure):
    """Mirror of struct MpcQpLegInertia (include/mpcqp_joints.h)."""
    _fields_ = [("size", c_uint32), ("reserved", c_uint32), ("mass", c_double * 3 * 4), ("com", c_double * 3 * 3 * 4),
                ("inertia", c_double * 6 * 3 * 4), ("q_min", c_double * 3), ("q_max", c_double * 3), ("qd_max", c_double * 3),
                ("tau_max", c_double * 3), ("gravity", c_double)]
    ARRAYS = ("mass", "com", "inertia", "q_min", "q_max", "qd_max", "tau_max")

    @classmethod
    def from_dict(cls, d):
        """The struct of a dict of arrays as lite3_model.leg_inertia() returns it (no check: the library checks the row)."""
        r = cls()
        r.size = ctypes.sizeof(cls)
        for k in cls.ARRAYS:
            a = np.ascontiguousarray(d[k], dtype=np.float64)
            field = getattr(r, k)
            if a.nbytes != ctypes.sizeof(field):
                raise ValueError(f"leg inertia field {k}: expected {ctypes.sizeof(field) // 8} values, got {a.size}")
            ctypes.memmove(field, a.ctypes.data, a.nbytes)
        r.gravity = float(d["gravity"])
        return r

    def as_dict(self):
        out = {k: np.ctypeslib.as_array(getattr(self, k)).copy() for k in self.ARRAYS}
        out["gravity"] = float(self.gravity)
        return out


class MpcQpScoreRule(ctypes.Structure):
    """Mirror of struct MpcQpScoreRule (include/mpcqp_sim.h): when a log row counts as fallen."""
    _fields_ = [("size", c_uint32), ("z_frac", c_double), ("tilt_max", c_double)]


class MpcQpEstimator(ctypes.Structure):
    """Mirror of struct MpcQpEstimator (include/mpcqp_estimate.h): the state estimator's gains and noise figures."""
    _fields_ = [("size", c_uint32), ("gravity", c_double), ("kappa", c_double), ("q_p", c_double), ("q_v", c_double), ("q_f", c_double),
                ("r_p", c_double), ("r_v", c_double), ("r_z", c_double), ("k_swing", c_double), ("p0_p", c_double), ("p0_v", c_double),
                ("p0_f", c_double)]
    FIELDS = tuple(name for name, _ in _fields_[1:])


class MpcQpTrustGate(ctypes.Structure):
    """Mirror of struct MpcQpTrustGate (include/mpcqp_gate.h): the thresholds of the estimator's per-leg trust gate."""
    _fields_ = [("size", c_uint32), ("d_lo", c_double), ("d_hi", c_double)]
    FIELDS = tuple(name for name, _ in _fields_[1:])


class MpcQpAttitude(ctypes.Structure):
    """Mirror of struct MpcQpAttitude (include/mpcqp_attitude.h): the gains of the estimator's velocity-aided attitude rule."""
    _fields_ = [("size", c_uint32), ("k_s", c_double), ("k_v", c_double), ("k_b", c_double), ("b_max", c_double)]
    FIELDS = tuple(name for name, _ in _fields_[1:])


class MpcQpWrenchObserver(ctypes.Structure):
    """Mirror of struct MpcQpWrenchObserver (include/mpcqp_disturb.h): the wrench observer's gravity, gain and clamps."""
    _fields_ = [("size", c_uint32), ("gravity", c_double), ("kappa", c_double), ("f_lim", c_double), ("t_lim", c_double)]
    FIELDS = tuple(name for name, _ in _fields_[1:])


class MpcQpCompensate(ctypes.Structure):
    """Mirror of struct MpcQpCompensate (include/mpcqp_compensate.h): the estimator variant, the observer's source, the ticks between
    two table updates and the observer's parameters."""
    _fields_ = [("size", c_uint32), ("flags", c_uint32), ("source", c_int32), ("hold", c_int32), ("observer", MpcQpWrenchObserver)]


class MpcQpConfig(ctypes.Structure):
    """Mirror of ``struct MpcQpConfig`` (include/mpcqp.h)."""
    _fields_ = [
        ("size", c_uint32), ("N", c_int32), ("delta", c_double), ("m", c_double),
        ("Ibody_inv", c_double * 3), ("w", c_double * 13), ("alpha", c_double),
        ("f_min", c_double), ("f_max", c_double), ("disc", c_int32), ("dtype", c_int32),
        ("precision", c_int32), ("flags", c_uint32), ("rho", c_double), ("sigma", c_double),
        ("relax", c_double), ("max_iter", c_int32), ("check_every", c_int32),
        ("eps_abs", c_double), ("eps_rel", c_double), ("polish_max", c_int32), ("device", c_int32),
        ("first_block", c_int32), ("incr_legs", c_int32), ("listed_max", c_int32), ("adapt_thr", c_float), ("alpha_floor", c_double),
        ("polish_patience", c_int32), ("polish_cheap_steps", c_int32), ("polish_cheap_legs", c_int32), ("hard_block_x10", c_int32), ("polish_last_patience", c_int32), ("accel", c_int32), ("accel_restart", c_int32), ("reserved0", c_int32),
    ]

    def as_dict(self):
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
        return out


class MpcQpError(RuntimeError):
    pass


# The C-ABI, one row per function: (name, return type, parameter types), by the header that declares it.  include/mpcqp.h is required;
# the other four are exported by the product library only (the CPU checker under oracle/ does not have them).  tests/test_capi.py
# compares every row with the prototype in the header.
_P, _I32, _I64 = c_void_p, c_int32, c_int64   # any address (handle, buffer, stream), int32_t, int64_t
_CFG, _GEO, _INR = ctypes.POINTER(MpcQpConfig), ctypes.POINTER(MpcQpLegGeometry), ctypes.POINTER(MpcQpLegInertia)
_RULE = ctypes.POINTER(MpcQpScoreRule)
_EST = ctypes.POINTER(MpcQpEstimator)
_GATE = ctypes.POINTER(MpcQpTrustGate)
_ATT = ctypes.POINTER(MpcQpAttitude)
CORE_HEADER = "mpcqp.h"
ABI = {
    "mpcqp.h": (
        ("mpcqp_version", c_uint32, ()),
        ("mpcqp_default_config", c_int, (_CFG,)),
        ("mpcqp_create", c_int, (_CFG, ctypes.POINTER(c_void_p))),
        ("mpcqp_destroy", c_int, (_P,)),
        ("mpcqp_reserve", c_int, (_P, _I64)),
        ("mpcqp_solve_batch", c_int, (_P, _I64) + (_P,) * 11),
        ("mpcqp_solve_batch_gait", c_int, (_P, _I64) + (_P,) * 13),
        ("mpcqp_solve_batch_gait_steps", c_int, (_P, _I64, _I32) + (_P,) * 13),
        ("mpcqp_rollout", c_int, (_P, _I64, _I32, _I32) + (_P,) * 12),
        ("mpcqp_torque_map", c_int, (_P, _I64, _P, _P, _P, _P)),
        ("mpcqp_default_leg_geometry", c_int, (_GEO,)),
        ("mpcqp_leg_jacobians", c_int, (_P, _I64, _P, _P, _GEO, _P, _P, _P)),
        ("mpcqp_last_kernel_ms", c_int, (_P, ctypes.POINTER(c_float))),
        ("mpcqp_last_error", c_char_p, (_P,)),
    ),
    "mpcqp_plan.h": (   # footstep plans, swing-foot trajectories and per-leg periodic gaits
        ("mpcqp_plan_footsteps", c_int, (_P, _I64, _I32) + (_P,) * 9),
        ("mpcqp_swing_trajectories", c_int, (_P, _I64, _I32, _I32) + (_P,) * 9),
        ("mpcqp_phase_expand", c_int, (_P, _I64) + (_P,) * 11),
        ("mpcqp_solve_batch_phase", c_int, (_P, _I64) + (_P,) * 14),
        ("mpcqp_phase_swing", c_int, (_P, _I64, _I32) + (_P,) * 11),
    ),
    "mpcqp_sim.h": (    # the rigid-body plant
        ("mpcqp_plant_step", c_int, (_P, _I64) + (_P,) * 6 + (_I32, _P, _P)),
        ("mpcqp_rollout_plant", c_int, (_P, _I64, _I32, _I32) + (_P,) * 10 + (_I32,) + (_P,) * 5),
        ("mpcqp_rollout_phase", c_int, (_P, _I64, _I32) + (_P,) * 11 + (_I32,) + (_P,) * 7),
        ("mpcqp_rollout_legs", c_int, (_P, _I64, _I32) + (_P,) * 12 + (_I32, _P, _P, _I32, _GEO, _INR, _I32) + (_P,) * 15),
        ("mpcqp_rollout_score", c_int, (_P, _I64, _I32) + (_P,) * 8 + (_RULE, _I32, _P, _P)),
        ("mpcqp_stance_drive", c_int, (_P, _I64) + (_P,) * 5 + (_GEO, _INR) + (_P,) * 4),
        ("mpcqp_rollout_drive", c_int, (_P, _I64, _I32) + (_P,) * 12 + (_I32, _P, _P, _I32, _GEO, _INR, _I32, _I32, _P) + (_P,) * 16),
    ),
    "mpcqp_model.h": (  # per-robot model rows
        ("mpcqp_set_models", c_int, (_P, _I64, _P, _P)),
        ("mpcqp_clear_models", c_int, (_P,)),
    ),
    "mpcqp_joints.h": (  # closed-form leg inverse kinematics, the joint-space log and the leg dynamics
        ("mpcqp_leg_ik", c_int, (_P, _I64, _P, _P, _P, _GEO, _P, _P, _P)),
        ("mpcqp_joint_log", c_int, (_P, _I64, _I32, _P, _P, _P, _GEO, _P, _P, _P, _P)),
        ("mpcqp_joint_rates", c_int, (_P, _I64, _I32, _P, _P, _P, _P, _GEO) + (_P,) * 6),
        ("mpcqp_default_leg_inertia", c_int, (_INR,)),
        ("mpcqp_leg_dynamics", c_int, (_P, _I64) + (_P,) * 5 + (_GEO, _INR) + (_P,) * 4),
        ("mpcqp_leg_effort", c_int, (_P, _I64, _I32) + (_P,) * 7 + (_GEO, _INR) + (_P,) * 6),
        ("mpcqp_leg_accel", c_int, (_P, _I64) + (_P,) * 5 + (_GEO, _INR) + (_P,) * 3),
        ("mpcqp_swing_track", c_int, (_P, _I64, _I32) + (_P,) * 9 + (_I32, _GEO, _INR) + (_P,) * 7),
    ),
}
EXPORTED_SYMBOLS, PLAN_SYMBOLS, SIM_SYMBOLS, MODEL_SYMBOLS, JOINTS_SYMBOLS = (tuple(row[0] for row in rows) for rows in ABI.values())
# include/mpcqp_actuators.h, the newest header, in a table of its own with the same rows: a product library built before it binds the five
# headers above as it always did, and `has_actuators` tells the two apart.
ACTUATORS_HEADER = "mpcqp_actuators.h"
ACTUATORS_ABI = {
    ACTUATORS_HEADER: (  # per-robot actuator rows
        ("mpcqp_set_actuators", c_int, (_P, _I64, _P, _P)),
        ("mpcqp_clear_actuators", c_int, (_P,)),
    ),
}
ACTUATOR_SYMBOLS = tuple(row[0] for row in ACTUATORS_ABI[ACTUATORS_HEADER])
# include/mpcqp_slip.h came after it, again in a table of its own: `has_slip`.
SLIP_HEADER = "mpcqp_slip.h"
SLIP_ABI = {
    SLIP_HEADER: (  # stance feet that slide
        ("mpcqp_stance_slip", c_int, (_P, _I64) + (_P,) * 7 + (_I32, _GEO, _INR) + (_P,) * 6),
        ("mpcqp_rollout_slip", c_int, (_P, _I64, _I32) + (_P,) * 12 + (_I32, _P, _P, _I32, _GEO, _INR, _I32, _I32, _P, _P, _P) + (_P,) * 18),
    ),
}
SLIP_SYMBOLS = tuple(row[0] for row in SLIP_ABI[SLIP_HEADER])
# include/mpcqp_estimate.h, the state estimator, likewise: `has_estimate`.
ESTIMATE_HEADER = "mpcqp_estimate.h"
ESTIMATE_ABI = {
    ESTIMATE_HEADER: (  # the torso state from an IMU and leg kinematics
        ("mpcqp_default_estimator", c_int, (_EST,)),
        ("mpcqp_imu_log", c_int, (_P, _I64, _I32) + (_P,) * 7 + (_EST, _P, _P)),
        ("mpcqp_estimate_track", c_int, (_P, _I64, _I32) + (_P,) * 7 + (_EST, _GEO) + (_P,) * 6),
    ),
}
ESTIMATE_SYMBOLS = tuple(row[0] for row in ESTIMATE_ABI[ESTIMATE_HEADER])
EST_STATE = 131   # include/mpcqp_estimate.h, MPCQP_EST_STATE: doubles per robot of the filter state
# include/mpcqp_observe.h, the slip roll-out with the estimator inside its tick loop, likewise: `has_observe`.
OBSERVE_HEADER = "mpcqp_observe.h"
OBSERVE_ABI = {
    OBSERVE_HEADER: (  # sensors and the state estimator inside the roll-out
        ("mpcqp_rollout_observe", c_int, SLIP_ABI[SLIP_HEADER][1][2][:-1] + (_I32,) + (_P,) * 6 + (_EST,) + (_P,) * 8),
    ),
}
OBSERVE_SYMBOLS = tuple(row[0] for row in OBSERVE_ABI[OBSERVE_HEADER])
FEED_TRUTH, FEED_ESTIMATE = 0, 1   # include/mpcqp_observe.h, MPCQP_FEED_*
# include/mpcqp_gate.h, the estimator's trust gated on the legs' velocity innovations, likewise: `has_gate`.  Each gated call is its
# ungated row with the thresholds and the trust output in front of the stream.
GATE_HEADER = "mpcqp_gate.h"
GATE_ABI = {
    GATE_HEADER: (  # the per-leg trust gate of the estimator, over a log and inside the roll-out
        ("mpcqp_default_trust_gate", c_int, (_GATE,)),
        ("mpcqp_estimate_track_gated", c_int, ESTIMATE_ABI[ESTIMATE_HEADER][2][2][:-1] + (_GATE, _P, _P)),
        ("mpcqp_rollout_observe_gated", c_int, OBSERVE_ABI[OBSERVE_HEADER][0][2][:-1] + (_GATE, _P, _P)),
    ),
}
GATE_SYMBOLS = tuple(row[0] for row in GATE_ABI[GATE_HEADER])
# include/mpcqp_attitude.h, the velocity-aided attitude and gyro-bias states, likewise: `has_attitude`.  Each aided call is its gated
# row with the flags, the gains, att_state and the bias output in front of the stream.
ATTITUDE_HEADER = "mpcqp_attitude.h"
ATTITUDE_ABI = {
    ATTITUDE_HEADER: (  # the aided rule of the estimator, over a log and inside the roll-out
        ("mpcqp_default_attitude", c_int, (_ATT,)),
        ("mpcqp_estimate_track_aided", c_int, GATE_ABI[GATE_HEADER][1][2][:-1] + (_I32, _ATT, _P, _P, _P)),
        ("mpcqp_rollout_observe_aided", c_int, GATE_ABI[GATE_HEADER][2][2][:-1] + (_I32, _ATT, _P, _P, _P)),
    ),
}
ATTITUDE_SYMBOLS = tuple(row[0] for row in ATTITUDE_ABI[ATTITUDE_HEADER])
ATT_STATE = 8     # include/mpcqp_attitude.h, MPCQP_ATT_STATE: doubles per robot of the attitude state
AIDED_GATE = 1    # include/mpcqp_attitude.h, MPCQP_AIDED_GATE
# include/mpcqp_disturb.h, the disturbance wrench rows of the MPC and the wrench observer, likewise: `has_disturb`.  The table calls are
# mpcqp_model.h's rows under their own names.
DISTURB_HEADER = "mpcqp_disturb.h"
_OBS = ctypes.POINTER(MpcQpWrenchObserver)
DISTURB_ABI = {
    DISTURB_HEADER: (  # per-robot disturbance wrench rows and the observer over a roll-out's logs
        ("mpcqp_set_disturbance", c_int, ABI["mpcqp_model.h"][0][2]),
        ("mpcqp_clear_disturbance", c_int, ABI["mpcqp_model.h"][1][2]),
        ("mpcqp_disturbance_shift", c_int, (_P, _I64, _P, _P, _P, _P)),
        ("mpcqp_default_wrench_observer", c_int, (_OBS,)),
        ("mpcqp_disturbance_track", c_int, (_P, _I64, _I32, _P, _P, _P, _P, _OBS, _P, _P, _P, _P)),
    ),
}
DISTURB_SYMBOLS = tuple(row[0] for row in DISTURB_ABI[DISTURB_HEADER])
DIST_STATE = 40   # include/mpcqp_disturb.h, MPCQP_DIST_STATE: doubles per robot of the observer's state
# include/mpcqp_compensate.h, that observer and the table update inside the roll-out's tick loop, likewise: `has_compensate`.  The call is
# the aided roll-out's row with the parameters, the observer's body, its state and its two logs in front of the stream.
COMPENSATE_HEADER = "mpcqp_compensate.h"
_COMP = ctypes.POINTER(MpcQpCompensate)
COMPENSATE_ABI = {
    COMPENSATE_HEADER: (  # the wrench observer inside mpcqp_rollout_observe
        ("mpcqp_default_compensate", c_int, (_COMP,)),
        ("mpcqp_rollout_observe_compensated", c_int, ATTITUDE_ABI[ATTITUDE_HEADER][2][2][:-1] + (_COMP, _P, _P, _P, _P, _P)),
    ),
}
COMPENSATE_SYMBOLS = tuple(row[0] for row in COMPENSATE_ABI[COMPENSATE_HEADER])
WRENCH_TRUTH, WRENCH_SENSED = 0, 1   # include/mpcqp_compensate.h, MPCQP_WRENCH_*
COMP_GATED, COMP_AIDED = 1, 2        # include/mpcqp_compensate.h, MPCQP_COMP_*
# The swing-leg plant of include/mpcqp_joints.h came after the rest of that header: a product library built before it still has the
# header's other calls (`has_joints`) and is told apart by `has_legsim`.
LEGSIM_SYMBOLS = ("mpcqp_leg_accel", "mpcqp_swing_track")
# Likewise the roll-out with the swing legs inside it, which came after the rest of include/mpcqp_sim.h (`has_sim`): `has_legroll`.
LEGROLL_SYMBOLS = ("mpcqp_rollout_legs",)
# ... and the score row of a roll-out's logs, the header's newest call: `has_score`.
SCORE_SYMBOLS = ("mpcqp_rollout_score",)
# ... and the stance drive, the header's newest pair: `has_drive`.
DRIVE_SYMBOLS = ("mpcqp_stance_drive", "mpcqp_rollout_drive")
_GATED = {name: (gate, names) for gate, names in (("has_legsim", LEGSIM_SYMBOLS), ("has_legroll", LEGROLL_SYMBOLS), ("has_score", SCORE_SYMBOLS),
                                                  ("has_drive", DRIVE_SYMBOLS))
          for name in names}
LAND_RULE, LAND_ACTUAL = 0, 1   # include/mpcqp_sim.h, MPCQP_LAND_*
DRIVE_IDEAL, DRIVE_LIMITED = 0, 1   # include/mpcqp_sim.h, MPCQP_DRIVE_*
# The flag bits the stance drive writes (include/mpcqp_sim.h): clamped, q outside its limits, not resolvable, limited by the ground.
DRIVE_CLAMPED, DRIVE_QLIM, DRIVE_UNRESOLVED, DRIVE_GROUND, DRIVE_POISONED = 2, 4, 16, 32, 0xff
DRIVE_SLIDING = 128   # include/mpcqp_slip.h, MPCQP_DRIVE_SLIDING: the stance foot slides


class Library:
    """A loaded shared object exporting the mpcqp C-ABI.  `has_plan`, `has_sim`, `has_model`, `has_joints`, `has_actuators`, `has_slip`,
    `has_estimate`, `has_observe`, `has_gate`, `has_attitude` and `has_disturb` say whether it exports all of include/mpcqp_plan.h, mpcqp_sim.h, mpcqp_model.h,
    mpcqp_joints.h, mpcqp_actuators.h, mpcqp_slip.h, mpcqp_estimate.h, mpcqp_observe.h, mpcqp_gate.h, mpcqp_attitude.h and mpcqp_disturb.h (of mpcqp_joints.h: all but LEGSIM_SYMBOLS, which `has_legsim`
    answers for; of mpcqp_sim.h: all but LEGROLL_SYMBOLS, SCORE_SYMBOLS and DRIVE_SYMBOLS, `has_legroll`, `has_score` and `has_drive`).  An
    extension header's calls are bound only when the library
    has them all; `partial=True` binds whichever it has (an older build of the product library, in a comparison tool)."""

    def __init__(self, path: str, partial: bool = False):
        if not os.path.exists(path):
            raise MpcQpError(f"mpcqp library not found: {path} (run `python -c 'import __graft_entry__ as g; g.build()'`)")
        self.path = path
        self.lib = ctypes.CDLL(path)
        self.calls = {}   # name -> (function or None, its header, which parameters after the handle are addresses): Engine._call
        self.has_legsim = all(hasattr(self.lib, name) for name in LEGSIM_SYMBOLS)
        self.has_legroll = all(hasattr(self.lib, name) for name in LEGROLL_SYMBOLS)
        self.has_score = all(hasattr(self.lib, name) for name in SCORE_SYMBOLS)
        self.has_drive = all(hasattr(self.lib, name) for name in DRIVE_SYMBOLS)
        for header, rows in {**ABI, **ACTUATORS_ABI, **SLIP_ABI, **ESTIMATE_ABI, **OBSERVE_ABI, **GATE_ABI, **ATTITUDE_ABI, **DISTURB_ABI,
                             **COMPENSATE_ABI}.items():
            have = header == CORE_HEADER or all(hasattr(self.lib, row[0]) for row in rows if row[0] not in _GATED)
            if header != CORE_HEADER:
                setattr(self, "has_" + header[len("mpcqp_"):-len(".h")], have)
            for name, restype, argtypes in rows:
                fn = None
                bind = have and (name not in _GATED or getattr(self, _GATED[name][0]))
                if bind or (partial and hasattr(self.lib, name)):   # (a symbol of the core header that is missing raises here)
                    fn = getattr(self.lib, name)
                    fn.restype, fn.argtypes = restype, argtypes
                self.calls[name] = (fn, header, tuple(t not in (_I32, _I64) for t in argtypes[1:]))

    def version(self) -> int:
        return int(self.lib.mpcqp_version())

    def default_leg_inertia(self) -> "MpcQpLegInertia":
        """The Lite3's inertial row and actuator limits (include/mpcqp_joints.h, mpcqp_default_leg_inertia; product library only)."""
        fn, header, _ = self.calls["mpcqp_default_leg_inertia"]
        if fn is None:
            raise MpcQpError(f"mpcqp_default_leg_inertia: {self.path} does not export include/{header} (product library only)")
        row = MpcQpLegInertia()
        rc = fn(ctypes.byref(row))
        if rc != 0:
            raise MpcQpError(f"mpcqp_default_leg_inertia failed: {rc}")
        return row

    def default_estimator(self) -> "MpcQpEstimator":
        """The estimator's default gains and noise figures (include/mpcqp_estimate.h, mpcqp_default_estimator; product library only)."""
        fn, header, _ = self.calls["mpcqp_default_estimator"]
        if fn is None:
            raise MpcQpError(f"mpcqp_default_estimator: {self.path} does not export include/{header} (product library only)")
        row = MpcQpEstimator()
        rc = fn(ctypes.byref(row))
        if rc != 0:
            raise MpcQpError(f"mpcqp_default_estimator failed: {rc}")
        return row

    def default_trust_gate(self) -> "MpcQpTrustGate":
        """The trust gate's default thresholds (include/mpcqp_gate.h, mpcqp_default_trust_gate; product library only)."""
        fn, header, _ = self.calls["mpcqp_default_trust_gate"]
        if fn is None:
            raise MpcQpError(f"mpcqp_default_trust_gate: {self.path} does not export include/{header} (product library only)")
        row = MpcQpTrustGate()
        rc = fn(ctypes.byref(row))
        if rc != 0:
            raise MpcQpError(f"mpcqp_default_trust_gate failed: {rc}")
        return row

    def default_attitude(self) -> "MpcQpAttitude":
        """The aided attitude rule's default gains (include/mpcqp_attitude.h, mpcqp_default_attitude; product library only)."""
        fn, header, _ = self.calls["mpcqp_default_attitude"]
        if fn is None:
            raise MpcQpError(f"mpcqp_default_attitude: {self.path} does not export include/{header} (product library only)")
        row = MpcQpAttitude()
        rc = fn(ctypes.byref(row))
        if rc != 0:
            raise MpcQpError(f"mpcqp_default_attitude failed: {rc}")
        return row

    def default_wrench_observer(self) -> "MpcQpWrenchObserver":
        """The wrench observer's default parameters (include/mpcqp_disturb.h, mpcqp_default_wrench_observer; product library only)."""
        fn, header, _ = self.calls["mpcqp_default_wrench_observer"]
        if fn is None:
            raise MpcQpError(f"mpcqp_default_wrench_observer: {self.path} does not export include/{header} (product library only)")
        row = MpcQpWrenchObserver()
        rc = fn(ctypes.byref(row))
        if rc != 0:
            raise MpcQpError(f"mpcqp_default_wrench_observer failed: {rc}")
        return row

    def default_compensate(self) -> "MpcQpCompensate":
        """The compensated roll-out's default parameters (include/mpcqp_compensate.h, mpcqp_default_compensate; product library only)."""
        fn, header, _ = self.calls["mpcqp_default_compensate"]
        if fn is None:
            raise MpcQpError(f"mpcqp_default_compensate: {self.path} does not export include/{header} (product library only)")
        row = MpcQpCompensate()
        rc = fn(ctypes.byref(row))
        if rc != 0:
            raise MpcQpError(f"mpcqp_default_compensate failed: {rc}")
        return row

    def default_config(self, **overrides) -> MpcQpConfig:
        cfg = MpcQpConfig()
        rc = self.lib.mpcqp_default_config(ctypes.byref(cfg))
        if rc != 0:
            raise MpcQpError(f"mpcqp_default_config failed: {rc}")
        # the ADMM block length is tuned per horizon: 100 iterations at N = 10 (the C default), 200 at N = 20 (measured:
        # +20 % throughput and 100 % instead of 98.8 % solved, tools/n20_knobs.py); explicit overrides win
        n = int(overrides.get("N", cfg.N))
        stage = n not in (10, 20) or bool(int(overrides.get("flags", cfg.flags)) & FLAG_STAGE_KERNEL)
        if n != 10 and "check_every" not in overrides:   # scale the library's own N = 10 defaults
            # (stage-wise engine, any other horizon: an iteration costs two recursions of N steps there and a polish attempt one
            #  factorisation, so shorter blocks pay -- 2 N: 120 at the reference's N = 60, tools/stage_sweep.py: 79.9 k QP/s on the
            #  logged ticks against 29.3 k at 10 N, 38.2 k against 20.3 k on a synthetic mixed batch, 100 % solved at both; with the
            #  Anderson-accelerated first block 5 N / 3 -- 100 at N = 60 -- tools/stage_accel.py, profiles/r03_stage_accel.txt:
            #  logged ticks 133.6 -> 143.5 k QP/s MIXED, 89.8 -> 133.4 k F64)
            cfg.check_every = max(50, (5 * n) // 3) if stage else max(1, cfg.check_every * n // 10)
            if "max_iter" not in overrides:
                cfg.max_iter = max(400 if stage else 1, cfg.max_iter * n // 10)
        # ... and so is the polish budget per round: twice the leg-stages, twice the steps (N = 20, eight batches of 4096: 14 -> 3
        # QPs left at the iteration cap at the same rate, tools/adapt_sweep.py; the steps inside a round update the inverse)
        if n != 10 and "polish_max" not in overrides:
            cfg.polish_max = max(4, cfg.polish_max * min(n, 20) // 10)
        for k, v in overrides.items():
            if k in ("w", "Ibody_inv"):
                arr = getattr(cfg, k)
                for i, x in enumerate(v):
                    arr[i] = float(x)
            else:
                if not hasattr(cfg, k):
                    raise AttributeError(f"MpcQpConfig has no field {k!r}")
                setattr(cfg, k, v)
        return cfg


class Engine:
    """One handle = one configuration on one device / stream.  Not thread-safe (include/mpcqp.h)."""

    def __init__(self, library: Library, cfg: MpcQpConfig):
        self.library = library
        self.cfg = cfg
        self._h = c_void_p()
        rc = library.lib.mpcqp_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc != 0:
            raise MpcQpError(f"mpcqp_create failed with code {rc}")

    def close(self):
        if self._h:
            self.library.lib.mpcqp_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return (self.library.lib.mpcqp_last_error(self._h) or b"").decode()

    def _call(self, name, *args):
        """The one call path into the library: `args` are the C parameters after the handle, in the C order.  An address of 0 or
        None is passed as NULL; a nonzero return code raises with the library's own message."""
        fn, header, is_address = self.library.calls[name]
        if fn is None and name in _GATED and getattr(self.library, "has_" + header[len("mpcqp_"):-len(".h")]):
            raise MpcQpError(f"{name}: {self.library.path} exports include/{header} without {' / '.join(_GATED[name][1])} (built before them)")
        if fn is None:
            raise MpcQpError(f"{name}: {self.library.path} does not export include/{header} (product library only)")
        if len(args) != len(is_address):
            raise TypeError(f"{name} takes {len(is_address)} arguments after the handle, got {len(args)}")
        rc = fn(self._h, *[(a or None) if p else int(a) for a, p in zip(args, is_address)])
        if rc != 0:
            raise MpcQpError(f"{name} failed with code {rc}: {self.last_error()}")

    def reserve(self, B):
        """Pre-size the batch-dependent workspace so that no later solve of at most B QPs allocates or synchronises."""
        self._call("mpcqp_reserve", B)

    # Raw calls: every buffer and `stream` is an integer address (device memory for the product library, host memory for the checker).
    def solve_batch_ptr(self, B, x0, r, contact, xdes, mu, u_out, X_out, status, iters, res, stream=0):
        self._call("mpcqp_solve_batch", B, x0, r, contact, xdes, mu, u_out, X_out, status, iters, res, stream)

    def solve_batch_gait_ptr(self, B, x0, ref, feet0, footholds, gait, feet_id, mu, u_out, X_out, status, iters, res, stream=0):
        self._call("mpcqp_solve_batch_gait", B, x0, ref, feet0, footholds, gait, feet_id, mu, u_out, X_out, status, iters, res, stream)

    def solve_batch_gait_steps_ptr(self, B, S, x0, ref, feet0, footholds, gait, feet_id, mu, u_out, X_out, status, iters, res, stream=0):
        """The gait entry point with S plan steps per robot (footholds [B,S,4,3], feet_id [B,S,4])."""
        self._call("mpcqp_solve_batch_gait_steps", B, S, x0, ref, feet0, footholds, gait, feet_id, mu, u_out, X_out, status, iters, res, stream)

    def rollout_ptr(self, B, T, S, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, actual, desired, forces, solved, stream=0):
        """The closed-loop roll-out (include/mpcqp.h, mpcqp_rollout)."""
        self._call("mpcqp_rollout", B, T, S, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, actual, desired, forces, solved, stream)

    def plan_footsteps_ptr(self, B, S, feet0, cmd, gait, plan_pos, plan_feet_id, plan_meta, plan_ang=0, plan_hip=0, stream=0):
        """The device footstep planner (include/mpcqp_plan.h)."""
        self._call("mpcqp_plan_footsteps", B, S, feet0, cmd, gait, plan_pos, plan_feet_id, plan_meta, plan_ang, plan_hip, stream)

    def swing_trajectories_ptr(self, B, K, S, plan_pos, plan_feet_id, plan_meta, plan_ang, tick, step_height, traj, feet_des=0, stream=0):
        """The device swing-foot trajectory generator (include/mpcqp_plan.h)."""
        self._call("mpcqp_swing_trajectories", B, K, S, plan_pos, plan_feet_id, plan_meta, plan_ang, tick, step_height, traj, feet_des, stream)

    def plant_step_ptr(self, B, x, f, feet, contact, body, wrench, substeps, x_out, stream=0):
        """The rigid-body plant (include/mpcqp_sim.h, mpcqp_plant_step)."""
        self._call("mpcqp_plant_step", B, x, f, feet, contact, body, wrench, substeps, x_out, stream)

    def rollout_plant_ptr(self, B, T, S, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, body, push, push_ticks, substeps,
                          actual, desired, forces, solved, stream=0):
        """The roll-out on the rigid-body plant (include/mpcqp_sim.h, mpcqp_rollout_plant)."""
        self._call("mpcqp_rollout_plant", B, T, S, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, body, push, push_ticks, substeps,
                   actual, desired, forces, solved, stream)

    def phase_expand_ptr(self, B, x0, ref, feet, gait, tick, stand, gain, r, contact, xdes, stream=0):
        """The per-leg gait clock and foothold rule expanded into an operator tuple (include/mpcqp_plan.h, mpcqp_phase_expand)."""
        self._call("mpcqp_phase_expand", B, x0, ref, feet, gait, tick, stand, gain, r, contact, xdes, stream)

    def solve_batch_phase_ptr(self, B, x0, ref, feet, gait, tick, stand, gain, mu, u_out, X_out, status, iters, res, stream=0):
        """That expansion and the solve in one call (include/mpcqp_plan.h, mpcqp_solve_batch_phase)."""
        self._call("mpcqp_solve_batch_phase", B, x0, ref, feet, gait, tick, stand, gain, mu, u_out, X_out, status, iters, res, stream)

    def rollout_phase_ptr(self, B, T, x, ref, feet, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, actual, desired, forces,
                          feet_log, contact_log, solved, stream=0):
        """The roll-out on the plant with a gait clock and reactive footholds (include/mpcqp_sim.h, mpcqp_rollout_phase)."""
        self._call("mpcqp_rollout_phase", B, T, x, ref, feet, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, actual, desired,
                   forces, feet_log, contact_log, solved, stream)

    def rollout_legs_ptr(self, B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height, gains,
                         leg_substeps, land, actual, desired, forces, feet_log, contact_log, solved, swing_log, q_log, qd_log, tau_log,
                         foot_log, err_log, flag_log, miss_log, geometry=None, inertia=None, stream=0):
        """The roll-out on a gait clock with the swing legs integrated inside it (include/mpcqp_sim.h, mpcqp_rollout_legs)."""
        self._call("mpcqp_rollout_legs", B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height,
                   gains, leg_substeps, geometry, inertia, land, actual, desired, forces, feet_log, contact_log, solved, swing_log, q_log,
                   qd_log, tau_log, foot_log, err_log, flag_log, miss_log, stream)

    def rollout_score_ptr(self, B, T, actual, desired, forces, contact_log, tau, qd, flag, miss, accumulate, score, rule=None, stream=0):
        """The score row of a roll-out's logs (include/mpcqp_sim.h, mpcqp_rollout_score); `rule` is an MpcQpScoreRule or None = the defaults."""
        self._call("mpcqp_rollout_score", B, T, actual, desired, forces, contact_log, tau, qd, flag, miss, rule, accumulate, score, stream)

    def stance_drive_ptr(self, B, x, f, feet, contact, ground, f_out, tau=0, flag=0, geometry=None, inertia=None, stream=0):
        """What the stance legs deliver of a commanded force (include/mpcqp_sim.h, mpcqp_stance_drive)."""
        self._call("mpcqp_stance_drive", B, x, f, feet, contact, ground, geometry, inertia, f_out, tau, flag, stream)

    def rollout_drive_ptr(self, B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height, gains,
                          leg_substeps, land, drive, ground, actual, desired, forces, feet_log, contact_log, solved, swing_log, q_log, qd_log,
                          tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, geometry=None, inertia=None, stream=0):
        """`rollout_legs_ptr` with the stance drive in the loop (include/mpcqp_sim.h, mpcqp_rollout_drive)."""
        self._call("mpcqp_rollout_drive", B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height,
                   gains, leg_substeps, geometry, inertia, land, drive, ground, actual, desired, forces, feet_log, contact_log, solved,
                   swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, stream)

    def stance_slip_ptr(self, B, x, f, feet, contact, ground, foot_mass, slip_in, f_out, tau=0, flag=0, slip_out=0, disp=0, substeps=0,
                        geometry=None, inertia=None, stream=0):
        """The stance drive with slip kinematics on the caller's rows (include/mpcqp_slip.h, mpcqp_stance_slip)."""
        self._call("mpcqp_stance_slip", B, x, f, feet, contact, ground, foot_mass, slip_in, substeps, geometry, inertia, f_out, tau, flag,
                   slip_out, disp, stream)

    def rollout_slip_ptr(self, B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height, gains,
                         leg_substeps, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log, contact_log, solved, swing_log,
                         q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log, geometry=None,
                         inertia=None, stream=0):
        """`rollout_drive_ptr` with stance feet that slide (include/mpcqp_slip.h, mpcqp_rollout_slip)."""
        self._call("mpcqp_rollout_slip", B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height,
                   gains, leg_substeps, geometry, inertia, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log, contact_log,
                   solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log, stream)

    def rollout_observe_ptr(self, B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height, gains,
                            leg_substeps, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log, contact_log, solved,
                            swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log, imu_log,
                            q_enc_log, qd_enc_log, est_log, feet_est_log, sigma_log, nis_log, feed, est_state, est_init=0, height=0, bias=0,
                            noise=0, enc_noise=0, estimator=None, geometry=None, inertia=None, stream=0):
        """`rollout_slip_ptr` with sensors and the state estimator inside the tick loop (include/mpcqp_observe.h, mpcqp_rollout_observe).
        As in the other roll-outs every log comes before what is not one: the seven logs of the estimator follow disp_log here, the feed,
        the filter state and the sensors' operands follow them (the C order has them in between)."""
        self._call("mpcqp_rollout_observe", B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height,
                   gains, leg_substeps, geometry, inertia, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log, contact_log,
                   solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log, feed,
                   est_state, est_init, height, bias, noise, enc_noise, estimator, imu_log, q_enc_log, qd_enc_log, est_log, feet_est_log,
                   sigma_log, nis_log, stream)

    def rollout_observe_gated_ptr(self, B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height,
                                  gains, leg_substeps, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log, contact_log,
                                  solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log,
                                  imu_log, q_enc_log, qd_enc_log, est_log, feet_est_log, sigma_log, nis_log, trust_log, feed, est_state,
                                  est_init=0, height=0, bias=0, noise=0, enc_noise=0, estimator=None, gate=None, geometry=None, inertia=None,
                                  stream=0):
        """`rollout_observe_ptr` with the estimator's trust gated per leg (include/mpcqp_gate.h, mpcqp_rollout_observe_gated): trust_log
        follows nis_log among the logs, `gate` (an MpcQpTrustGate or None = the defaults) follows `estimator`."""
        self._call("mpcqp_rollout_observe_gated", B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps,
                   step_height, gains, leg_substeps, geometry, inertia, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log,
                   contact_log, solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log,
                   feed, est_state, est_init, height, bias, noise, enc_noise, estimator, imu_log, q_enc_log, qd_enc_log, est_log, feet_est_log,
                   sigma_log, nis_log, gate, trust_log, stream)

    def rollout_observe_aided_ptr(self, B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps, step_height,
                                  gains, leg_substeps, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log, contact_log,
                                  solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log,
                                  imu_log, q_enc_log, qd_enc_log, est_log, feet_est_log, sigma_log, nis_log, trust_log, bias_log, feed,
                                  est_state, est_init=0, height=0, bias=0, noise=0, enc_noise=0, estimator=None, gate=None, flags=0,
                                  attitude=None, att_state=0, geometry=None, inertia=None, stream=0):
        """`rollout_observe_gated_ptr` with the aided attitude rule (include/mpcqp_attitude.h, mpcqp_rollout_observe_aided): bias_log
        follows trust_log among the logs; `flags` (AIDED_GATE: run the gate), `attitude` (an MpcQpAttitude or None = the defaults) and
        att_state follow `gate`."""
        self._call("mpcqp_rollout_observe_aided", B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps,
                   step_height, gains, leg_substeps, geometry, inertia, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log,
                   contact_log, solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log,
                   feed, est_state, est_init, height, bias, noise, enc_noise, estimator, imu_log, q_enc_log, qd_enc_log, est_log, feet_est_log,
                   sigma_log, nis_log, gate, trust_log, flags, attitude, att_state, bias_log, stream)

    def rollout_observe_compensated_ptr(self, B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps,
                                        step_height, gains, leg_substeps, land, drive, ground, foot_mass, slip, actual, desired, forces,
                                        feet_log, contact_log, solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log,
                                        miss_log, cmd_log, slip_log, disp_log, imu_log, q_enc_log, qd_enc_log, est_log, feet_est_log,
                                        sigma_log, nis_log, trust_log, bias_log, dist_log, resid_log, feed, est_state, est_init=0, height=0,
                                        bias=0, noise=0, enc_noise=0, estimator=None, gate=None, flags=0, attitude=None, att_state=0,
                                        compensate=None, obs_body=0, dist_state=0, geometry=None, inertia=None, stream=0):
        """`rollout_observe_aided_ptr` with the wrench observer and the table update inside the tick (include/mpcqp_compensate.h,
        mpcqp_rollout_observe_compensated): dist_log and resid_log follow bias_log among the logs; `compensate` (an MpcQpCompensate or
        None = the defaults), obs_body and dist_state follow att_state."""
        self._call("mpcqp_rollout_observe_compensated", B, T, x, ref, feet, legs, gait, stand, gain, tick, mu, body, push, push_ticks, substeps,
                   step_height, gains, leg_substeps, geometry, inertia, land, drive, ground, foot_mass, slip, actual, desired, forces, feet_log,
                   contact_log, solved, swing_log, q_log, qd_log, tau_log, foot_log, err_log, flag_log, miss_log, cmd_log, slip_log, disp_log,
                   feed, est_state, est_init, height, bias, noise, enc_noise, estimator, imu_log, q_enc_log, qd_enc_log, est_log, feet_est_log,
                   sigma_log, nis_log, gate, trust_log, flags, attitude, att_state, bias_log, compensate, obs_body, dist_state, dist_log,
                   resid_log, stream)

    # (`estimator` is an MpcQpEstimator or None = the defaults)
    def imu_log_ptr(self, B, T, actual, forces, feet, base_acc, body, bias, noise, imu, estimator=None, stream=0):
        """What an IMU at the CoM reads on every row of a log (include/mpcqp_estimate.h, mpcqp_imu_log)."""
        self._call("mpcqp_imu_log", B, T, actual, forces, feet, base_acc, body, bias, noise, estimator, imu, stream)

    def estimate_track_ptr(self, B, T, imu, q, qd, contact_log, trust, height, init, state, est, feet_est, sigma, nis, estimator=None,
                           geometry=None, stream=0):
        """The state estimator over the rows of a log (include/mpcqp_estimate.h, mpcqp_estimate_track)."""
        self._call("mpcqp_estimate_track", B, T, imu, q, qd, contact_log, trust, height, init, estimator, geometry, state, est, feet_est,
                   sigma, nis, stream)

    def estimate_track_gated_ptr(self, B, T, imu, q, qd, contact_log, trust, height, init, state, est, feet_est, sigma, nis, trust_out,
                                 estimator=None, gate=None, geometry=None, stream=0):
        """`estimate_track_ptr` with the trust gated per leg (include/mpcqp_gate.h, mpcqp_estimate_track_gated); `gate` is an
        MpcQpTrustGate or None = the defaults."""
        self._call("mpcqp_estimate_track_gated", B, T, imu, q, qd, contact_log, trust, height, init, estimator, geometry, state, est, feet_est,
                   sigma, nis, gate, trust_out, stream)

    def estimate_track_aided_ptr(self, B, T, imu, q, qd, contact_log, trust, height, init, state, est, feet_est, sigma, nis, trust_out,
                                 bias_log, estimator=None, gate=None, flags=0, attitude=None, att_state=0, geometry=None, stream=0):
        """`estimate_track_gated_ptr` with the aided attitude rule (include/mpcqp_attitude.h, mpcqp_estimate_track_aided): `flags`
        (AIDED_GATE: run the gate), `attitude` an MpcQpAttitude or None = the defaults, att_state the address of float64 [B,8] or 0."""
        self._call("mpcqp_estimate_track_aided", B, T, imu, q, qd, contact_log, trust, height, init, estimator, geometry, state, est, feet_est,
                   sigma, nis, gate, trust_out, flags, attitude, att_state, bias_log, stream)

    def phase_swing_ptr(self, B, T, actual, desired, feet_log, gait, tick0, stand, gain, step_height, swing, feet_des=0, stream=0):
        """The swing-foot trajectories of a roll-out on a gait clock, from its logs (include/mpcqp_plan.h, mpcqp_phase_swing)."""
        self._call("mpcqp_phase_swing", B, T, actual, desired, feet_log, gait, tick0, stand, gain, step_height, swing, feet_des, stream)

    def set_models_ptr(self, B, model, stream=0):
        """mpcqp_set_models (include/mpcqp_model.h): `model` is the address of an fp64 [B,6] device table."""
        self._call("mpcqp_set_models", B, model, stream)

    def clear_models(self):
        """mpcqp_clear_models (include/mpcqp_model.h): back to the configuration's m, Ibody_inv, f_min, f_max."""
        self._call("mpcqp_clear_models")

    def set_disturbance_ptr(self, B, rows, stream=0):
        """mpcqp_set_disturbance (include/mpcqp_disturb.h): `rows` is the address of an fp64 [B,6] device table."""
        self._call("mpcqp_set_disturbance", B, rows, stream)

    def clear_disturbance(self):
        """mpcqp_clear_disturbance (include/mpcqp_disturb.h): back to no disturbance for every QP."""
        self._call("mpcqp_clear_disturbance")

    def disturbance_shift_ptr(self, B, x0, xdes, out, stream=0):
        """mpcqp_disturbance_shift (include/mpcqp_disturb.h): out = xdes - s with the table that is set."""
        self._call("mpcqp_disturbance_shift", B, x0, xdes, out, stream)

    def disturbance_track_ptr(self, B, T, actual, forces, feet, body, state, dist, resid, observer=None, stream=0):
        """The wrench observer over the rows of a log (include/mpcqp_disturb.h, mpcqp_disturbance_track)."""
        self._call("mpcqp_disturbance_track", B, T, actual, forces, feet, body, observer, state, dist, resid, stream)

    def set_actuators_ptr(self, B, act, stream=0):
        """mpcqp_set_actuators (include/mpcqp_actuators.h): `act` is the address of an fp64 [B,9] device table."""
        self._call("mpcqp_set_actuators", B, act, stream)

    def clear_actuators(self):
        """mpcqp_clear_actuators (include/mpcqp_actuators.h): back to the inertia row's tau_max for every clamp."""
        self._call("mpcqp_clear_actuators")

    # (`geometry` is an MpcQpLegGeometry or None = the Lite3; ctypes passes the structure by reference)
    def leg_ik_ptr(self, B, foot, rot, origin, q, reach=0, geometry=None, stream=0):
        """The closed-form leg inverse kinematics (include/mpcqp_joints.h, mpcqp_leg_ik)."""
        self._call("mpcqp_leg_ik", B, foot, rot, origin, geometry, q, reach, stream)

    def joint_log_ptr(self, B, T, actual, forces, feet, q, tau, reach, geometry=None, stream=0):
        """The joint-space log of a roll-out (include/mpcqp_joints.h, mpcqp_joint_log)."""
        self._call("mpcqp_joint_log", B, T, actual, forces, feet, geometry, q, tau, reach, stream)

    def joint_rates_ptr(self, B, T, actual, forces, feet, foot_vel, q, qd, tau, power, reach, geometry=None, stream=0):
        """The joint-space log with joint rates and power (include/mpcqp_joints.h, mpcqp_joint_rates)."""
        self._call("mpcqp_joint_rates", B, T, actual, forces, feet, foot_vel, geometry, q, qd, tau, power, reach, stream)

    # (`inertia` is an MpcQpLegInertia or None = the Lite3)
    def leg_dynamics_ptr(self, B, q, qd, qdd, rot, base, tau, mass, bias, geometry=None, inertia=None, stream=0):
        """The leg's equations of motion (include/mpcqp_joints.h, mpcqp_leg_dynamics)."""
        self._call("mpcqp_leg_dynamics", B, q, qd, qdd, rot, base, geometry, inertia, tau, mass, bias, stream)

    def leg_effort_ptr(self, B, T, actual, forces, feet, foot_vel, foot_acc, base_acc, body, qdd, tau_dyn, tau, power, limit, geometry=None,
                       inertia=None, stream=0):
        """The full joint torques of a roll-out's log and the actuator-limit flags (include/mpcqp_joints.h, mpcqp_leg_effort)."""
        self._call("mpcqp_leg_effort", B, T, actual, forces, feet, foot_vel, foot_acc, base_acc, body, geometry, inertia, qdd, tau_dyn, tau,
                   power, limit, stream)

    def leg_accel_ptr(self, B, q, qd, tau, rot, base, qdd, det=0, geometry=None, inertia=None, stream=0):
        """The leg's forward dynamics (include/mpcqp_joints.h, mpcqp_leg_accel)."""
        self._call("mpcqp_leg_accel", B, q, qd, tau, rot, base, geometry, inertia, qdd, det, stream)

    def swing_track_ptr(self, B, T, actual, forces, feet_log, contact_log, swing, base_acc, body, gains, state, substeps, q, qd, tau, foot,
                        err, flag, geometry=None, inertia=None, stream=0):
        """The swing legs of a roll-out as a controlled plant (include/mpcqp_joints.h, mpcqp_swing_track)."""
        self._call("mpcqp_swing_track", B, T, actual, forces, feet_log, contact_log, swing, base_acc, body, gains, state, substeps, geometry,
                   inertia, q, qd, tau, foot, err, flag, stream)

    def torque_map_ptr(self, B, u, jac, tau, stream=0):
        self._call("mpcqp_torque_map", B, u, jac, tau, stream)

    def leg_jacobians_ptr(self, B, q, rot, jac, foot=0, geometry=None, stream=0):
        self._call("mpcqp_leg_jacobians", B, q, rot, geometry, jac, foot, stream)

    def last_kernel_ms(self) -> float:
        ms = c_float()
        self._call("mpcqp_last_kernel_ms", ctypes.byref(ms))
        return float(ms.value)

    # host-pointer convenience (numpy); valid for libraries that take host memory
    def rollout_host(self, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T):
        """Oracle convenience (host memory, float64): returns the advanced (x, ref, tick) and the per-tick logs."""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64).copy()
        x, ref, mu = f(x), f(ref), f(mu)
        pos = f(plan_pos); fid = np.ascontiguousarray(plan_feet_id, dtype=np.uint8)
        meta = np.ascontiguousarray(plan_meta, dtype=np.int32); tick = np.ascontiguousarray(tick, dtype=np.int32).copy()
        B, S = pos.shape[0], pos.shape[1]
        actual = np.zeros((B, T, 12)); desired = np.zeros((B, T, 12)); forces = np.zeros((B, T, 12)); solved = np.zeros(B, np.int32)
        self.rollout_ptr(B, T, S, x.ctypes.data, ref.ctypes.data, pos.ctypes.data, fid.ctypes.data, meta.ctypes.data, tick.ctypes.data,
                         mu.ctypes.data, actual.ctypes.data, desired.ctypes.data, forces.ctypes.data, solved.ctypes.data)
        return {"x": x, "ref": ref, "tick": tick, "actual": actual, "desired": desired, "forces": forces, "solved": solved}

    def leg_jacobians_host(self, q, rot=None, geometry=None):
        """Host-memory call (the CPU checker): q [B,4,3], rot [B,3,3] or None -> (jac [B,4,3,3], foot [B,4,3]), float64."""
        q = np.ascontiguousarray(q, dtype=np.float64); B = q.shape[0]
        rot = None if rot is None else np.ascontiguousarray(rot, dtype=np.float64)
        jac = np.zeros((B, 4, 3, 3)); foot = np.zeros((B, 4, 3))
        self.leg_jacobians_ptr(B, q.ctypes.data, 0 if rot is None else rot.ctypes.data, jac.ctypes.data, foot.ctypes.data, geometry)
        return jac, foot

    def _host_dtype(self):
        return np.float64 if self.cfg.dtype == DTYPE_F64 else np.float32

    def _host_results(self, B, want_X):
        """The result dict of the two *_host solves and the addresses of its arrays, in the C order of the outputs."""
        N, ft = self.cfg.N, self._host_dtype()
        out = {"u": np.zeros((B, N, 12), ft), "X": np.zeros((B, N + 1, 13), ft) if want_X else None,
               "status": np.zeros(B, np.int32), "iters": np.zeros(B, np.int32), "res": np.zeros((B, 2), np.float32)}
        return out, [a.ctypes.data if a is not None else None for a in out.values()]

    def solve_batch_host(self, x0, r, contact, xdes, mu, want_X=True):
        N, ft = self.cfg.N, self._host_dtype()
        x0 = np.ascontiguousarray(x0, dtype=ft); r = np.ascontiguousarray(r, dtype=ft)
        xdes = np.ascontiguousarray(xdes, dtype=ft); mu = np.ascontiguousarray(mu, dtype=ft)
        contact = np.ascontiguousarray(contact, dtype=np.uint8)
        B = x0.shape[0]
        assert x0.shape == (B, 13) and r.shape == (B, N, 4, 3) and contact.shape == (B, N, 4)
        assert xdes.shape == (B, N + 1, 13) and mu.shape == (B,)
        out, out_ptrs = self._host_results(B, want_X)
        self.solve_batch_ptr(B, x0.ctypes.data, r.ctypes.data, contact.ctypes.data, xdes.ctypes.data, mu.ctypes.data, *out_ptrs)
        return out

    def solve_batch_gait_host(self, g, want_X=True):
        """Host-pointer convenience for the gait entry point; `g` is a dict as produced by synth.make_gait_batch (footholds [B,S,4,3])."""
        ft = self._host_dtype()
        a = {k: np.ascontiguousarray(g[k], dtype=ft) for k in ("x0", "ref", "feet0", "footholds", "mu")}
        gait = np.ascontiguousarray(g["gait"], dtype=np.int32); fid = np.ascontiguousarray(g["feet_id"], dtype=np.uint8)
        B, S = a["x0"].shape[0], a["footholds"].shape[1]
        out, out_ptrs = self._host_results(B, want_X)
        self.solve_batch_gait_steps_ptr(B, S, a["x0"].ctypes.data, a["ref"].ctypes.data, a["feet0"].ctypes.data, a["footholds"].ctypes.data,
                                        gait.ctypes.data, fid.ctypes.data, a["mu"].ctypes.data, *out_ptrs)
        return out


_product = None


def product_library() -> Library:
    """The HIP engine.  Raises (loudly) when the extension has not been built -- never falls back."""
    global _product
    if _product is None:
        # PyTorch-ROCm carries its own HIP runtime: it has to be in the process BEFORE libmpcqp.so pulls in /opt/rocm's, or the
        # one loaded second sees no device (mpcqp_create: MPCQP_ENODEV after `build()` + `smoke()` in one process, measured).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _product = Library(PRODUCT_LIB)
    return _product
