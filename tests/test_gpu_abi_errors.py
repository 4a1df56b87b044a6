"""The host checks of the C-ABI, entry point by entry point: which call is rejected, with which text, and which text wins when two
things are wrong at once.

One table (`_chains`).  An entry point's row is the ordered chain of its checks as csrc/mpcqp_kernels.hip makes them: a step is a list
of defects (arguments to replace in an otherwise complete call, the text after "<name>: ").  The test sends every defect by itself and
every defect together with the first one of each later step, and expects the text of the earlier step.  The model and actuator tables of the two
handles (two rows each, against the calls' B = 1) are defects that are always there: they are the last steps of the entry points that
read a table, so a call without another defect is rejected by them, and a call that nothing rejects is never sent.  Every call here
returns before the entry point touches the device (the only launches of this module are the three table conversions of the set-up)."""
import ctypes
import inspect
import math

import pytest

import mpcqp
from mpcqp._capi import MpcQpLegGeometry, MpcQpScoreRule

NAN, INF = math.nan, math.inf
RANGE, SIZE, NULL = "batch size out of range", "size out of range", "null buffer"
SUBSTEPS, LEG_SUBSTEPS = "substeps out of range [0, 1000]", "leg_substeps out of range [0, 1000]"
PUSH = "push without push_ticks"
INTS = {"B": 1, "T": 1, "S": 1, "K": 1, "substeps": 0, "leg_substeps": 0, "land": 0, "drive": 1, "accumulate": 0}
BIG31, BIG29 = 1 << 31, 1 << 29      # one past the 0x7fffffff / 0x1fffffff limits


def _geometry(lib, *edits):
    g = MpcQpLegGeometry()
    assert lib.lib.mpcqp_default_leg_geometry(ctypes.byref(g)) == 0
    for e in edits:
        e(g)
    return g


def _inertia(lib, *edits):
    r = lib.default_leg_inertia()
    for e in edits:
        e(r)
    return r


def _set(field, value, *index):
    def edit(s):
        if not index:
            setattr(s, field, value)
            return
        a = getattr(s, field)
        for i in index[:-1]:
            a = a[i]
        a[index[-1]] = value
    return edit


# The fields of the two structs in the order in which they are checked: (edit, text)
SIZE_GEO = (_set("size", 0), "geometry struct size mismatch")
CLOSED = "the closed form needs the Lite3's leg structure: "
IK_GEO = [SIZE_GEO,
          (_set("axis_x", 0.0, 0), CLOSED + "axis_x is not +-e_x"),
          (_set("axis_x", 0.1, 1), CLOSED + "axis_x is not +-e_x"),
          (_set("axis_y", NAN, 1), CLOSED + "axis_y is not +-e_y"),
          (_set("knee", 0.2, 2), CLOSED + "knee is not (0, 0, -l1), l1 > 0"),
          (_set("foot", 0.01, 0), CLOSED + "foot is not (0, 0, -l2), l2 > 0"),
          (_set("hip_y", 0.01, 1, 0), CLOSED + "hip_y is not (0, d, 0)"),
          (_set("hip_x", INF, 1, 2), CLOSED + "hip_x is not finite")]
FK_GEO = [SIZE_GEO,
          (_set("axis_x", 0.0, 0), "zero joint axis"),
          (_set("axis_y", NAN, 2), "zero joint axis")]
ROW = "invalid leg inertia row: "
INERTIA = [(_set("size", 8), "inertia struct size mismatch"),
           (_set("mass", NAN, 3, 2), ROW + "mass is not finite"),
           (_set("com", INF, 0, 1, 2), ROW + "com is not finite"),
           (_set("inertia", NAN, 2, 0, 5), ROW + "inertia is not finite"),
           (_set("q_min", NAN, 1), ROW + "q_min is not finite"),
           (_set("q_max", INF, 2), ROW + "q_max is not finite"),
           (_set("qd_max", NAN, 0), ROW + "qd_max is not finite"),
           (_set("tau_max", NAN, 2), ROW + "tau_max is not finite"),
           (_set("gravity", 0.0), ROW + "gravity is not negative and finite"),
           (_set("mass", -0.1, 1, 1), ROW + "mass is negative"),
           (_set("q_min", 1.0, 0), ROW + "q_min > q_max"),
           (_set("qd_max", -1.0, 0), ROW + "qd_max is negative"),
           (_set("tau_max", -1.0, 0), ROW + "tau_max is negative")]


def _struct_step(lib, make, arg, fields):
    """One step of a chain from a struct's fields: every field by itself, and every two neighbours in one struct (the earlier wins)."""
    step = [({arg: make(lib, e)}, text) for e, text in fields]
    step += [({arg: make(lib, e0, e1)}, t0) for (e0, t0), (e1, _) in zip(fields, fields[1:])]
    return step


def _chains(lib, a):
    """name of the C function -> (Engine method, name in the texts, [steps]); a is a device address that no call gets to read."""
    ik = _struct_step(lib, _geometry, "geometry", IK_GEO)
    fk = _struct_step(lib, _geometry, "geometry", FK_GEO)
    inr = _struct_step(lib, _inertia, "inertia", INERTIA)
    null = lambda *names: [({n: 0}, NULL) for n in names]
    rng31 = [({"B": -1}, RANGE), ({"B": BIG31}, RANGE)]
    rng29 = [({"B": -1}, RANGE), ({"B": BIG29}, RANGE)]
    bt = lambda lim: [({"B": -1}, SIZE), ({"T": -1}, SIZE), ({"B": BIG31}, SIZE), ({"B": lim >> 1, "T": 2}, SIZE)]
    sub = [({"substeps": -1}, SUBSTEPS), ({"substeps": 1001}, SUBSTEPS)]
    push = [({"push_ticks": 0}, PUSH)]
    models = [({}, "batch size 1, but the model table has 2 rows")]
    acts = [({}, "batch size 1, but the actuator table has 2 rows")]
    gait_null = null("x0", "ref", "feet0", "footholds", "gait", "feet_id", "mu", "u_out", "status", "iters")
    plan_null = null("x", "ref", "plan_pos", "plan_feet_id", "plan_meta", "tick", "mu")
    legs = [bt(BIG31), sub, [({"leg_substeps": -1}, LEG_SUBSTEPS), ({"leg_substeps": 1001}, LEG_SUBSTEPS)],
            [({"land": v}, "land is neither MPCQP_LAND_RULE nor MPCQP_LAND_ACTUAL") for v in (-1, 2)]]
    drive = [[({"drive": v}, "drive is neither MPCQP_DRIVE_IDEAL nor MPCQP_DRIVE_LIMITED") for v in (-1, 2)]]
    legs_null = [push, null("x", "ref", "feet", "legs", "gait", "stand", "tick", "mu", "step_height")]
    legs_rows = [ik, inr, models, acts]
    none_of = lambda *names: [({n: 0 for n in names}, f"no output buffer ({', '.join(names[:-1])} and {names[-1]} are all null)")]
    log_null = null("actual", "forces", "feet")
    return {
        "mpcqp_reserve": ("reserve", None, [rng31]),
        "mpcqp_solve_batch": ("solve_batch_ptr", None, [rng31, null("x0", "r", "contact", "xdes", "mu", "u_out", "status", "iters"), models]),
        "mpcqp_solve_batch_gait": ("solve_batch_gait_ptr", "mpcqp_solve_batch_gait_steps", [rng31, gait_null, models]),
        "mpcqp_solve_batch_gait_steps": ("solve_batch_gait_steps_ptr", None,
                                         [[({"S": 0}, "at least one plan step"), ({"S": -3}, "at least one plan step")], rng31, gait_null, models]),
        "mpcqp_rollout": ("rollout_ptr", None, [[({"B": -1}, SIZE), ({"B": BIG31}, SIZE), ({"T": -1}, SIZE), ({"S": 0}, SIZE)], plan_null, models]),
        "mpcqp_torque_map": ("torque_map_ptr", None, [rng29, null("u", "jac", "tau")]),
        "mpcqp_leg_jacobians": ("leg_jacobians_ptr", None, [rng29, null("q", "jac"), fk]),
        "mpcqp_last_kernel_ms": ("last_kernel_ms", None, [[({}, "no solve recorded")]]),
        "mpcqp_plan_footsteps": ("plan_footsteps_ptr", None,
                                 [[({"B": -1}, SIZE), ({"B": BIG31}, SIZE), ({"S": 0}, SIZE), ({"B": 1 << 30, "S": 2}, SIZE)],
                                  null("feet0", "cmd", "gait", "plan_pos", "plan_feet_id", "plan_meta")]),
        "mpcqp_swing_trajectories": ("swing_trajectories_ptr", None,
                                     [[({"B": -1}, SIZE), ({"B": BIG31}, SIZE), ({"K": -1}, SIZE), ({"S": 0}, SIZE), ({"B": 1 << 30, "K": 2}, SIZE)],
                                      null("plan_pos", "plan_feet_id", "plan_meta", "plan_ang", "tick", "step_height", "traj")]),
        "mpcqp_phase_expand": ("phase_expand_ptr", None, [rng31, null("x0", "ref", "feet", "gait", "tick", "stand", "r", "contact", "xdes")]),
        "mpcqp_solve_batch_phase": ("solve_batch_phase_ptr", None,
                                    [rng31, null("x0", "ref", "feet", "gait", "tick", "stand", "mu", "u_out", "status", "iters"), models]),
        "mpcqp_phase_swing": ("phase_swing_ptr", None,
                              [bt(BIG31), null("actual", "desired", "feet_log", "gait", "tick0", "stand", "step_height", "swing")]),
        "mpcqp_plant_step": ("plant_step_ptr", None, [rng31, sub, null("x", "f", "feet", "contact", "x_out")]),
        "mpcqp_rollout_plant": ("rollout_plant_ptr", None,
                                [[({"B": -1}, SIZE), ({"B": BIG31}, SIZE), ({"T": -1}, SIZE), ({"S": 0}, SIZE)], sub, push, plan_null, models]),
        "mpcqp_rollout_phase": ("rollout_phase_ptr", None, [bt(BIG31), sub, push, null("x", "ref", "feet", "gait", "stand", "tick", "mu"), models]),
        "mpcqp_rollout_legs": ("rollout_legs_ptr", None, legs + legs_null + legs_rows),
        "mpcqp_rollout_drive": ("rollout_drive_ptr", None, legs + drive + legs_null + legs_rows),
        "mpcqp_rollout_slip": ("rollout_slip_ptr", None, legs + drive + legs_null + [null("ground", "foot_mass", "slip")] + legs_rows),
        "mpcqp_rollout_score": ("rollout_score_ptr", None, [
            bt(BIG31),
            [(d, "the leg group is tau, qd and flag: all three or none") for d in ({"tau": 0}, {"qd": 0}, {"flag": 0}, {"tau": 0, "flag": 0})],
            null("score", "actual", "desired", "forces", "contact_log"),
            [({"rule": MpcQpScoreRule(0, 0.5, 1.0)}, "rule struct size mismatch")],
            [({"rule": MpcQpScoreRule(ctypes.sizeof(MpcQpScoreRule), z, t)}, "z_frac and tilt_max must be finite and positive")
             for z, t in ((0.0, 1.0), (0.5, -1.0), (NAN, 1.0), (0.5, INF))],
            [({n: a + 8}, "a log buffer is not 16-byte aligned") for n in ("actual", "desired", "forces", "tau", "qd", "miss")],
            [({"contact_log": a + 2}, "contact_log / flag not 4-byte or score not 8-byte aligned"),
             ({"flag": a + 1}, "contact_log / flag not 4-byte or score not 8-byte aligned"),
             ({"score": a + 4}, "contact_log / flag not 4-byte or score not 8-byte aligned")]]),
        "mpcqp_stance_drive": ("stance_drive_ptr", None, [rng29, null("x", "f", "feet", "contact", "f_out"), ik, inr, acts]),
        "mpcqp_set_models": ("set_models_ptr", None, [[({"B": -1}, RANGE), ({"B": 0}, RANGE), ({"B": BIG31}, RANGE)], [({"model": 0}, "null model table")]]),
        "mpcqp_set_actuators": ("set_actuators_ptr", None,
                                [[({"B": -1}, RANGE), ({"B": 0}, RANGE), ({"B": BIG31}, RANGE)], [({"act": 0}, "null actuator table")]]),
        "mpcqp_leg_ik": ("leg_ik_ptr", None, [rng29, [({"foot": 0}, "null foot buffer")], [({"q": 0}, "null q buffer")], ik]),
        "mpcqp_joint_log": ("joint_log_ptr", None, [bt(BIG29), none_of("q", "tau", "reach"), log_null, ik]),
        "mpcqp_joint_rates": ("joint_rates_ptr", None, [bt(BIG29), none_of("q", "qd", "tau", "power", "reach"), log_null, ik]),
        "mpcqp_leg_dynamics": ("leg_dynamics_ptr", None, [rng29, none_of("tau", "mass", "bias"), [({"q": 0}, "null q buffer")], fk, inr]),
        "mpcqp_leg_effort": ("leg_effort_ptr", None, [bt(BIG29), none_of("qdd", "tau_dyn", "tau", "power", "limit"), log_null, ik, inr, acts]),
        "mpcqp_leg_accel": ("leg_accel_ptr", None, [rng29, [({"q": 0}, "null q buffer")], [({"tau": 0}, "null tau buffer")],
                                                    [({"qdd": 0}, "null qdd buffer")], fk, inr]),
        "mpcqp_swing_track": ("swing_track_ptr", None, [bt(BIG29), sub, none_of("q", "qd", "tau", "foot", "err", "flag"),
                                                        null("actual", "forces", "feet_log", "contact_log", "swing"), ik, inr, acts]),
        "mpcqp_stance_slip": ("stance_slip_ptr", None,
                              [rng29, sub, null("x", "f", "feet", "contact", "ground", "foot_mass", "slip_in", "f_out"), ik, inr, acts]),
    }


def _rows(steps, tables):
    """(arguments to replace, expected text) of every call the chain gives on a handle with `tables` in ("models", "actuators")."""
    absent = [f"the {t[:-1]} table" for t in ("models", "actuators") if t not in tables]
    steps = [s for s in steps if not any(a in s[0][1] for a in absent)]
    ambient = [i for i, s in enumerate(steps) if not s[0][0]]
    out = []

    def add(defects):   # [(step index, arguments, text)]
        first = min([(i, t) for i, _, t in defects] + [(i, steps[i][0][1]) for i in ambient])
        args = {}
        for _, d, _ in defects:
            if set(d) & set(args):
                return      # (the two defects are values of one argument)
            args.update(d)
        out.append((args, first[1]))

    if ambient:
        add([])
    for i, s in enumerate(steps):
        if i in ambient:
            continue
        for d, t in s:
            add([(i, d, t)])
        for j in range(i + 1, len(steps)):
            if j not in ambient:   # (every defect of the earlier step with the later step's first)
                for d, t in s:
                    add([(i, d, t), (j,) + steps[j][0]])
    return out


def _send(eng, method, args, a):
    fn = getattr(eng, method)
    call = {}
    for p in inspect.signature(getattr(type(eng), method)).parameters:
        if p == "self":
            continue
        if p in args:
            call[p] = args[p]
        elif p in INTS:
            call[p] = INTS[p]
        elif p in ("geometry", "inertia", "rule"):
            call[p] = None
        elif p == "stream":
            call[p] = 0
        else:
            call[p] = a
    assert not set(args) - set(call), (method, args)
    return fn(**call)


@pytest.mark.gpu
def test_every_entry_point_rejects_in_order():
    import torch
    lib = mpcqp.product_library()
    buf = torch.zeros(1 << 17, dtype=torch.float64, device="cuda")
    a = buf.data_ptr()
    assert a % 256 == 0
    both = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f64", precision="mixed")
    acts = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed")
    both.set_models(mpcqp.models.model_rows(both.cfg, 2)); both.set_actuators(mpcqp.actuators.actuator_rows(2))
    acts.set_actuators(mpcqp.actuators.actuator_rows(2))
    torch.cuda.synchronize()
    chains = _chains(lib, a)
    every = {row[0] for table in (mpcqp._capi.ABI, mpcqp._capi.ACTUATORS_ABI, mpcqp._capi.SLIP_ABI) for rows in table.values() for row in rows
             if row[2] and row[2][0] is mpcqp._capi._P}
    # (mpcqp_destroy, mpcqp_last_error and the two clear calls reject nothing)
    assert set(chains) == every - {"mpcqp_destroy", "mpcqp_last_error", "mpcqp_clear_models", "mpcqp_clear_actuators"}
    wrong, sent = [], 0
    for cname, (method, who, steps) in chains.items():
        for sol, tables in ((both, ("models", "actuators")), (acts, ("actuators",))):
            for args, text in _rows(steps, tables):
                want = f"{cname} failed with code -1: {who or cname}: {text}"
                try:
                    _send(sol.engine, method, args, a)
                    got = "no error"
                except mpcqp.MpcQpError as e:
                    got = str(e)
                sent += 1
                if got != want:
                    wrong.append(f"{cname} {sorted(args)}: {got!r}, expected {want!r}")
    print(f"{sent} rejected calls over {len(chains)} entry points")
    assert not wrong, "\n".join(wrong[:40])
    assert sent > 2000
    both.clear_actuators(); both.clear_models(); acts.clear_actuators()
