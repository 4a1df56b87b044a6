"""Developer aid for changes that must not change a result: seeded outputs of every entry point with whichever csrc/libmpcqp.so
is in place, as raw arrays in one .npz, and their comparison byte for byte (integer views: NaN payloads and signed zeros count).
Solves (tuple, gait S = 2, gait steps S = 4; f32 / f64 I/O; N = 10 / 20 / 60; MIXED / F64; warm start + shift over three calls),
the stage-wise engine at N = 60 and, by MPCQP_FLAG_STAGE_KERNEL, at N = 10 (MIXED / F64, cold and warm-started with shift),
roll-outs on the model and on the plant (T = 50, B = 1024, cold and warm, with the malformed plan rows of tests/test_rollout.py),
planner + swing trajectories, plant step, leg Jacobians and torque map, and the newer entry points (phase gaits, joints, leg dynamics,
leg simulation, leg roll-outs, score; with and without the model and actuator tables; at the tests' small shapes and at a ragged B = 333:
the section before the last), and the state estimator (imu_log, estimate_track and rollout_observe with their gated forms, every output and
the final est_state: the last section).  The stance rule's calls are in tools/stance_rule_compare.py.  One process per library build: copy the wanted build over
csrc/libmpcqp.so before starting each.
usage: dump_outputs.py OUT.npz            (needs a GPU)
       dump_outputs.py --compare A.npz B.npz"""

import os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = 0
    for k in sorted(set(a.files) | set(b.files)):
        if k not in a.files or k not in b.files:
            print("ONLY ONE SIDE", k); bad += 1; continue
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            bad += 1
            n = int((x.view(np.uint8) != y.view(np.uint8)).sum()) if x.shape == y.shape and x.dtype == y.dtype else -1
            print(f"DIFF {k}: {n} bytes of {x.nbytes} differ")
    print(f"{pa} vs {pb}: {len(a.files)} arrays, {bad} differ")
    return 1 if bad else 0


if sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))
import torch
import mpcqp
OUT = {}
def put(name, t):
    if t is None: return
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    OUT[name] = a.copy()
def dev(a, dt): return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()

# ---- solves: tuple, gait (S = 2), gait steps (S = 4)
for io in ("f32", "f64"):
    tdt = torch.float32 if io == "f32" else torch.float64
    for N in (10, 20, 60):
        B = 512 if N == 60 else 4096
        for prec in ("mixed", "f64"):
            tag = f"{io}_N{N}_{prec}"
            sol = mpcqp.MPCBatch(N=N, delta=0.03, io_dtype=io, precision=prec)
            d = sol.upload(mpcqp.synth.make_batch(B, N=N, seed=101, gait_names=("trot", "amble", "gallop"), mus=(0.3, 0.7, 1.0)))
            o = sol.solve_batch(d["x0"], d["r"], d["contact"], d["xdes"], d["mu"], want_X=True)
            torch.cuda.synchronize()
            for k in ("u", "X", "status", "iters", "res"): put(f"solve_{tag}_{k}", o[k])
            for S in (2, 4):
                g = sol.upload_gait(mpcqp.synth.make_gait_batch(B, N=N, seed=202 + S, steps=S))
                o = sol.solve_batch_gait(g["x0"], g["ref"], g["feet0"], g["footholds"], g["gait"], g["feet_id"], g["mu"], want_X=True)
                torch.cuda.synchronize()
                for k in ("u", "X", "status", "iters", "res"): put(f"gait{S}_{tag}_{k}", o[k])
            del sol
    # warm start + shift over three consecutive calls
    sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed", warm_start=True, warm_shift=True)
    d = sol.upload(mpcqp.synth.make_batch(4096, N=10, seed=303, gait_names=("trot", "amble"), mus=(0.5, 1.0)))
    for call in range(3):
        o = sol.solve_batch(d["x0"], d["r"], d["contact"], d["xdes"], d["mu"], want_X=True)
        torch.cuda.synchronize()
        for k in ("u", "X", "status", "iters", "res"): put(f"warm{call}_{io}_{k}", o[k])
    del sol
    print("solves", io, "done", flush=True)

# ---- the stage-wise engine by itself: the reference's horizon, and horizon 10 by MPCQP_FLAG_STAGE_KERNEL; MIXED / F64; cold, and
#      warm-started with shift over three consecutive calls
for N, flags in ((60, mpcqp.FLAG_POLISH), (10, mpcqp.FLAG_POLISH | mpcqp.FLAG_STAGE_KERNEL)):
    B = 256 if N == 60 else 1024
    d0 = mpcqp.synth.make_batch(B, N=N, seed=404, gait_names=("trot", "amble", "gallop"), mus=(0.3, 0.7, 1.0))
    for prec in ("mixed", "f64"):
        for warm in (False, True):
            sol = mpcqp.MPCBatch(N=N, delta=0.03, io_dtype="f64", precision=prec, warm_start=warm, warm_shift=warm, flags=flags)
            d = sol.upload(d0)
            for call in range(3 if warm else 1):
                o = sol.solve_batch(d["x0"], d["r"], d["contact"], d["xdes"], d["mu"], want_X=True)
                torch.cuda.synchronize()
                for k in ("u", "X", "status", "iters", "res"): put(f"stage_N{N}_{prec}_{'warm%d' % call if warm else 'cold'}_{k}", o[k])
            del sol
print("stage engine done", flush=True)

# ---- roll-outs, T = 50, B = 1024, with the malformed plan rows of tests/test_rollout.py
from test_rollout import _malformed
T, B = 50, 1024
rb = mpcqp.synth.make_rollout_batch(B, seed=11)
meta, tick = _malformed(rb)
rows = mpcqp.synth.make_plant_rows(B, seed=12, push_start=(3, 20))
for io in ("f32", "f64"):
    tdt = torch.float32 if io == "f32" else torch.float64
    for warm in (False, True):
        for kind in ("model", "plant", "plant_nopush"):
            sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed", warm_start=warm, warm_shift=warm)
            x, rf, tk = dev(rb["x"], tdt), dev(rb["ref"], tdt), dev(tick, torch.int32)
            args = (x, rf, dev(rb["plan_pos"], tdt), dev(rb["plan_feet_id"], torch.uint8), dev(meta, torch.int32), tk, dev(rb["mu"], tdt), T)
            if kind == "model": o = sol.rollout(*args)
            elif kind == "plant": o = sol.rollout_plant(*args, body=dev(rows["body"], tdt), push=dev(rows["push"], tdt), push_ticks=dev(rows["push_ticks"], torch.int32))
            else: o = sol.rollout_plant(*args, body=dev(rows["body"], tdt))
            torch.cuda.synchronize()
            tag = f"roll_{kind}_{io}_{'warm' if warm else 'cold'}"
            put(tag + "_x", x); put(tag + "_ref", rf); put(tag + "_tick", tk)
            for k in ("actual", "desired", "forces", "solved"): put(f"{tag}_{k}", o[k])
            del sol
    print("roll-outs", io, "done", flush=True)

# ---- planner + swing, plant step, leg Jacobians + torque map: the inputs of their GPU tests
from test_gpu_plant import _plant_inputs
from test_leg_jacobians import _angles
for io in ("f32", "f64"):
    tdt = torch.float32 if io == "f32" else torch.float64
    sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed")
    pi = mpcqp.synth.make_plan_inputs(2048)
    plan = sol.plan_footsteps(dev(pi["feet0"], tdt), dev(pi["cmd"], tdt), dev(pi["gait"], torch.int32), 24, want_ang=True, want_hip=True)
    for k, v in plan.items(): put(f"plan_{io}_{k}", v)
    rng = np.random.default_rng(5)
    tk = rng.integers(-3, 200, 2048).astype(np.int32)
    sw = sol.swing_trajectories(plan, dev(tk, torch.int32), 16, dev(pi["step_height"], tdt))
    put(f"swing_{io}_traj", sw["traj"]); put(f"swing_{io}_des", sw["feet_des"])
    bad = plan["plan_meta"].clone(); bad[0] = torch.tensor([0, 4, 2, 0]); bad[1] = torch.tensor([5, 0, 0, 0]); bad[2] = torch.tensor([99, 4, 2, 0]); bad[3] = torch.tensor([5, -3, -1, 0])
    plan2 = dict(plan); plan2["plan_meta"] = bad
    sw = sol.swing_trajectories(plan2, dev(tk, torch.int32), 16, dev(pi["step_height"], tdt))
    put(f"swingbad_{io}_traj", sw["traj"]); put(f"swingbad_{io}_des", sw["feet_des"])
    p = _plant_inputs(4096, 3)
    dp = {k: dev(v, torch.uint8 if k == "contact" else tdt) for k, v in p.items()}
    for sub in (1, 10):
        put(f"plantstep_{io}_{sub}", sol.plant_step(dp["x"], dp["f"], dp["feet"], dp["contact"], dp["body"], dp["wrench"], sub))
        put(f"plantstep_none_{io}_{sub}", sol.plant_step(dp["x"], dp["f"], dp["feet"], dp["contact"], None, None, sub))
    q, R = _angles(3000, 11)
    tq, tR = dev(q, tdt), dev(R, tdt)
    J, P = sol.leg_jacobians(tq, tR); put(f"jac_{io}_J", J); put(f"jac_{io}_P", P)
    J0, P0 = sol.leg_jacobians(tq, None); put(f"jac0_{io}_J", J0); put(f"jac0_{io}_P", P0)
    u = dev(np.random.default_rng(2).normal(0, 30, (3000, 10, 12)), tdt)
    put(f"tau_{io}", sol.torque_map(u, J))
    torch.cuda.synchronize()
    del sol

# ---- the entry points that came after the ones above and that tools/stance_rule_compare.py does not run: phase_expand, solve_batch_phase,
#      rollout_phase, phase_swing, rollout_legs, joint_log, joint_rates, leg_effort, swing_track, rollout_score, leg_ik, leg_dynamics, leg_accel.
#      Inputs: the legs batch of tests/models_rollout_cases.py (B = 16, T = 25), the joint rows of tests/legsim_cases.py (33), the synthetic
#      logs of tests/score_cases.py (24 x 25), at their own shapes without and with the two row tables (model rows: every solve and roll-out;
#      actuator rows of tests/actuator_cases.py: rollout_legs, swing_track, leg_effort), and tiled and cut to B = 333 (T = 4 for the roll-outs):
#      more than one block of 256 threads and a ragged last one, whether a kernel runs one thread per leg, per robot or per tuple element.
#      Outputs start zero-filled, so a row that a build does not write cannot compare equal by accident.
import actuator_cases as ac, legsim_cases as lc, models_rollout_cases as C, score_cases as scc
import test_gpu_models_rollouts as mr


def puts(prefix, out):
    for k, v in out.items(): put(f"{prefix}_{k}", v)


def zero_filled(sol):
    alloc = sol._alloc
    sol._alloc = lambda stream, *specs: alloc(stream, *[s and (s[0], s[1], True) for s in specs])
    return sol


def tiled(d, B):
    """Every array of d repeated along its first axis and cut to B rows."""
    if d is None or isinstance(d, np.ndarray):
        return d if d is None else np.tile(d, (-(-B // len(d)),) + (1,) * (d.ndim - 1))[:B]
    return {k: (tiled(v, B) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def newer(tag, io, pb, pr, T, rows, acts, q, ops, slog):
    tdt = torch.float32 if io == "f32" else torch.float64
    sol = zero_filled(mr._engine(io))
    if rows is not None:
        sol.set_models(rows); sol.set_actuators(acts)
    plant = mr._plant(sol, pr)
    d = mr._dev(sol, pb)
    phase = [d[k] for k in ("x", "ref", "feet", "gait", "tick", "stand")]
    puts(f"{tag}_expand", sol.phase_expand(*phase, d.get("gain")))
    puts(f"{tag}_solvephase", sol.solve_batch_phase(*phase, d.get("gain"), d["mu"], want_X=True))
    logs = sol.rollout_phase(*[d[k] for k in C.PHASE_ARGS], T, **plant)
    puts(f"{tag}_rollphase", logs); puts(f"{tag}_rollphase_end", {k: d[k] for k in C.PHASE_STATE})
    sw = sol.phase_swing(logs, d["gait"], dev(pb["tick"], torch.int32), d["stand"], d.get("gain"), d["step_height"])
    puts(f"{tag}_phaseswing", sw)
    vel, acc = sw["swing"][:, :, :, 1].contiguous(), sw["swing"][:, :, :, 2].contiguous()
    puts(f"{tag}_jointlog", sol.joint_log(logs["actual"], logs["forces"], sw["feet_des"]))
    puts(f"{tag}_jointrates", sol.joint_rates(logs["actual"], logs["forces"], sw["feet_des"], vel))
    puts(f"{tag}_effort", sol.leg_effort(logs["actual"], logs["forces"], sw["feet_des"], vel, acc, body=plant["body"]))
    puts(f"{tag}_effort_bare", sol.leg_effort(logs["actual"], logs["forces"], sw["feet_des"]))
    state = torch.zeros((len(pb["x"]), 4, 7), dtype=tdt, device="cuda")
    puts(f"{tag}_track", sol.swing_track(logs, sw["swing"], body=plant["body"], state=state)); put(f"{tag}_track_state", state)
    d = mr._dev(sol, pb)
    for land in ("rule", "actual"):
        legs = sol.rollout_legs(*[d[k] for k in C.LEGS_ARGS], T, d["step_height"], land=land, **plant)
        puts(f"{tag}_rolllegs_{land}", legs); puts(f"{tag}_rolllegs_{land}_end", {k: d[k] for k in C.LEGS_ARGS[:4] + ("tick",)})
        put(f"{tag}_score_{land}", sol.score(legs))
    sl = {k: dev(v, torch.uint8 if v.dtype == np.uint8 else tdt) for k, v in slog.items()}
    score = sol.score(sl); put(f"{tag}_score_synthetic", score.clone())
    put(f"{tag}_score_accumulated", sol.score(sl, score=score))
    put(f"{tag}_score_body_only", sol.score({k: sl[k] for k in ("actual", "desired", "forces", "contact_log")}))
    tq, o = dev(q, tdt), {k: dev(v, tdt) for k, v in ops.items()}
    J, P = sol.leg_jacobians(tq, o["rot"])
    for name, (iq, reach) in (("ik", sol.leg_ik(P, o["rot"])), ("ik0", sol.leg_ik(sol.leg_jacobians(tq, None)[1]))):
        put(f"{tag}_{name}_q", iq); put(f"{tag}_{name}_reach", reach)
    dyn = sol.leg_dynamics(tq, o["qd"], o["qdd"], o["rot"], o["base"])
    puts(f"{tag}_dynamics", dyn); puts(f"{tag}_dynamics_bare", sol.leg_dynamics(tq))
    puts(f"{tag}_accel", sol.leg_accel(tq, dyn["tau"], o["qd"], o["rot"], o["base"])); puts(f"{tag}_accel_bare", sol.leg_accel(tq, dyn["tau"]))
    torch.cuda.synchronize()
    if rows is not None:
        sol.clear_actuators(); sol.clear_models()


pb, pr, rows, T = C.legs_case()
acts = ac.combined_tables(len(rows))[0]
q, ops = lc.box_rows()
RAGGED = 333
for io in ("f32", "f64"):
    slog = scc.synthetic_logs(24, 25, 8, np.float32)
    newer(f"new_{io}", io, pb, pr, T, None, None, q, ops, slog)
    newer(f"new_{io}_tables", io, pb, pr, T, rows, acts, q, ops, slog)
    for name, tables in (("ragged", False), ("ragged_tables", True)):
        newer(f"new_{io}_{name}", io, tiled(pb, RAGGED), tiled(pr, RAGGED), 4, tiled(rows, RAGGED) if tables else None, tiled(acts, RAGGED),
              tiled(q, RAGGED), tiled(ops, RAGGED), tiled(slog, RAGGED))
    print("newer entry points", io, "done", flush=True)

# ---- the state estimator: imu_log, estimate_track and rollout_observe with their gated forms, at the shapes of their tests.
#      imu_log: the real case (16 x 25) and every synthetic edge of tests/estimate_cases.py with the edge's own optional operands, and on one
#      edge every combination of base_acc, bias and noise given or not.  estimate_track: the same cases as they come; on the real case and
#      on one edge with and without height, trust and state, in two pieces (13 + 12 rows) through the state, and each of these ungated and
#      gated (tests/gate_cases.py's thresholds); the real case tiled and cut to B = 333.  rollout_observe: the 16 x 25 batch of
#      tests/test_gpu_rollout_observe.py on the ice with its sensor draws, both feeds, with and without the gate and the height rows.
import drive_cases as dc, estimate_cases as ec, gate_cases as gc
import test_gpu_rollout_observe as ro


def est_track(tag, sol, ops, state=True, pieces=False, gate=None):
    tdt = sol.tdtype
    d = {k: (None if v is None else dev(v, torch.uint8 if k == "contact_log" else tdt)) for k, v in ops.items()}
    st = torch.zeros((len(ops["imu"]), 131), dtype=torch.float64, device="cuda") if state else None
    T = ops["imu"].shape[1]
    for name, rows in (("a", slice(0, 13)), ("b", slice(13, T))) if pieces else (("", slice(None)),):
        part = {k: (v[:, rows].contiguous() if v is not None and k in ("imu", "q", "qd", "contact_log", "trust") else v) for k, v in d.items()}
        puts(tag + name, sol.estimate_track(part["imu"], part["q"], part["qd"], part["contact_log"], part["init"], trust=part["trust"],
                                            height=part["height"], state=st, gate=gate))
    put(tag + "_state", st)


for io in ("f32", "f64"):
    tdt = torch.float32 if io == "f32" else torch.float64
    sol = zero_filled(mpcqp.MPCBatch(N=10, delta=ec.DELTA, io_dtype=io))
    cases = [("real", ec.as_io(ec.real_case(), io))] + [("edge_%d_%d" % k[:2], ec.as_io(ec.edge_case(*k), io)) for k in ec.edge_cases()]
    for name, case in cases:
        logs = {k: dev(case[k], tdt) for k in ("actual", "forces", "feet_log")}
        put(f"est_{io}_{name}_imu", sol.imu_log(logs, **{k: (None if v is None else dev(v, tdt)) for k, v in ec.imu_operands(case).items()}))
        est_track(f"est_{io}_{name}_track", sol, ec.operands(case))
    edge = ec.as_io(ec.edge_case(65, 25, True), io)
    logs = {k: dev(edge[k], tdt) for k in ("actual", "forces", "feet_log")}
    for bits in range(8):
        kw = {k: (dev(edge[k], tdt) if bits >> i & 1 else None) for i, k in enumerate(("base_acc", "bias", "noise"))}
        put(f"est_{io}_imu_operands{bits}", sol.imu_log(logs, body=dev(edge["body"], tdt), **kw))
    for name, case in (("real", dict(cases[0][1], trust=edge["trust"][:16], height=edge["height"][:16])), ("edge", edge)):
        for gname, gate in (("", None), ("_gated", gc.GATE)):
            for bits in range(8):
                ops = dict(ec.operands(case), **{k: (case[k] if bits >> i & 1 else None) for i, k in enumerate(("height", "trust"))})
                est_track(f"est_{io}_{name}{gname}_variant{bits}", sol, ops, state=bool(bits & 4), gate=gate)
            est_track(f"est_{io}_{name}{gname}_pieces", sol, ec.operands(case), pieces=True, gate=gate)
    ragged = tiled(dict(cases[0][1], trust=edge["trust"][:16], height=edge["height"][:16]), RAGGED)
    put(f"est_{io}_ragged_imu", sol.imu_log({k: dev(ragged[k], tdt) for k in ("actual", "forces", "feet_log")}, body=dev(ragged["body"], tdt)))
    for gname, gate in (("", None), ("_gated", gc.GATE)):
        est_track(f"est_{io}_ragged{gname}", sol, ec.operands(ragged), gate=gate)
    ops = ro._Ops(io)
    zero_filled(ops.sol)
    for feed in ("truth", "estimate"):
        for gname, gate in (("", None), ("_gated", gc.GATE)):
            for hname, height in (("", None), ("_height", ops.height)):
                st = ops.state()
                tag = f"observe_{io}_{feed}{gname}{hname}"
                puts(tag, ops.observe(st, ro.ROLL_T, feed, inertia=dc.weak_row(0.5), height=height, gate=gate))
                puts(tag + "_end", st)
    torch.cuda.synchronize()
    print("estimator", io, "done", flush=True)
np.savez(sys.argv[1], **OUT)
print("dumped", len(OUT), "arrays", flush=True)
