"""Every MPCBatch entry point on torch's current stream and on a side stream: the same bits.  The outputs of a call are allocated
with the call's stream current (engine.MPCBatch._alloc), whichever stream that is."""
import numpy as np
import pytest

import mpcqp
from mpcqp import synth
from test_gpu_joint_log import _synthetic
from test_gpu_plant import _plant_inputs
from test_leg_jacobians import _angles

B, T, S = 65, 3, 2      # one robot more than a wave


def _inputs(sol):
    """Device operands of every entry point, built once on the current stream."""
    import torch
    dt = sol.tdtype
    t = lambda a, d=dt: torch.as_tensor(np.ascontiguousarray(a), dtype=d).cuda().contiguous()
    inp = {"tuple": sol.upload(synth.make_batch(B, N=sol.N, seed=65, gait_names=("trot", "amble", "gallop"), mus=(0.3, 0.7, 1.0))),
           "gait": sol.upload_gait(synth.make_gait_batch(B, N=sol.N, seed=66, steps=S))}
    rb = synth.make_rollout_batch(B, seed=67, total_steps=S)
    rows = synth.make_plant_rows(B, seed=68, push_start=(0, 1), push_len=(1, 2))
    inp["roll"] = {k: t(rb[k], {"plan_feet_id": torch.uint8, "plan_meta": torch.int32, "tick": torch.int32}.get(k, dt))
                   for k in ("x", "ref", "plan_pos", "plan_feet_id", "plan_meta", "tick", "mu")}
    inp["rows"] = {"body": t(rows["body"]), "push": t(rows["push"]), "push_ticks": t(rows["push_ticks"], torch.int32)}
    p = _plant_inputs(B, 69)
    inp["plant"] = {k: t(v, torch.uint8 if k == "contact" else dt) for k, v in p.items()}
    pi = synth.make_plan_inputs(B, seed=70)
    inp["plan"] = {"feet0": t(pi["feet0"]), "cmd": t(pi["cmd"]), "gait": t(pi["gait"], torch.int32), "step_height": t(pi["step_height"]),
                   "tick": t(np.random.default_rng(71).integers(0, 12, B), torch.int32)}
    q, R = _angles(B, 72)
    inp["q"], inp["rot"] = t(q), t(R)
    inp["u"] = t(np.random.default_rng(73).normal(0.0, 30.0, (B, sol.N, 12)))
    s = _synthetic(B, T)
    inp["log"] = {k: t(s[k]) for k in ("actual", "forces", "feet")}
    torch.cuda.synchronize()
    return inp


def _every_call(sol, inp, stream):
    """Each entry point once on `stream`; fresh clones of the operands a roll-out advances in place.  Returns {name: host array}."""
    import torch
    got = {}

    def keep(name, out):
        torch.cuda.synchronize()
        items = out.items() if isinstance(out, dict) else enumerate(out) if isinstance(out, tuple) else [("", out)]
        got.update({f"{name}.{k}": v.cpu().numpy().copy() for k, v in items if v is not None})
        return out

    d, g, r, pl = inp["tuple"], inp["gait"], inp["roll"], inp["plan"]
    keep("solve_batch", sol.solve_batch(d["x0"], d["r"], d["contact"], d["xdes"], d["mu"], want_X=True, stream=stream))
    keep("solve_batch_gait", sol.solve_batch_gait(g["x0"], g["ref"], g["feet0"], g["footholds"], g["gait"], g["feet_id"], g["mu"],
                                                  want_X=True, stream=stream))
    for name, kw in (("rollout", {}), ("rollout_plant", inp["rows"])):
        x, ref, tick = r["x"].clone(), r["ref"].clone(), r["tick"].clone()
        torch.cuda.synchronize()
        out = getattr(sol, name)(x, ref, r["plan_pos"], r["plan_feet_id"], r["plan_meta"], tick, r["mu"], T, stream=stream, **kw)
        keep(name, dict(out, x=x, ref=ref, tick=tick))
    p = inp["plant"]
    keep("plant_step", sol.plant_step(p["x"], p["f"], p["feet"], p["contact"], p["body"], p["wrench"], stream=stream))
    plan = keep("plan_footsteps", sol.plan_footsteps(pl["feet0"], pl["cmd"], pl["gait"], S, want_hip=True, stream=stream))
    keep("swing_trajectories", sol.swing_trajectories(plan, pl["tick"], T, pl["step_height"], stream=stream))
    jac, foot = keep("leg_jacobians", sol.leg_jacobians(inp["q"], inp["rot"], stream=stream))
    keep("torque_map", sol.torque_map(inp["u"], jac, stream=stream))
    keep("leg_ik", sol.leg_ik(foot, inp["rot"], stream=stream))
    keep("joint_log", sol.joint_log(inp["log"]["actual"], inp["log"]["forces"], inp["log"]["feet"], stream=stream))
    return got


@pytest.mark.gpu
def test_a_side_stream_gives_the_bits_of_the_current_stream():
    import torch
    sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed")
    inp = _inputs(sol)
    here = _every_call(sol, inp, None)
    sol._out.clear()                                   # (so that the two solves allocate their outputs on the side stream as well)
    there = _every_call(sol, inp, torch.cuda.Stream())
    assert len(here) >= 30 and here.keys() == there.keys()
    assert np.all(here["rollout.tick"] == T) and here["rollout.solved"].max() == T and here["rollout.forces"].any()   # (work was done)
    differ = [k for k in here if here[k].shape != there[k].shape or here[k].tobytes() != there[k].tobytes()]
    assert not differ, differ
