"""Batched solve surface over the HIP engine (torch is used only for device memory and streams).

``MPCBatch.solve_batch`` is the B>1 counterpart of the reference's ``MPC.solve`` (src/mpc.py:176-303): it
takes the operator tuple that the reference pushes into CasADi with seven ``opt.set_value`` calls
(src/mpc.py:242-255) in compact batched form and returns ``sol.value(U)`` / ``sol.value(X)``
(src/mpc.py:265-268) for every instance, plus per-QP status / iteration / residual outputs.
"""
from __future__ import annotations

import numpy as np

from . import _capi


def _torch():
    import torch
    return torch


class MPCBatch:
    """One engine handle on one GPU.  All tensors live on ``cuda:<device>``; nothing is copied to the host."""

    def __init__(self, N=10, delta=0.03, device=0, io_dtype="f32", precision="mixed", warm_start=False, warm_shift=False,
                 **overrides):
        """``warm_start=True`` sets MPCQP_FLAG_WARM_START: every solve is seeded with the forces already in the output
        buffer -- the previous solve's solution unless ``u_init`` is passed -- like ``opt.set_initial(U, sol.value(U))``
        in the reference (src/mpc.py:270-271)."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise _capi.MpcQpError("MPCBatch needs a GPU: the mpcqp engine has no CPU path")
        lib = _capi.product_library()
        if warm_start:
            overrides["flags"] = int(overrides.get("flags", _capi.FLAG_POLISH)) | _capi.FLAG_WARM_START
            if warm_shift:   # the buffer holds the previous control tick's solution: the engine shifts it (and its duals)
                overrides["flags"] |= _capi.FLAG_WARM_SHIFT
        self.warm_start = bool(warm_start)
        cfg = lib.default_config(N=N, delta=delta, device=device,
                                 dtype={"f32": _capi.DTYPE_F32, "f64": _capi.DTYPE_F64}[io_dtype],
                                 precision={"f32": _capi.PREC_F32, "mixed": _capi.PREC_MIXED, "f64": _capi.PREC_F64}[precision],
                                 **overrides)
        self.N, self.delta = N, delta
        self.device = torch.device("cuda", device)
        self.tdtype = torch.float32 if io_dtype == "f32" else torch.float64
        self.engine = _capi.Engine(lib, cfg)
        self.cfg = cfg
        self._out = {}

    def upload(self, batch):
        """Host numpy batch (mpcqp.synth layout) -> resident device tensors."""
        torch = _torch()
        f = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=self.tdtype).to(self.device).contiguous()
        return {"x0": f(batch["x0"]), "r": f(batch["r"]), "xdes": f(batch["xdes"]), "mu": f(batch["mu"]),
                "contact": torch.as_tensor(np.ascontiguousarray(batch["contact"], dtype=np.uint8)).to(self.device).contiguous()}

    def _outputs(self, B, want_X, st=None):
        torch = _torch()
        key = (B, want_X)
        if key not in self._out:   # allocated once per batch size, reused afterwards
            N = self.N
            # The zero fill below is a kernel on torch's CURRENT stream; the solve that reads the buffer (warm start) or writes it runs
            # on `st`, which may be a non-blocking side stream that nothing orders after it: fill on `st` itself.
            with torch.cuda.stream(st if st is not None else torch.cuda.current_stream(self.device)):
                self._out[key] = {
                    "u": torch.zeros((B, N, 12), dtype=self.tdtype, device=self.device),   # zeros = "no guess" for a warm-started engine
                    "X": torch.empty((B, N + 1, 13), dtype=self.tdtype, device=self.device) if want_X else None,
                    "status": torch.empty(B, dtype=torch.int32, device=self.device),
                    "iters": torch.empty(B, dtype=torch.int32, device=self.device),
                    "res": torch.empty((B, 2), dtype=torch.float32, device=self.device),
                }
        return self._out[key]

    def _seed(self, out, u_init, st):
        if u_init is None:
            return
        if not self.warm_start:
            raise ValueError("u_init needs an engine created with warm_start=True")
        if tuple(u_init.shape) != tuple(out["u"].shape) or u_init.dtype != self.tdtype or u_init.device != self.device:
            raise ValueError(f"u_init must be a {tuple(out['u'].shape)} {self.tdtype} tensor on {self.device}")
        if u_init.data_ptr() != out["u"].data_ptr():
            with _torch().cuda.stream(st):
                out["u"].copy_(u_init)

    def solve_batch(self, x0, r, contact, xdes, mu, want_X=False, stream=None, u_init=None):
        """Asynchronous on ``stream`` (default: torch's current stream); results valid after a stream sync."""
        torch = _torch()
        N = self.N
        B = int(x0.shape[0])
        for t, shape, dt in ((x0, (B, 13), self.tdtype), (r, (B, N, 4, 3), self.tdtype), (contact, (B, N, 4), torch.uint8),
                             (xdes, (B, N + 1, 13), self.tdtype), (mu, (B,), self.tdtype)):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"operand mismatch: expected {shape} {dt} contiguous on {self.device}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        out = self._outputs(B, want_X, st)
        self._seed(out, u_init, st)
        self.engine.solve_batch_ptr(B, x0.data_ptr(), r.data_ptr(), contact.data_ptr(), xdes.data_ptr(), mu.data_ptr(),
                                    out["u"].data_ptr(), out["X"].data_ptr() if want_X else None, out["status"].data_ptr(),
                                    out["iters"].data_ptr(), out["res"].data_ptr(), st.cuda_stream)
        return out

    def set_models(self, models, stream=None):
        """Per-robot model rows (include/mpcqp_model.h, mpcqp_set_models): `models` [B,6] = (m, Ixx, Iyy, Izz, f_min, f_max) per batch
        slot, a float64 tensor on the engine's device or a numpy array (uploaded).  Every later solve, gait solve and roll-out of
        this engine builds QP b from row b and must have B robots; rows are fp64 whatever the I/O dtype (mpcqp.models has the row
        helpers and the host checker).  Asynchronous on `stream`."""
        torch = _torch()
        if not hasattr(models, "data_ptr"):
            models = torch.as_tensor(np.ascontiguousarray(models, dtype=np.float64)).to(self.device)
        if models.dim() != 2 or models.shape[1] != 6 or models.shape[0] < 1 or models.dtype != torch.float64 or not models.is_contiguous() \
                or models.device != self.device:
            raise ValueError(f"models must be a contiguous [B,6] float64 tensor on {self.device}, got {tuple(models.shape)} {models.dtype} on {models.device}")
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        models.record_stream(st)   # (the conversion kernel reads it on `st`; the engine keeps its own table)
        self.engine.set_models_ptr(int(models.shape[0]), models.data_ptr(), st.cuda_stream)

    def clear_models(self):
        """Back to the configuration's model for every QP (mpcqp_clear_models; waits for the device)."""
        self.engine.clear_models()

    def upload_gait(self, g):
        """Host numpy gait descriptors (mpcqp.synth.make_gait_batch layout) -> resident device tensors."""
        torch = _torch()
        f = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=self.tdtype).to(self.device).contiguous()
        return {"x0": f(g["x0"]), "ref": f(g["ref"]), "feet0": f(g["feet0"]), "footholds": f(g["footholds"]), "mu": f(g["mu"]),
                "gait": torch.as_tensor(np.ascontiguousarray(g["gait"], dtype=np.int32)).to(self.device).contiguous(),
                "feet_id": torch.as_tensor(np.ascontiguousarray(g["feet_id"], dtype=np.uint8)).to(self.device).contiguous()}

    def solve_batch_gait(self, x0, ref, feet0, footholds, gait, feet_id, mu, want_X=False, stream=None, u_init=None):
        """Gait entry point: contact masks, stance lever arms and x_des are generated on the device (include/mpcqp.h) from S plan steps
        per robot (footholds [B,S,4,3], feet_id [B,S,4]; S = 2 is the original two-step form)."""
        torch = _torch()
        N = self.N
        B = int(x0.shape[0])
        S = int(footholds.shape[1]) if footholds.dim() == 4 else -1
        for t, shape, dt in ((x0, (B, 13), self.tdtype), (ref, (B, 10), self.tdtype), (feet0, (B, 4, 3), self.tdtype),
                             (footholds, (B, S, 4, 3), self.tdtype), (gait, (B, 4), torch.int32), (feet_id, (B, S, 4), torch.uint8),
                             (mu, (B,), self.tdtype)):
            if S < 1 or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"operand mismatch: expected {shape} {dt} contiguous on {self.device}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        out = self._outputs(B, want_X, st)
        self._seed(out, u_init, st)
        self.engine.solve_batch_gait_steps_ptr(B, S, x0.data_ptr(), ref.data_ptr(), feet0.data_ptr(), footholds.data_ptr(), gait.data_ptr(),
                                               feet_id.data_ptr(), mu.data_ptr(), out["u"].data_ptr(),
                                               out["X"].data_ptr() if want_X else None, out["status"].data_ptr(),
                                               out["iters"].data_ptr(), out["res"].data_ptr(), st.cuda_stream)
        return out

    def rollout(self, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T, log=True, stream=None):
        """Closed-loop roll-out of B robots over T control ticks on the device (include/mpcqp.h, mpcqp_rollout): `x`, `ref` and `tick`
        are advanced IN PLACE; returns the per-tick logs (the reference log's TRACKING PERFORMANCE actual / desired rows and stage-0
        FORCES, src/logger.py:22-46) and the per-robot count of solved ticks."""
        torch = _torch()
        B, S = int(plan_pos.shape[0]), int(plan_pos.shape[1])
        for t, shape, dt in ((x, (B, 13), self.tdtype), (ref, (B, 10), self.tdtype), (plan_pos, (B, S, 4, 3), self.tdtype),
                             (plan_feet_id, (B, S, 4), torch.uint8), (plan_meta, (B, 4), torch.int32), (tick, (B,), torch.int32),
                             (mu, (B,), self.tdtype)):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"operand mismatch: expected {shape} {dt} contiguous on {self.device}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        mk = lambda: torch.empty((B, T, 12), dtype=self.tdtype, device=self.device) if log else None
        actual, desired, forces = mk(), mk(), mk()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        # (the advance kernel initialises `solved` at the first tick, on `st`; a zero fill here would run on torch's current stream)
        solved = (torch.empty if T > 0 else torch.zeros)(B, dtype=torch.int32, device=self.device)
        p = lambda t: t.data_ptr() if t is not None else None
        self.engine.rollout_ptr(B, T, S, x.data_ptr(), ref.data_ptr(), plan_pos.data_ptr(), plan_feet_id.data_ptr(), plan_meta.data_ptr(),
                                tick.data_ptr(), mu.data_ptr(), p(actual), p(desired), p(forces), solved.data_ptr(), st.cuda_stream)
        return {"actual": actual, "desired": desired, "forces": forces, "solved": solved}

    def _check_plant_rows(self, B, body, extra):
        torch = _torch()
        rows = [(body, (B, 7), self.tdtype)] + extra
        for t, shape, dt in rows:
            if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device):
                raise ValueError(f"operand mismatch: expected {shape} {dt} contiguous on {self.device}, got {tuple(t.shape)} {t.dtype} on {t.device}")

    def plant_step(self, x, f, feet, contact, body=None, wrench=None, substeps=10, stream=None):
        """One control period of the rigid-body plant for B robots (include/mpcqp_sim.h, mpcqp_plant_step): x [B,13], f [B,12] foot
        forces held over the tick, feet [B,4,3] world foot positions, contact uint8 [B,4] (nonzero = stance), body [B,7] (m, Ixx, Iyy,
        Izz, Ixy, Ixz, Iyz; None = the engine's model), wrench [B,6] (force, torque about the CoM; None = no push).  Returns a new
        [B,13] tensor; asynchronous on `stream`.  The host checker is plant.srb_step."""
        torch = _torch()
        B = int(x.shape[0])
        for t, shape, dt in ((x, (B, 13), self.tdtype), (f, (B, 12), self.tdtype), (feet, (B, 4, 3), self.tdtype), (contact, (B, 4), torch.uint8)):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"operand mismatch: expected {shape} {dt} contiguous on {self.device}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        self._check_plant_rows(B, body, [(wrench, (B, 6), self.tdtype)])
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            out = torch.empty((B, 13), dtype=self.tdtype, device=self.device)
        p = lambda t: t.data_ptr() if t is not None else 0
        self.engine.plant_step_ptr(B, x.data_ptr(), f.data_ptr(), feet.data_ptr(), contact.data_ptr(), p(body), p(wrench), substeps,
                                   out.data_ptr(), st.cuda_stream)
        return out

    def rollout_plant(self, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T, body=None, push=None, push_ticks=None, substeps=10,
                      log=True, stream=None):
        """`rollout` with the world step x <- X[:,1] replaced by the rigid-body plant (include/mpcqp_sim.h, mpcqp_rollout_plant):
        body [B,7] per-robot mass and torso-frame inertia (None = the engine's model), push [B,6] a world-frame wrench acting on the
        robot's own ticks push_ticks[b][0] <= tick < push_ticks[b][1] (int32 [B,2], required with push).  Same in-place advance of
        `x`, `ref` and `tick`, same logs and `solved` count as `rollout`."""
        torch = _torch()
        B, S = int(plan_pos.shape[0]), int(plan_pos.shape[1])
        for t, shape, dt in ((x, (B, 13), self.tdtype), (ref, (B, 10), self.tdtype), (plan_pos, (B, S, 4, 3), self.tdtype),
                             (plan_feet_id, (B, S, 4), torch.uint8), (plan_meta, (B, 4), torch.int32), (tick, (B,), torch.int32),
                             (mu, (B,), self.tdtype)):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"operand mismatch: expected {shape} {dt} contiguous on {self.device}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        self._check_plant_rows(B, body, [(push, (B, 6), self.tdtype), (push_ticks, (B, 2), torch.int32)])
        mk = lambda: torch.empty((B, T, 12), dtype=self.tdtype, device=self.device) if log else None
        actual, desired, forces = mk(), mk(), mk()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        solved = (torch.empty if T > 0 else torch.zeros)(B, dtype=torch.int32, device=self.device)
        p = lambda t: t.data_ptr() if t is not None else None
        self.engine.rollout_plant_ptr(B, T, S, x.data_ptr(), ref.data_ptr(), plan_pos.data_ptr(), plan_feet_id.data_ptr(),
                                      plan_meta.data_ptr(), tick.data_ptr(), mu.data_ptr(), p(body), p(push), p(push_ticks), substeps,
                                      p(actual), p(desired), p(forces), solved.data_ptr(), st.cuda_stream)
        return {"actual": actual, "desired": desired, "forces": forces, "solved": solved}

    def plan_footsteps(self, feet0, cmd, gait, S, want_ang=True, want_hip=False, stream=None):
        """Footstep plans of B robots on the device (include/mpcqp_plan.h, mpcqp_plan_footsteps; the host FootstepPlanner per robot):
        feet0 [B,4,3] initial feet FL, FR, HL, HR and cmd [B,5] (yaw0, v_com_ref x, v_com_ref y, theta_dot, h) of the engine's dtype,
        gait int32 [B,4] (total_steps, ss, ds, first_swing bit mask; bit k = leg k stays down in step 1).  Returns device tensors
        plan_pos [B,S,4,3], plan_feet_id uint8 [B,S,4] and plan_meta int32 [B,4] -- the plan arguments of `rollout` -- plus plan_ang
        [B,S] and plan_hip [B,S,3] when asked for (None otherwise).  The tick length is the engine's delta; asynchronous on `stream`."""
        torch = _torch()
        B, S = int(feet0.shape[0]), int(S)
        for t, shape, dt in ((feet0, (B, 4, 3), self.tdtype), (cmd, (B, 5), self.tdtype), (gait, (B, 4), torch.int32)):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"operand mismatch: expected {shape} {dt} contiguous on {self.device}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        if S < 1:
            raise ValueError(f"S must be >= 1, got {S}")
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            e = lambda *shape: torch.empty(shape, dtype=self.tdtype, device=self.device)
            out = {"plan_pos": e(B, S, 4, 3), "plan_feet_id": torch.empty((B, S, 4), dtype=torch.uint8, device=self.device),
                   "plan_meta": torch.empty((B, 4), dtype=torch.int32, device=self.device),
                   "plan_ang": e(B, S) if want_ang else None, "plan_hip": e(B, S, 3) if want_hip else None}
        p = lambda t: t.data_ptr() if t is not None else 0
        self.engine.plan_footsteps_ptr(B, S, feet0.data_ptr(), cmd.data_ptr(), gait.data_ptr(), out["plan_pos"].data_ptr(),
                                       out["plan_feet_id"].data_ptr(), out["plan_meta"].data_ptr(), p(out["plan_ang"]), p(out["plan_hip"]),
                                       st.cuda_stream)
        return out

    def swing_trajectories(self, plan, tick, K, step_height, want_des=True, stream=None):
        """Swing-foot trajectories of every leg at ticks tick[b] + j, j < K (include/mpcqp_plan.h, mpcqp_swing_trajectories; the host
        FootTrajectoryGenerator per robot, leg and tick): `plan` as returned by `plan_footsteps` (plan_ang required), tick int32 [B],
        step_height [B] of the engine's dtype.  Returns {"traj": [B,K,4,3,6] pos / vel / acc 6-vectors (angle xyz, position xyz),
        "feet_des": [B,K,4,3] the closed-loop log's desired foot positions, or None}.  Asynchronous on `stream`."""
        torch = _torch()
        pos, fid, meta, ang = plan["plan_pos"], plan["plan_feet_id"], plan["plan_meta"], plan.get("plan_ang")
        if ang is None:
            raise ValueError("swing_trajectories needs plan['plan_ang'] (plan_footsteps(..., want_ang=True))")
        B, S, K = int(pos.shape[0]), int(pos.shape[1]) if pos.dim() == 4 else -1, int(K)
        for t, shape, dt in ((pos, (B, S, 4, 3), self.tdtype), (fid, (B, S, 4), torch.uint8), (meta, (B, 4), torch.int32),
                             (ang, (B, S), self.tdtype), (tick, (B,), torch.int32), (step_height, (B,), self.tdtype)):
            if S < 1 or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"operand mismatch: expected {shape} {dt} contiguous on {self.device}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        if K < 0:
            raise ValueError(f"K must be >= 0, got {K}")
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            traj = torch.empty((B, K, 4, 3, 6), dtype=self.tdtype, device=self.device)
            des = torch.empty((B, K, 4, 3), dtype=self.tdtype, device=self.device) if want_des else None
        self.engine.swing_trajectories_ptr(B, K, S, pos.data_ptr(), fid.data_ptr(), meta.data_ptr(), ang.data_ptr(), tick.data_ptr(),
                                           step_height.data_ptr(), traj.data_ptr(), des.data_ptr() if des is not None else 0, st.cuda_stream)
        return {"traj": traj, "feet_des": des}

    def torque_map(self, u, jac, stream=None):
        """tau[B,4,3] = J^T (-f) of the stage-0 forces (src/main.py:212-214); jac[B,4,3,3] world-frame leg Jacobians."""
        torch = _torch()
        B = int(u.shape[0])
        if tuple(jac.shape) != (B, 4, 3, 3) or jac.dtype != self.tdtype or u.dtype != self.tdtype or not jac.is_contiguous():
            raise ValueError("jac must be a contiguous [B,4,3,3] tensor of the engine's dtype")
        tau = torch.empty((B, 4, 3), dtype=self.tdtype, device=self.device)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.engine.torque_map_ptr(B, u.data_ptr(), jac.data_ptr(), tau.data_ptr(), st.cuda_stream)
        return tau

    def leg_jacobians(self, q, rot=None, geometry=None, want_foot=True, stream=None):
        """World-frame 3x3 linear Jacobian block of each foot w.r.t. its leg's joints (what src/main.py:205-210 asks DART for), on the
        device: q [B,4,3] joint angles (HipX, HipY, Knee per leg), rot [B,3,3] torso orientation or None -> (jac [B,4,3,3], foot [B,4,3])."""
        torch = _torch()
        B = int(q.shape[0])
        if tuple(q.shape) != (B, 4, 3) or q.dtype != self.tdtype or not q.is_contiguous():
            raise ValueError("q must be a contiguous [B,4,3] tensor of the engine's dtype")
        if rot is not None and (tuple(rot.shape) != (B, 3, 3) or rot.dtype != self.tdtype or not rot.is_contiguous()):
            raise ValueError("rot must be a contiguous [B,3,3] tensor of the engine's dtype")
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            jac = torch.empty((B, 4, 3, 3), dtype=self.tdtype, device=self.device)
            foot = torch.empty((B, 4, 3), dtype=self.tdtype, device=self.device) if want_foot else None
        self.engine.leg_jacobians_ptr(B, q.data_ptr(), rot.data_ptr() if rot is not None else 0, jac.data_ptr(),
                                      foot.data_ptr() if foot is not None else 0, geometry, st.cuda_stream)
        return jac, foot

    def _check_rows(self, rows):
        for name, t, shape in rows:
            if t is not None and (tuple(t.shape) != shape or t.dtype != self.tdtype or not t.is_contiguous() or t.device != self.device):
                raise ValueError(f"{name} must be a contiguous {shape} {self.tdtype} tensor on {self.device}, got {tuple(t.shape)} {t.dtype} on {t.device}")

    def leg_ik(self, foot, rot=None, origin=None, geometry=None, want_reach=True, stream=None):
        """Closed-form inverse kinematics of the four legs on the device (include/mpcqp_joints.h, mpcqp_leg_ik; the host counterpart is
        lite3_model.leg_ik_closed): foot [B,4,3] foot positions in world orientation, rot [B,3,3] torso orientation (world <- torso) or
        None, origin [B,3] torso origin or None -> (q [B,4,3] HipX, HipY, Knee, reach uint8 [B,4] or None).  With rot and origin None
        this inverts the `foot` output of `leg_jacobians`.  Out of reach: q of the nearest boundary and reach = 0; a non-finite leg:
        NaN and 0.  Asynchronous on `stream`."""
        torch = _torch()
        B = int(foot.shape[0])
        self._check_rows([("foot", foot, (B, 4, 3)), ("rot", rot, (B, 3, 3)), ("origin", origin, (B, 3))])
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            q = torch.empty((B, 4, 3), dtype=self.tdtype, device=self.device)
            reach = torch.empty((B, 4), dtype=torch.uint8, device=self.device) if want_reach else None
        p = lambda t: t.data_ptr() if t is not None else 0
        self.engine.leg_ik_ptr(B, foot.data_ptr(), p(rot), p(origin), q.data_ptr(), p(reach), geometry, st.cuda_stream)
        return q, reach

    def joint_log(self, actual, forces, feet, geometry=None, stream=None):
        """Joint-space log of a roll-out on the device (include/mpcqp_joints.h, mpcqp_joint_log; the host counterpart is
        lite3_model.joint_log_host): actual, forces [B,T,12] as `rollout` / `rollout_plant` return them, feet [B,T,4,3] world foot
        positions -- `swing_trajectories(plan, first_tick, K=T, ...)["feet_des"]` -> {"q": [B,T,4,3] joint angles, "tau": [B,T,4,3]
        joint torques (R J)^T (-f), "reach": uint8 [B,T,4]}.  Asynchronous on `stream`."""
        torch = _torch()
        B, T = int(actual.shape[0]), int(actual.shape[1]) if actual.dim() == 3 else -1
        self._check_rows([("actual", actual, (B, T, 12)), ("forces", forces, (B, T, 12)), ("feet", feet, (B, T, 4, 3))])
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            q = torch.empty((B, T, 4, 3), dtype=self.tdtype, device=self.device)
            tau = torch.empty((B, T, 4, 3), dtype=self.tdtype, device=self.device)
            reach = torch.empty((B, T, 4), dtype=torch.uint8, device=self.device)
        self.engine.joint_log_ptr(B, T, actual.data_ptr(), forces.data_ptr(), feet.data_ptr(), q.data_ptr(), tau.data_ptr(), reach.data_ptr(),
                                  geometry, st.cuda_stream)
        return {"q": q, "tau": tau, "reach": reach}

    def last_kernel_ms(self):
        return self.engine.last_kernel_ms()
