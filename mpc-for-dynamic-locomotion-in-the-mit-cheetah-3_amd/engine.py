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


def check_operands(device, rows, optional=()):
    """The operand check of every MPCBatch method.  Each row (name, tensor, shape, dtype) must be a contiguous tensor of that shape
    and dtype on `device`; a None tensor passes only where its name is in `optional`."""
    for name, t, shape, dt in rows:
        if t is None and name in optional:
            continue
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dt or not t.is_contiguous() or t.device != device:
            got = "None" if t is None else f"{tuple(t.shape)} {t.dtype}{'' if t.is_contiguous() else ' non-contiguous'} on {t.device}"
            raise ValueError(f"operand mismatch: {name} expected {tuple(shape)} {dt} contiguous on {device}, got {got}")


def _ptr(t):
    """Address of a tensor, or null for None."""
    return t.data_ptr() if t is not None else 0


_NO_DRIVE = object()      # MPCBatch._rollout_legs: the entry point takes no drive mode (a caller's drive=None is a wrong mode, not this)


class MPCBatch:
    """One engine handle on one GPU.  All tensors live on ``cuda:<device>``; nothing is copied to the host."""

    def __init__(self, N=10, delta=0.03, device=0, io_dtype="f32", precision="mixed", warm_start=False, warm_shift=False, library=None,
                 **overrides):
        """``warm_start=True`` sets MPCQP_FLAG_WARM_START: every solve is seeded with the forces already in the output
        buffer -- the previous solve's solution unless ``u_init`` is passed -- like ``opt.set_initial(U, sol.value(U))``
        in the reference (src/mpc.py:270-271).  `library`: another build of the product library (a `_capi.Library`) instead of the
        in-tree one, for tools that compare builds."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise _capi.MpcQpError("MPCBatch needs a GPU: the mpcqp engine has no CPU path")
        lib = library or _capi.product_library()
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

    def _stream(self, stream):
        """The stream a call runs on: the caller's, or torch's current stream."""
        return stream if stream is not None else _torch().cuda.current_stream(self.device)

    def _alloc(self, stream, *specs):
        """Every output tensor is created here, with the call's stream current: the caching allocator ties a block to the stream that
        is current when it is handed out, and may hand it out again while kernels on any other stream still write it.  `stream` is the
        caller's argument (None = torch's current stream: nothing to switch).  A spec is (shape, dtype) for an uninitialised tensor,
        (shape, dtype, True) for one zero-filled on that stream, or None for an output that was not asked for."""
        torch = _torch()
        with torch.cuda.stream(stream):
            new = lambda shape, dt, zero=False: (torch.zeros if zero else torch.empty)(shape, dtype=dt, device=self.device)
            return [s and new(*s) for s in specs]

    def _upload(self, host, floats, ints):
        """Host numpy arrays -> resident device tensors: the keys `floats` in the engine's dtype, the keys of `ints` in theirs."""
        torch = _torch()
        f = lambda a, npdt, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=npdt), dtype=dt).to(self.device).contiguous()
        return {**{k: f(host[k], None, self.tdtype) for k in floats}, **{k: f(host[k], npdt, None) for k, npdt in ints.items()}}

    def upload(self, batch):
        """Host numpy batch (mpcqp.synth layout) -> resident device tensors."""
        return self._upload(batch, ("x0", "r", "xdes", "mu"), {"contact": np.uint8})

    def upload_gait(self, g):
        """Host numpy gait descriptors (mpcqp.synth.make_gait_batch layout) -> resident device tensors."""
        return self._upload(g, ("x0", "ref", "feet0", "footholds", "mu"), {"gait": np.int32, "feet_id": np.uint8})

    def _outputs(self, B, want_X, stream):
        torch = _torch()
        key = (B, want_X)
        if key not in self._out:   # allocated once per batch size, reused afterwards
            N = self.N
            u, X, status, iters, res = self._alloc(
                stream, ((B, N, 12), self.tdtype, True),   # zeros = "no guess" for a warm-started engine
                ((B, N + 1, 13), self.tdtype) if want_X else None, ((B,), torch.int32), ((B,), torch.int32), ((B, 2), torch.float32))
            self._out[key] = {"u": u, "X": X, "status": status, "iters": iters, "res": res}
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

    def _solve(self, call, sizes, inputs, want_X, stream, u_init):
        """What the two solves share: the cached outputs, the seed, the call (sizes, input addresses, output addresses, stream)."""
        st = self._stream(stream)
        out = self._outputs(sizes[0], want_X, stream)
        self._seed(out, u_init, st)
        call(*sizes, *[t.data_ptr() for t in inputs], out["u"].data_ptr(), _ptr(out["X"]), out["status"].data_ptr(),
             out["iters"].data_ptr(), out["res"].data_ptr(), st.cuda_stream)
        return out

    def solve_batch(self, x0, r, contact, xdes, mu, want_X=False, stream=None, u_init=None):
        """Asynchronous on ``stream`` (default: torch's current stream); results valid after a stream sync."""
        torch = _torch()
        N = self.N
        B = int(x0.shape[0])
        check_operands(self.device, (("x0", x0, (B, 13), self.tdtype), ("r", r, (B, N, 4, 3), self.tdtype),
                                     ("contact", contact, (B, N, 4), torch.uint8), ("xdes", xdes, (B, N + 1, 13), self.tdtype),
                                     ("mu", mu, (B,), self.tdtype)))
        return self._solve(self.engine.solve_batch_ptr, (B,), (x0, r, contact, xdes, mu), want_X, stream, u_init)

    def set_models(self, models, stream=None):
        """Per-robot model rows (include/mpcqp_model.h, mpcqp_set_models): `models` [B,6] = (m, Ixx, Iyy, Izz, f_min, f_max) per batch
        slot, a float64 tensor on the engine's device or a numpy array (uploaded).  Every later `solve_batch`, `solve_batch_gait`,
        `solve_batch_phase`, `rollout`, `rollout_plant`, `rollout_phase`, `rollout_legs` and `rollout_drive` of this engine builds
        QP b -- on every tick -- from row b and must have B robots; rows are fp64 whatever the I/O dtype (mpcqp.models has the row
        helpers and the host checkers).  The row is the MPC's model only: the plant (`rollout_*`, `plant_step`), the legs step of
        `rollout_legs` / `rollout_drive`, `leg_effort` and `swing_track` take `body`, and with body=None the CONFIGURATION's model,
        whatever the table says (a matched plant is body[b] = (m, Ixx, Iyy, Izz, 0, 0, 0) of row b).  Asynchronous on `stream`."""
        self._set_rows(self.engine.set_models_ptr, "models", models, 6, stream)

    def _set_rows(self, set_ptr, name, rows, width, stream):
        """`set_models` / `set_actuators`: a float64 [B,width] table, uploaded when it is a numpy array, handed to the library on `stream`."""
        torch = _torch()
        if not hasattr(rows, "data_ptr"):
            rows = torch.as_tensor(np.ascontiguousarray(rows, dtype=np.float64)).to(self.device)
        B = int(rows.shape[0]) if rows.dim() == 2 else 0
        check_operands(self.device, [(name, rows, (max(B, 1), width), torch.float64)])   # (at least one row)
        st = self._stream(stream)
        rows.record_stream(st)   # (the conversion kernel reads it on `st`; the engine keeps its own table)
        set_ptr(B, rows.data_ptr(), st.cuda_stream)

    def clear_models(self):
        """Back to the configuration's model for every QP (mpcqp_clear_models; waits for the device)."""
        self.engine.clear_models()

    def set_actuators(self, rows, stream=None):
        """Per-robot actuator rows with a torque-speed curve (include/mpcqp_actuators.h, mpcqp_set_actuators, which has the envelope):
        `rows` [B,9] = (tau_max[3], qd_knee[3], qd_free[3]) of HipX, HipY, Knee per robot, a float64 tensor on the engine's device or a
        numpy array (uploaded); mpcqp.actuators has the row helpers and the host counterpart.  Every later `swing_track`, `leg_effort`,
        `stance_drive`, `rollout_legs` and `rollout_drive` of this engine clamps robot b's joint torques at row b's envelope -- the
        tau_max of `inertia` is then ignored -- and must have B robots; `stance_drive` on the B T logged rows of a roll-out wants the
        table tiled (actuators.tile).  A table of flat rows with the inertia row's tau_max (actuators.actuator_rows(B)) is no table, bit
        for bit.  The MPC is not told.  Asynchronous on `stream`."""
        self._set_rows(self.engine.set_actuators_ptr, "rows", rows, 9, stream)

    def clear_actuators(self):
        """Back to the inertia row's tau_max for every clamp (mpcqp_clear_actuators; waits for the device)."""
        self.engine.clear_actuators()

    def set_disturbance(self, rows, stream=None):
        """Per-robot disturbance wrench rows (include/mpcqp_disturb.h, mpcqp_set_disturbance, which has the rule): `rows` [B,6] =
        (F_x, F_y, F_z, tau_x, tau_y, tau_z), a world-frame force at the CoM and torque about it -- the layout of a `push` row --, a
        float64 tensor on the engine's device or a numpy array (uploaded); mpcqp.disturbance has the row helper and the host
        counterparts.  Every later solve and every tick of every roll-out of this engine plans robot b under row b (xdes - s goes into
        the solve, s is added to "X") and must have B robots.  The plant is not told: its push stays `push`.  Asynchronous on `stream`."""
        self._set_rows(self.engine.set_disturbance_ptr, "rows", rows, 6, stream)

    def clear_disturbance(self):
        """Back to no disturbance for every QP (mpcqp_clear_disturbance; waits for the device)."""
        self.engine.clear_disturbance()

    def disturbance_shift(self, x0, xdes, stream=None):
        """The shift kernel alone (include/mpcqp_disturb.h, mpcqp_disturbance_shift; the host counterpart is disturbance.shift_host):
        x0 [B,13], xdes [B,N+1,13] -> xdes - s [B,N+1,13] under the table that is set (an error without one).  Asynchronous on `stream`."""
        B, N = int(x0.shape[0]), self.N
        check_operands(self.device, (("x0", x0, (B, 13), self.tdtype), ("xdes", xdes, (B, N + 1, 13), self.tdtype)))
        st = self._stream(stream)
        out, = self._alloc(stream, ((B, N + 1, 13), self.tdtype))
        self.engine.disturbance_shift_ptr(B, x0.data_ptr(), xdes.data_ptr(), out.data_ptr(), st.cuda_stream)
        return out

    def disturbance_track(self, logs, body=None, observer=None, state=None, feet="feet_log", want=("dist", "resid"), stream=None):
        """The wrench observer over the rows of a roll-out's logs (include/mpcqp_disturb.h, mpcqp_disturbance_track, which has the rule;
        the host counterpart is disturbance.disturbance_track_host): `logs` with "actual", "forces" [B,T,12] and logs[feet] [B,T,4,3] --
        the plant's truth, or a dict made of the "est" and "cmd" logs of `rollout_observe` under those names; body [B,7] or None (the
        engine's model); `observer` None, a dict of disturbance.observer_row's fields or an MpcQpWrenchObserver; state float64 [B,40]
        advanced IN PLACE (zeros: a fresh observer) or None (a fresh one is made) -> {"dist", "resid" [B,T,6], "state"}; an output not
        in `want` is None.  Asynchronous on `stream`."""
        from . import disturbance as _dist
        torch = _torch()
        actual = logs.get("actual")
        if actual is None or actual.dim() != 3:
            raise ValueError("disturbance_track needs the logs of a roll-out run with log=True")
        B, T = int(actual.shape[0]), int(actual.shape[1])
        rows = ((B, T, 6), self.tdtype)
        check_operands(self.device, (("actual", actual, (B, T, 12), self.tdtype), ("forces", logs.get("forces"), (B, T, 12), self.tdtype),
                                     (feet, logs.get(feet), (B, T, 4, 3), self.tdtype), ("body", body, (B, 7), self.tdtype),
                                     ("state", state, (B, _capi.DIST_STATE), torch.float64)), optional=("body", "state"))
        unknown = set(want) - set(_dist.OUT)
        if unknown or not want:
            raise ValueError(f"want must name at least one of {_dist.OUT}, got {tuple(want)}")
        st = self._stream(stream)
        if state is None:
            state, = self._alloc(stream, ((B, _capi.DIST_STATE), torch.float64, True))
        dist, resid = self._alloc(stream, *[rows if k in want else None for k in _dist.OUT])
        self.engine.disturbance_track_ptr(B, T, actual.data_ptr(), logs["forces"].data_ptr(), logs[feet].data_ptr(), _ptr(body), state.data_ptr(),
                                          _ptr(dist), _ptr(resid), _dist.observer_struct(observer), st.cuda_stream)
        return {"dist": dist, "resid": resid, "state": state}

    def solve_batch_gait(self, x0, ref, feet0, footholds, gait, feet_id, mu, want_X=False, stream=None, u_init=None):
        """Gait entry point: contact masks, stance lever arms and x_des are generated on the device (include/mpcqp.h) from S plan steps
        per robot (footholds [B,S,4,3], feet_id [B,S,4]; S = 2 is the original two-step form)."""
        torch = _torch()
        B = int(x0.shape[0])
        S = int(footholds.shape[1]) if footholds.dim() == 4 and footholds.shape[1] >= 1 else -1   # (-1: no shape matches)
        check_operands(self.device, (("x0", x0, (B, 13), self.tdtype), ("ref", ref, (B, 10), self.tdtype),
                                     ("feet0", feet0, (B, 4, 3), self.tdtype), ("footholds", footholds, (B, S, 4, 3), self.tdtype),
                                     ("gait", gait, (B, 4), torch.int32), ("feet_id", feet_id, (B, S, 4), torch.uint8),
                                     ("mu", mu, (B,), self.tdtype)))
        return self._solve(self.engine.solve_batch_gait_steps_ptr, (B, S), (x0, ref, feet0, footholds, gait, feet_id, mu), want_X, stream,
                           u_init)

    def _rollout(self, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T, log, stream, plant=None):
        """The body of `rollout` (plant = None) and of `rollout_plant` (plant = (body, push, push_ticks, substeps))."""
        torch = _torch()
        B, S = int(plan_pos.shape[0]), int(plan_pos.shape[1])
        body, push, push_ticks, substeps = plant or (None, None, None, 0)
        check_operands(self.device, (("x", x, (B, 13), self.tdtype), ("ref", ref, (B, 10), self.tdtype),
                                     ("plan_pos", plan_pos, (B, S, 4, 3), self.tdtype), ("plan_feet_id", plan_feet_id, (B, S, 4), torch.uint8),
                                     ("plan_meta", plan_meta, (B, 4), torch.int32), ("tick", tick, (B,), torch.int32),
                                     ("mu", mu, (B,), self.tdtype), ("body", body, (B, 7), self.tdtype), ("push", push, (B, 6), self.tdtype),
                                     ("push_ticks", push_ticks, (B, 2), torch.int32)), optional=("body", "push", "push_ticks"))
        st = self._stream(stream)
        rows = ((B, T, 12), self.tdtype) if log else None
        # (the advance kernel initialises `solved` at the first tick, on `st`; without a tick nothing does)
        actual, desired, forces, solved = self._alloc(stream, rows, rows, rows, ((B,), torch.int32, not T > 0))
        state = [t.data_ptr() for t in (x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu)]
        logs = (_ptr(actual), _ptr(desired), _ptr(forces), solved.data_ptr(), st.cuda_stream)
        if plant is None:
            self.engine.rollout_ptr(B, T, S, *state, *logs)
        else:
            self.engine.rollout_plant_ptr(B, T, S, *state, _ptr(body), _ptr(push), _ptr(push_ticks), substeps, *logs)
        return {"actual": actual, "desired": desired, "forces": forces, "solved": solved}

    def rollout(self, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T, log=True, stream=None):
        """Closed-loop roll-out of B robots over T control ticks on the device (include/mpcqp.h, mpcqp_rollout): `x`, `ref` and `tick`
        are advanced IN PLACE; returns the per-tick logs (the reference log's TRACKING PERFORMANCE actual / desired rows and stage-0
        FORCES, src/logger.py:22-46) and the per-robot count of solved ticks."""
        return self._rollout(x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T, log, stream)

    def plant_step(self, x, f, feet, contact, body=None, wrench=None, substeps=10, stream=None):
        """One control period of the rigid-body plant for B robots (include/mpcqp_sim.h, mpcqp_plant_step): x [B,13], f [B,12] foot
        forces held over the tick, feet [B,4,3] world foot positions, contact uint8 [B,4] (nonzero = stance), body [B,7] (m, Ixx, Iyy,
        Izz, Ixy, Ixz, Iyz; None = the engine's model), wrench [B,6] (force, torque about the CoM; None = no push).  Returns a new
        [B,13] tensor; asynchronous on `stream`.  The host checker is plant.srb_step."""
        torch = _torch()
        B = int(x.shape[0])
        check_operands(self.device, (("x", x, (B, 13), self.tdtype), ("f", f, (B, 12), self.tdtype), ("feet", feet, (B, 4, 3), self.tdtype),
                                     ("contact", contact, (B, 4), torch.uint8), ("body", body, (B, 7), self.tdtype),
                                     ("wrench", wrench, (B, 6), self.tdtype)), optional=("body", "wrench"))
        st = self._stream(stream)
        out, = self._alloc(stream, ((B, 13), self.tdtype))
        self.engine.plant_step_ptr(B, x.data_ptr(), f.data_ptr(), feet.data_ptr(), contact.data_ptr(), _ptr(body), _ptr(wrench), substeps,
                                   out.data_ptr(), st.cuda_stream)
        return out

    def rollout_plant(self, x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T, body=None, push=None, push_ticks=None, substeps=10,
                      log=True, stream=None):
        """`rollout` with the world step x <- X[:,1] replaced by the rigid-body plant (include/mpcqp_sim.h, mpcqp_rollout_plant):
        body [B,7] per-robot mass and torso-frame inertia (None = the engine's model), push [B,6] a world-frame wrench acting on the
        robot's own ticks push_ticks[b][0] <= tick < push_ticks[b][1] (int32 [B,2], required with push).  Same in-place advance of
        `x`, `ref` and `tick`, same logs and `solved` count as `rollout`."""
        return self._rollout(x, ref, plan_pos, plan_feet_id, plan_meta, tick, mu, T, log, stream, (body, push, push_ticks, substeps))

    def _phase_rows(self, B, x, ref, feet, gait, tick, stand, gain, x_name="x0"):
        """Operand rows the three phase calls share."""
        torch = _torch()
        return ((x_name, x, (B, 13), self.tdtype), ("ref", ref, (B, 10), self.tdtype), ("feet", feet, (B, 4, 3), self.tdtype),
                ("gait", gait, (B, 9), torch.int32), ("tick", tick, (B,), torch.int32), ("stand", stand, (B, 4, 3), self.tdtype),
                ("gain", gain, (B,), self.tdtype))

    def phase_expand(self, x0, ref, feet, gait, tick, stand, gain=None, stream=None):
        """The operator tuple of a per-leg periodic gait, generated on the device (include/mpcqp_plan.h, mpcqp_phase_expand; the host
        counterpart is gaits.phase_expand_host): x0 [B,13], ref [B,10], feet [B,4,3] the held feet, gait int32 [B,9] = (P, offset[4],
        stance[4]) in ticks (gaits.gait_rows), tick int32 [B], stand [B,4,3] (nominal foot x / y in the yaw frame, world ground z),
        gain [B] or None (0) -> {"r": [B,N,4,3], "contact": uint8 [B,N,4], "xdes": [B,N+1,13]}.  Asynchronous on `stream`."""
        torch = _torch()
        B, N = int(x0.shape[0]), self.N
        check_operands(self.device, self._phase_rows(B, x0, ref, feet, gait, tick, stand, gain), optional=("gain",))
        st = self._stream(stream)
        r, contact, xdes = self._alloc(stream, ((B, N, 4, 3), self.tdtype), ((B, N, 4), torch.uint8), ((B, N + 1, 13), self.tdtype))
        self.engine.phase_expand_ptr(B, x0.data_ptr(), ref.data_ptr(), feet.data_ptr(), gait.data_ptr(), tick.data_ptr(), stand.data_ptr(),
                                     _ptr(gain), r.data_ptr(), contact.data_ptr(), xdes.data_ptr(), st.cuda_stream)
        return {"r": r, "contact": contact, "xdes": xdes}

    def solve_batch_phase(self, x0, ref, feet, gait, tick, stand, gain, mu, want_X=False, stream=None, u_init=None):
        """`phase_expand` into the engine's own workspace and `solve_batch` on that tuple, in one call (include/mpcqp_plan.h,
        mpcqp_solve_batch_phase).  `gain` may be None."""
        B = int(x0.shape[0])
        check_operands(self.device, self._phase_rows(B, x0, ref, feet, gait, tick, stand, gain) + (("mu", mu, (B,), self.tdtype),),
                       optional=("gain",))
        call = lambda B, x0, ref, feet, gait, tick, stand, mu, *out: self.engine.solve_batch_phase_ptr(
            B, x0, ref, feet, gait, tick, stand, _ptr(gain), mu, *out)
        return self._solve(call, (B,), (x0, ref, feet, gait, tick, stand, mu), want_X, stream, u_init)

    def rollout_phase(self, x, ref, feet, gait, stand, gain, tick, mu, T, body=None, push=None, push_ticks=None, substeps=10, log=True,
                      stream=None):
        """`rollout_plant` on a per-leg gait clock with reactive footholds (include/mpcqp_sim.h, mpcqp_rollout_phase; the host
        counterpart is gaits.rollout_phase_host): `feet` [B,4,3] is state next to `x`, `ref` and `tick`, all advanced IN PLACE -- a leg
        that touches down gets its foothold from the measured state, every other foot is untouched.  gait, stand, gain as in
        `phase_expand`; body, push, push_ticks, substeps as in `rollout_plant`.  Returns the logs of `rollout` plus "feet_log"
        [B,T,4,3] and "contact_log" uint8 [B,T,4], the feet and stance mask the plant used each tick (a swing leg's row is its lift-off
        foot: `phase_swing` turns these logs into the swing trajectories, and its "feet_des" is the operand `joint_log` and
        `joint_rates` want).  Keep a copy of `tick` for that call: the roll-out advances it."""
        torch = _torch()
        B, T = int(x.shape[0]), int(T)
        check_operands(self.device, self._phase_rows(B, x, ref, feet, gait, tick, stand, gain, "x") + (
            ("mu", mu, (B,), self.tdtype), ("body", body, (B, 7), self.tdtype), ("push", push, (B, 6), self.tdtype),
            ("push_ticks", push_ticks, (B, 2), torch.int32)), optional=("gain", "body", "push", "push_ticks"))
        st = self._stream(stream)
        rows = ((B, T, 12), self.tdtype) if log else None
        actual, desired, forces, feet_log, contact_log, solved = self._alloc(
            stream, rows, rows, rows, ((B, T, 4, 3), self.tdtype) if log else None, ((B, T, 4), torch.uint8) if log else None,
            ((B,), torch.int32, not T > 0))
        self.engine.rollout_phase_ptr(B, T, x.data_ptr(), ref.data_ptr(), feet.data_ptr(), gait.data_ptr(), stand.data_ptr(), _ptr(gain),
                                      tick.data_ptr(), mu.data_ptr(), _ptr(body), _ptr(push), _ptr(push_ticks), substeps, _ptr(actual),
                                      _ptr(desired), _ptr(forces), _ptr(feet_log), _ptr(contact_log), solved.data_ptr(), st.cuda_stream)
        return {"actual": actual, "desired": desired, "forces": forces, "feet_log": feet_log, "contact_log": contact_log, "solved": solved}

    def phase_swing(self, logs, gait, tick0, stand, gain, step_height, want_des=True, stream=None):
        """Swing-foot trajectories of a `rollout_phase` from its logs (include/mpcqp_plan.h, mpcqp_phase_swing; the host counterpart is
        gaits.phase_swing_host): `logs` as `rollout_phase` returns them ("actual", "desired", "feet_log"), gait / stand / gain the
        roll-out's rows (gain may be None), tick0 int32 [B] the value `tick` had BEFORE the roll-out (a copy: the roll-out advances
        `tick` in place), step_height [B].  Returns {"swing": [B,T,4,4,3] pos / vel / acc / target of every (robot, tick, leg),
        "feet_des": [B,T,4,3] = pos, or None}: a swing leg runs from its lift-off foot to the foothold rule at the touchdown predicted
        from the tick's measured state; a stance leg keeps its feet_log row with vel = acc = 0.  Asynchronous on `stream`."""
        torch = _torch()
        actual, desired, feet_log = logs["actual"], logs["desired"], logs["feet_log"]
        if actual is None or actual.dim() != 3:
            raise ValueError("phase_swing needs the logs of rollout_phase(..., log=True)")
        B, T = int(actual.shape[0]), int(actual.shape[1])
        check_operands(self.device, (("actual", actual, (B, T, 12), self.tdtype), ("desired", desired, (B, T, 12), self.tdtype),
                                     ("feet_log", feet_log, (B, T, 4, 3), self.tdtype), ("gait", gait, (B, 9), torch.int32),
                                     ("tick0", tick0, (B,), torch.int32), ("stand", stand, (B, 4, 3), self.tdtype),
                                     ("gain", gain, (B,), self.tdtype), ("step_height", step_height, (B,), self.tdtype)), optional=("gain",))
        st = self._stream(stream)
        swing, des = self._alloc(stream, ((B, T, 4, 4, 3), self.tdtype), ((B, T, 4, 3), self.tdtype) if want_des else None)
        self.engine.phase_swing_ptr(B, T, actual.data_ptr(), desired.data_ptr(), feet_log.data_ptr(), gait.data_ptr(), tick0.data_ptr(),
                                    stand.data_ptr(), _ptr(gain), step_height.data_ptr(), swing.data_ptr(), _ptr(des), st.cuda_stream)
        return {"swing": swing, "feet_des": des}

    def plan_footsteps(self, feet0, cmd, gait, S, want_ang=True, want_hip=False, stream=None):
        """Footstep plans of B robots on the device (include/mpcqp_plan.h, mpcqp_plan_footsteps; the host FootstepPlanner per robot):
        feet0 [B,4,3] initial feet FL, FR, HL, HR and cmd [B,5] (yaw0, v_com_ref x, v_com_ref y, theta_dot, h) of the engine's dtype,
        gait int32 [B,4] (total_steps, ss, ds, first_swing bit mask; bit k = leg k stays down in step 1).  Returns device tensors
        plan_pos [B,S,4,3], plan_feet_id uint8 [B,S,4] and plan_meta int32 [B,4] -- the plan arguments of `rollout` -- plus plan_ang
        [B,S] and plan_hip [B,S,3] when asked for (None otherwise).  The tick length is the engine's delta; asynchronous on `stream`."""
        torch = _torch()
        B, S = int(feet0.shape[0]), int(S)
        check_operands(self.device, (("feet0", feet0, (B, 4, 3), self.tdtype), ("cmd", cmd, (B, 5), self.tdtype),
                                     ("gait", gait, (B, 4), torch.int32)))
        if S < 1:
            raise ValueError(f"S must be >= 1, got {S}")
        st = self._stream(stream)
        out = dict(zip(("plan_pos", "plan_feet_id", "plan_meta", "plan_ang", "plan_hip"), self._alloc(
            stream, ((B, S, 4, 3), self.tdtype), ((B, S, 4), torch.uint8), ((B, 4), torch.int32),
            ((B, S), self.tdtype) if want_ang else None, ((B, S, 3), self.tdtype) if want_hip else None)))
        self.engine.plan_footsteps_ptr(B, S, feet0.data_ptr(), cmd.data_ptr(), gait.data_ptr(), out["plan_pos"].data_ptr(),
                                       out["plan_feet_id"].data_ptr(), out["plan_meta"].data_ptr(), _ptr(out["plan_ang"]),
                                       _ptr(out["plan_hip"]), st.cuda_stream)
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
        B, K = int(pos.shape[0]), int(K)
        S = int(pos.shape[1]) if pos.dim() == 4 and pos.shape[1] >= 1 else -1   # (-1: no shape matches)
        check_operands(self.device, (("plan_pos", pos, (B, S, 4, 3), self.tdtype), ("plan_feet_id", fid, (B, S, 4), torch.uint8),
                                     ("plan_meta", meta, (B, 4), torch.int32), ("plan_ang", ang, (B, S), self.tdtype),
                                     ("tick", tick, (B,), torch.int32), ("step_height", step_height, (B,), self.tdtype)))
        if K < 0:
            raise ValueError(f"K must be >= 0, got {K}")
        st = self._stream(stream)
        traj, des = self._alloc(stream, ((B, K, 4, 3, 6), self.tdtype), ((B, K, 4, 3), self.tdtype) if want_des else None)
        self.engine.swing_trajectories_ptr(B, K, S, pos.data_ptr(), fid.data_ptr(), meta.data_ptr(), ang.data_ptr(), tick.data_ptr(),
                                           step_height.data_ptr(), traj.data_ptr(), _ptr(des), st.cuda_stream)
        return {"traj": traj, "feet_des": des}

    def torque_map(self, u, jac, stream=None):
        """tau[B,4,3] = J^T (-f) of the stage-0 forces (src/main.py:212-214); u[B,N,12] as the solves return it, jac[B,4,3,3]
        world-frame leg Jacobians."""
        B = int(u.shape[0])
        check_operands(self.device, (("u", u, (B, self.N, 12), self.tdtype), ("jac", jac, (B, 4, 3, 3), self.tdtype)))
        st = self._stream(stream)
        tau, = self._alloc(stream, ((B, 4, 3), self.tdtype))
        self.engine.torque_map_ptr(B, u.data_ptr(), jac.data_ptr(), tau.data_ptr(), st.cuda_stream)
        return tau

    def leg_jacobians(self, q, rot=None, geometry=None, want_foot=True, stream=None):
        """World-frame 3x3 linear Jacobian block of each foot w.r.t. its leg's joints (what src/main.py:205-210 asks DART for), on the
        device: q [B,4,3] joint angles (HipX, HipY, Knee per leg), rot [B,3,3] torso orientation or None -> (jac [B,4,3,3], foot [B,4,3])."""
        B = int(q.shape[0])
        check_operands(self.device, (("q", q, (B, 4, 3), self.tdtype), ("rot", rot, (B, 3, 3), self.tdtype)), optional=("rot",))
        st = self._stream(stream)
        jac, foot = self._alloc(stream, ((B, 4, 3, 3), self.tdtype), ((B, 4, 3), self.tdtype) if want_foot else None)
        self.engine.leg_jacobians_ptr(B, q.data_ptr(), _ptr(rot), jac.data_ptr(), _ptr(foot), geometry, st.cuda_stream)
        return jac, foot

    def leg_ik(self, foot, rot=None, origin=None, geometry=None, want_reach=True, stream=None):
        """Closed-form inverse kinematics of the four legs on the device (include/mpcqp_joints.h, mpcqp_leg_ik; the host counterpart is
        lite3_model.leg_ik_closed): foot [B,4,3] foot positions in world orientation, rot [B,3,3] torso orientation (world <- torso) or
        None, origin [B,3] torso origin or None -> (q [B,4,3] HipX, HipY, Knee, reach uint8 [B,4] or None).  With rot and origin None
        this inverts the `foot` output of `leg_jacobians`.  Out of reach: q of the nearest boundary and reach = 0; a non-finite leg:
        NaN and 0.  Asynchronous on `stream`."""
        B = int(foot.shape[0])
        check_operands(self.device, (("foot", foot, (B, 4, 3), self.tdtype), ("rot", rot, (B, 3, 3), self.tdtype),
                                     ("origin", origin, (B, 3), self.tdtype)), optional=("rot", "origin"))
        st = self._stream(stream)
        q, reach = self._alloc(stream, ((B, 4, 3), self.tdtype), ((B, 4), _torch().uint8) if want_reach else None)
        self.engine.leg_ik_ptr(B, foot.data_ptr(), _ptr(rot), _ptr(origin), q.data_ptr(), _ptr(reach), geometry, st.cuda_stream)
        return q, reach

    def joint_log(self, actual, forces, feet, geometry=None, stream=None):
        """Joint-space log of a roll-out on the device (include/mpcqp_joints.h, mpcqp_joint_log; the host counterpart is
        lite3_model.joint_log_host): actual, forces [B,T,12] as `rollout` / `rollout_plant` return them, feet [B,T,4,3] world foot
        positions -- `swing_trajectories(plan, first_tick, K=T, ...)["feet_des"]` -> {"q": [B,T,4,3] joint angles, "tau": [B,T,4,3]
        joint torques (R J)^T (-f), "reach": uint8 [B,T,4]}.  Asynchronous on `stream`."""
        B, T = int(actual.shape[0]), int(actual.shape[1]) if actual.dim() == 3 else -1
        check_operands(self.device, (("actual", actual, (B, T, 12), self.tdtype), ("forces", forces, (B, T, 12), self.tdtype),
                                     ("feet", feet, (B, T, 4, 3), self.tdtype)))
        st = self._stream(stream)
        q, tau, reach = self._alloc(stream, ((B, T, 4, 3), self.tdtype), ((B, T, 4, 3), self.tdtype), ((B, T, 4), _torch().uint8))
        self.engine.joint_log_ptr(B, T, actual.data_ptr(), forces.data_ptr(), feet.data_ptr(), q.data_ptr(), tau.data_ptr(), reach.data_ptr(),
                                  geometry, st.cuda_stream)
        return {"q": q, "tau": tau, "reach": reach}

    def joint_rates(self, actual, forces, feet, foot_vel=None, geometry=None, stream=None):
        """`joint_log` plus joint rates and joint power (include/mpcqp_joints.h, mpcqp_joint_rates; the host counterpart is
        lite3_model.joint_rates_host): foot_vel [B,T,4,3] the feet's world velocities -- `phase_swing(...)["swing"][:, :, :, 1]`, made
        contiguous -- or None for feet at rest in the world -> {"q", "qd" [B,T,4,3] rad / s, "tau", "power" [B,T,4] = tau . qd per leg
        in W, "reach"}; q, tau and reach are `joint_log`'s, bit for bit.  Out of reach: qd = power = 0.  Asynchronous on `stream`."""
        B, T = int(actual.shape[0]), int(actual.shape[1]) if actual.dim() == 3 else -1
        check_operands(self.device, (("actual", actual, (B, T, 12), self.tdtype), ("forces", forces, (B, T, 12), self.tdtype),
                                     ("feet", feet, (B, T, 4, 3), self.tdtype), ("foot_vel", foot_vel, (B, T, 4, 3), self.tdtype)),
                       optional=("foot_vel",))
        st = self._stream(stream)
        legs = ((B, T, 4, 3), self.tdtype)
        q, qd, tau, power, reach = self._alloc(stream, legs, legs, legs, ((B, T, 4), self.tdtype), ((B, T, 4), _torch().uint8))
        self.engine.joint_rates_ptr(B, T, actual.data_ptr(), forces.data_ptr(), feet.data_ptr(), _ptr(foot_vel), q.data_ptr(), qd.data_ptr(),
                                    tau.data_ptr(), power.data_ptr(), reach.data_ptr(), geometry, st.cuda_stream)
        return {"q": q, "qd": qd, "tau": tau, "power": power, "reach": reach}

    @staticmethod
    def _inertia(inertia):
        """None, an MpcQpLegInertia, or a dict of arrays as lite3_model.leg_inertia() returns it."""
        return _capi.MpcQpLegInertia.from_dict(inertia) if isinstance(inertia, dict) else inertia

    def leg_dynamics(self, q, qd=None, qdd=None, rot=None, base=None, inertia=None, geometry=None, want=("tau", "mass", "bias"), stream=None):
        """The leg's equations of motion on the device (include/mpcqp_joints.h, mpcqp_leg_dynamics; the host counterpart is
        lite3_model.leg_dynamics_host): q [B,4,3], qd / qdd [B,4,3] or None (0), rot [B,3,3] world <- torso or None, base [B,9] = the
        torso's world-frame angular velocity, angular acceleration and the linear acceleration of its origin, or None (at rest);
        inertia a dict as lite3_model.leg_inertia() or None (the Lite3) -> {"tau": [B,4,3] joint torques that produce qdd, "mass":
        [B,4,3,3] M(q), "bias": [B,4,3] tau at qdd = 0}, so tau = M qdd + bias; an output not in `want` is None.  Asynchronous."""
        B = int(q.shape[0])
        legs = (B, 4, 3)
        check_operands(self.device, (("q", q, legs, self.tdtype), ("qd", qd, legs, self.tdtype), ("qdd", qdd, legs, self.tdtype),
                                     ("rot", rot, (B, 3, 3), self.tdtype), ("base", base, (B, 9), self.tdtype)),
                       optional=("qd", "qdd", "rot", "base"))
        st = self._stream(stream)
        tau, mass, bias = self._alloc(stream, (legs, self.tdtype) if "tau" in want else None,
                                      ((B, 4, 3, 3), self.tdtype) if "mass" in want else None, (legs, self.tdtype) if "bias" in want else None)
        self.engine.leg_dynamics_ptr(B, q.data_ptr(), _ptr(qd), _ptr(qdd), _ptr(rot), _ptr(base), _ptr(tau), _ptr(mass), _ptr(bias), geometry,
                                     self._inertia(inertia), st.cuda_stream)
        return {"tau": tau, "mass": mass, "bias": bias}

    def leg_effort(self, actual, forces, feet, foot_vel=None, foot_acc=None, base_acc=None, body=None, inertia=None, geometry=None,
                   stream=None):
        """The full joint torques of a roll-out's log and whether the actuators could deliver them (include/mpcqp_joints.h,
        mpcqp_leg_effort; the host counterpart is lite3_model.leg_effort_host): actual, forces, feet, foot_vel as for `joint_rates`;
        foot_acc [B,T,4,3] the feet's world accelerations -- `phase_swing(...)["swing"][:, :, :, 2]`, made contiguous -- or None (0);
        base_acc [B,T,6] the torso's angular and the CoM's linear acceleration, or None for the unpushed plant's right-hand side at each
        row, formed with body [B,7] (None = the engine's model) -> {"qdd", "tau_dyn", "tau" [B,T,4,3], "power" [B,T,4], "limit" uint8
        [B,T,4]: 1 = a joint angle, 2 = a joint rate, 4 = a joint torque beyond the actuator's limit, 8 = out of reach; 0xff = a
        non-finite leg}.  tau = `joint_rates`' tau + tau_dyn.  Asynchronous on `stream`."""
        B, T = int(actual.shape[0]), int(actual.shape[1]) if actual.dim() == 3 else -1
        legs = ((B, T, 4, 3), self.tdtype)
        check_operands(self.device, (("actual", actual, (B, T, 12), self.tdtype), ("forces", forces, (B, T, 12), self.tdtype),
                                     ("feet", feet, *legs), ("foot_vel", foot_vel, *legs), ("foot_acc", foot_acc, *legs),
                                     ("base_acc", base_acc, (B, T, 6), self.tdtype), ("body", body, (B, 7), self.tdtype)),
                       optional=("foot_vel", "foot_acc", "base_acc", "body"))
        st = self._stream(stream)
        qdd, tau_dyn, tau, power, limit = self._alloc(stream, legs, legs, legs, ((B, T, 4), self.tdtype), ((B, T, 4), _torch().uint8))
        self.engine.leg_effort_ptr(B, T, actual.data_ptr(), forces.data_ptr(), feet.data_ptr(), _ptr(foot_vel), _ptr(foot_acc), _ptr(base_acc),
                                   _ptr(body), qdd.data_ptr(), tau_dyn.data_ptr(), tau.data_ptr(), power.data_ptr(), limit.data_ptr(), geometry,
                                   self._inertia(inertia), st.cuda_stream)
        return {"qdd": qdd, "tau_dyn": tau_dyn, "tau": tau, "power": power, "limit": limit}

    def leg_accel(self, q, tau, qd=None, rot=None, base=None, inertia=None, geometry=None, want_det=True, stream=None):
        """The leg's forward dynamics on the device (include/mpcqp_joints.h, mpcqp_leg_accel; the host counterpart is
        lite3_model.leg_accel_host): the operands of `leg_dynamics` with the applied joint torques tau [B,4,3] on the input side ->
        {"qdd": [B,4,3] = M^-1 (tau - bias), "det": [B,4] = det M(q) or None}.  Massless legs: qdd = 0.  Asynchronous on `stream`."""
        B = int(q.shape[0])
        legs = (B, 4, 3)
        check_operands(self.device, (("q", q, legs, self.tdtype), ("tau", tau, legs, self.tdtype), ("qd", qd, legs, self.tdtype),
                                     ("rot", rot, (B, 3, 3), self.tdtype), ("base", base, (B, 9), self.tdtype)),
                       optional=("qd", "rot", "base"))
        st = self._stream(stream)
        qdd, det = self._alloc(stream, (legs, self.tdtype), ((B, 4), self.tdtype) if want_det else None)
        self.engine.leg_accel_ptr(B, q.data_ptr(), _ptr(qd), tau.data_ptr(), _ptr(rot), _ptr(base), qdd.data_ptr(), _ptr(det), geometry,
                                  self._inertia(inertia), st.cuda_stream)
        return {"qdd": qdd, "det": det}

    from .lite3_model import SWING_OUT      # ("q", "qd", "tau", "foot", "err", "flag"): the host counterpart's names, in the C order

    def swing_track(self, logs, swing, body=None, base_acc=None, gains=None, state=None, substeps=0, inertia=None, geometry=None,
                    want=SWING_OUT, stream=None):
        """The swing legs of a roll-out under their tracking controller, on the device (include/mpcqp_joints.h, mpcqp_swing_track; the
        host counterpart is lite3_model.swing_track_host): `logs` as `rollout_phase` returns them ("actual", "forces", "feet_log",
        "contact_log"), swing [B,T,4,4,3] the "swing" of `phase_swing`; base_acc [B,T,6] or None for the unpushed plant's right-hand
        side formed with body [B,7] (None = the engine's model); gains [B,2] = (Kp, Kd) or None (250, 15); state [B,4,7] = per leg q,
        qd, live, advanced IN PLACE, or None (every leg starts from its row); `substeps` control periods per tick (0: 2 ms periods) ->
        {"q", "qd", "tau", "foot" [B,T,4,3], "err" [B,T,4] = |desired - actual foot| and on a landing row the landing miss, "flag" uint8
        [B,T,4]: 1 swing row, 2 torque clamped, 4 joint angle, 8 joint rate beyond its limit, 16 singular, 64 landing row, 0xff
        non-finite}; an output not in `want` is None.  Asynchronous on `stream`."""
        torch = _torch()
        actual, forces, feet_log, contact = logs["actual"], logs["forces"], logs["feet_log"], logs["contact_log"]
        if actual is None or actual.dim() != 3:
            raise ValueError("swing_track needs the logs of rollout_phase(..., log=True)")
        B, T = int(actual.shape[0]), int(actual.shape[1])
        legs = ((B, T, 4, 3), self.tdtype)
        check_operands(self.device, (("actual", actual, (B, T, 12), self.tdtype), ("forces", forces, (B, T, 12), self.tdtype),
                                     ("feet_log", feet_log, *legs), ("contact_log", contact, (B, T, 4), torch.uint8),
                                     ("swing", swing, (B, T, 4, 4, 3), self.tdtype), ("base_acc", base_acc, (B, T, 6), self.tdtype),
                                     ("body", body, (B, 7), self.tdtype), ("gains", gains, (B, 2), self.tdtype),
                                     ("state", state, (B, 4, 7), self.tdtype)), optional=("base_acc", "body", "gains", "state"))
        unknown = set(want) - set(self.SWING_OUT)
        if unknown or not want:
            raise ValueError(f"want must name at least one of {self.SWING_OUT}, got {tuple(want)}")
        st = self._stream(stream)
        spec = {"q": legs, "qd": legs, "tau": legs, "foot": legs, "err": ((B, T, 4), self.tdtype), "flag": ((B, T, 4), torch.uint8)}
        out = dict(zip(self.SWING_OUT, self._alloc(stream, *[spec[k] if k in want else None for k in self.SWING_OUT])))
        self.engine.swing_track_ptr(B, T, actual.data_ptr(), forces.data_ptr(), feet_log.data_ptr(), contact.data_ptr(), swing.data_ptr(),
                                    _ptr(base_acc), _ptr(body), _ptr(gains), _ptr(state), int(substeps),
                                    *[_ptr(out[k]) for k in self.SWING_OUT], geometry, self._inertia(inertia), st.cuda_stream)
        return out

    LEGS_LOGS = ("swing",) + SWING_OUT + ("miss",)      # the logs `rollout_legs` adds to `rollout_phase`'s, in the C order

    def _rollout_legs(self, call, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land, body, push, push_ticks, substeps,
                      gains, leg_substeps, inertia, geometry, log, stream, drive=_NO_DRIVE, operands=(), optional=(), logs=(), tail=()):
        """What `rollout_legs`, `rollout_drive` and `rollout_slip` share: the checks, the log spec, the allocation and the addresses
        for `call`, the engine's entry point.  drive (left out: `call` takes no drive mode) goes to `call` after the landing mode, then the
        tensors of `operands`, rows as `check_operands` takes them (None passes for the names in `optional`); `logs`, rows (name,
        shape after [B,T], dtype), follow `rollout_legs`' logs in the result and in the call; `tail`, arguments as `call` takes them, go
        between the logs and the geometry."""
        torch = _torch()
        B, T = int(x.shape[0]), int(T)
        if land not in ("rule", "actual"):
            raise ValueError(f"land must be 'rule' or 'actual', got {land!r}")
        modes = {"ideal": _capi.DRIVE_IDEAL, "limited": _capi.DRIVE_LIMITED}
        if drive is not _NO_DRIVE and not isinstance(drive, int) and drive not in modes:
            raise ValueError(f"drive must be 'ideal' or 'limited', got {drive!r}")
        check_operands(self.device, self._phase_rows(B, x, ref, feet, gait, tick, stand, gain, "x") + (
            ("legs", legs, (B, 4, 7), torch.float64), ("mu", mu, (B,), self.tdtype), ("body", body, (B, 7), self.tdtype),
            ("push", push, (B, 6), self.tdtype), ("push_ticks", push_ticks, (B, 2), torch.int32),
            ("step_height", step_height, (B,), self.tdtype), ("gains", gains, (B, 2), self.tdtype)) + operands,
            optional=("gain", "body", "push", "push_ticks", "gains") + tuple(optional))
        st = self._stream(stream)
        rows, leg3 = ((B, T, 12), self.tdtype), ((B, T, 4, 3), self.tdtype)
        leg1, mask = ((B, T, 4), self.tdtype), ((B, T, 4), torch.uint8)
        spec = (rows, rows, rows, leg3, mask) + (((B, T, 4, 4, 3), self.tdtype), leg3, leg3, leg3, leg3, leg1, mask, leg1)
        spec += tuple(((B, T) + tail, dt) for _, tail, dt in logs)
        names = ("actual", "desired", "forces", "feet_log", "contact_log") + self.LEGS_LOGS + tuple(k for k, _, _ in logs)
        out = dict(zip(names, self._alloc(stream, *[s if log else None for s in spec])))
        solved, = self._alloc(stream, ((B,), torch.int32, not T > 0))
        p = lambda k: _ptr(out[k])
        mode = () if drive is _NO_DRIVE else (drive if isinstance(drive, int) else modes[drive],)
        call(B, T, x.data_ptr(), ref.data_ptr(), feet.data_ptr(), legs.data_ptr(), gait.data_ptr(), stand.data_ptr(), _ptr(gain),
             tick.data_ptr(), mu.data_ptr(), _ptr(body), _ptr(push), _ptr(push_ticks), substeps, step_height.data_ptr(), _ptr(gains),
             int(leg_substeps), _capi.LAND_ACTUAL if land == "actual" else _capi.LAND_RULE, *mode, *[_ptr(t) for _, t, _, _ in operands],
             *[p(k) for k in names[:5]], solved.data_ptr(), *[p(k) for k in names[5:]], *tail, geometry, self._inertia(inertia), st.cuda_stream)
        out["solved"] = solved
        return out

    def rollout_legs(self, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land="rule", body=None, push=None,
                     push_ticks=None, substeps=10, gains=None, leg_substeps=0, inertia=None, geometry=None, log=True, stream=None):
        """`rollout_phase` with the swing legs integrated inside the roll-out (include/mpcqp_sim.h, mpcqp_rollout_legs; the host
        counterpart is gaits.rollout_legs_host): legs float64 [B,4,7] = per leg q, qd, live (the `state` of `swing_track`; zeros: every
        leg starts from its row) is state next to `x`, `ref`, `feet` and `tick`, all advanced IN PLACE.  Per tick the legs take one row
        of `phase_swing` and of `swing_track` formed from the live buffers, under the plant's right-hand side with the robot's push;
        step_height [B] as in `phase_swing`; gains [B,2], leg_substeps, inertia, geometry as `gains`, `substeps`, ... of `swing_track`.
        land="rule": a foot that touches down lands on the foothold rule, and x, ref, feet, tick and `rollout_phase`'s logs are what
        `rollout_phase` gives, bit for bit; land="actual": it lands where its leg put it (the rule's z).  Returns the logs of
        `rollout_phase` plus "swing" [B,T,4,4,3] (`phase_swing`'s), "q", "qd", "tau", "foot" [B,T,4,3], "err" [B,T,4], "flag" uint8
        [B,T,4] (`swing_track`'s) and "miss" [B,T,4]: the distance between the delivered foot and the rule's foothold of a leg that
        touches down after tick t, 0 elsewhere.  Asynchronous on `stream`."""
        return self._rollout_legs(self.engine.rollout_legs_ptr, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land, body,
                                  push, push_ticks, substeps, gains, leg_substeps, inertia, geometry, log, stream)

    def _stance_rows(self, x, f, feet, contact, stream):
        """What `stance_drive` and `stance_slip` share of their operands: B, x (a 12-wide row padded to 13 columns on `stream`) and the
        rows of x, f, feet and contact for `check_operands`."""
        torch = _torch()
        B = int(x.shape[0])
        if x.dim() == 2 and x.shape[1] == 12:
            with torch.cuda.stream(stream):
                x = torch.cat([x, torch.zeros((B, 1), dtype=x.dtype, device=x.device)], dim=1).contiguous()
        return B, x, (("x", x, (B, 13), self.tdtype), ("f", f, (B, 12), self.tdtype), ("feet", feet, (B, 4, 3), self.tdtype),
                      ("contact", contact, (B, 4), torch.uint8))

    def stance_drive(self, x, f, feet, contact, ground=None, inertia=None, geometry=None, want=("tau", "flag"), stream=None):
        """What the stance legs deliver of a commanded force (include/mpcqp_sim.h, mpcqp_stance_drive, which has the rule; the host
        counterpart is lite3_model.stance_drive_host): x [B,13] or [B,12] (the rule reads the rotation vector and the CoM; a 12-wide
        row, as the roll-outs log it, is padded), f [B,12] the commanded foot forces, feet [B,4,3] the held feet, contact uint8 [B,4],
        ground [B] the ground's friction coefficient or None (no friction limit; a foot still cannot pull); inertia, geometry as for
        `leg_effort`: the row's tau_max, q_min and q_max are read -> {"f": [B,12] the applied forces, "tau": [B,4,3] the applied joint
        torques (0 on a swing leg), "flag": uint8 [B,4]: 2 torque clamped, 4 joint angle outside its limits, 16 clamped but not
        resolvable (out of reach or singular: the force is kept), 32 the ground limited the force, 0xff a non-finite leg}; "tau" /
        "flag" are None when not in `want`.  The held foot does not move (`stance_slip` lets it slide).  Asynchronous on `stream`."""
        torch = _torch()
        B, x, rows = self._stance_rows(x, f, feet, contact, stream)
        check_operands(self.device, rows + (("ground", ground, (B,), self.tdtype),), optional=("ground",))
        st = self._stream(stream)
        out, tau, flag = self._alloc(stream, ((B, 12), self.tdtype), ((B, 4, 3), self.tdtype) if "tau" in want else None,
                                     ((B, 4), torch.uint8) if "flag" in want else None)
        self.engine.stance_drive_ptr(B, x.data_ptr(), f.data_ptr(), feet.data_ptr(), contact.data_ptr(), _ptr(ground), out.data_ptr(),
                                     _ptr(tau), _ptr(flag), geometry, self._inertia(inertia), st.cuda_stream)
        return {"f": out, "tau": tau, "flag": flag}

    def rollout_drive(self, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land="rule", drive="limited", ground=None,
                      body=None, push=None, push_ticks=None, substeps=10, gains=None, leg_substeps=0, inertia=None, geometry=None,
                      log=True, stream=None):
        """`rollout_legs` with the stance legs as limited force sources (include/mpcqp_sim.h, mpcqp_rollout_drive; the host counterpart
        is gaits.rollout_drive_host): per tick the rule of `stance_drive` runs on the solve's stage-0 forces, and the legs step's torso
        acceleration, the plant and the "forces" log get the APPLIED forces.  drive="limited": the stance torques are clamped at the
        inertia row's tau_max, the limit the swing legs have; drive="ideal": no torque limit.  ground [B]: the ground's friction
        coefficient per robot (`mu` stays the controller's belief) or None.  Returns `rollout_legs`' dict plus "cmd" [B,T,12], the
        commanded forces; on stance rows "tau" is the applied torque and "flag" has the rule's bits 2 / 16 / 32 (score.py's CLAMP_ROWS
        then counts stance rows too).  The MPC is not told about either limit.  drive="ideal" with ground=None is `rollout_legs` bit
        for bit.  Every other argument as in `rollout_legs`.  Asynchronous on `stream`."""
        return self._rollout_legs(self.engine.rollout_drive_ptr, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land, body,
                                  push, push_ticks, substeps, gains, leg_substeps, inertia, geometry, log, stream, drive,
                                  operands=(("ground", ground, (int(x.shape[0]),), self.tdtype),), optional=("ground",),
                                  logs=(("cmd", (12,), self.tdtype),))

    def stance_slip(self, x, f, feet, contact, ground, foot_mass, slip, substeps=10, inertia=None, geometry=None, want=("tau", "flag"),
                    stream=None):
        """`stance_drive` with stance feet that slide (include/mpcqp_slip.h, mpcqp_stance_slip, which has the rule; the host counterpart
        is lite3_model.stance_slip_host): x, f, feet, contact as for `stance_drive`; ground [B] the ground's friction coefficient and
        foot_mass [B] the effective mass of a sliding foot (lite3_model.foot_mass()), both required; slip float64 [B,4,2] the world xy
        velocity of each held foot at the start of the tick (not altered); `substeps` the plant's substeps of the tick (0 means 10) ->
        {"f": [B,12] the applied forces, "tau": [B,4,3], "flag": uint8 [B,4], `stance_drive`'s bits and 128 = the foot slides, "slip":
        float64 [B,4,2] the velocities at the end of the tick (0 on a swing leg), "disp": [B,4,2] how far each foot slid}; "tau" /
        "flag" are None when not in `want`.  Asynchronous on `stream`."""
        torch = _torch()
        B, x, rows = self._stance_rows(x, f, feet, contact, stream)
        check_operands(self.device, rows + (("ground", ground, (B,), self.tdtype), ("foot_mass", foot_mass, (B,), self.tdtype),
                                            ("slip", slip, (B, 4, 2), torch.float64)))
        st = self._stream(stream)
        out, tau, flag, slip_out, disp = self._alloc(stream, ((B, 12), self.tdtype), ((B, 4, 3), self.tdtype) if "tau" in want else None,
                                                     ((B, 4), torch.uint8) if "flag" in want else None, ((B, 4, 2), torch.float64),
                                                     ((B, 4, 2), self.tdtype))
        self.engine.stance_slip_ptr(B, x.data_ptr(), f.data_ptr(), feet.data_ptr(), contact.data_ptr(), ground.data_ptr(), foot_mass.data_ptr(),
                                    slip.data_ptr(), out.data_ptr(), _ptr(tau), _ptr(flag), slip_out.data_ptr(), disp.data_ptr(), int(substeps),
                                    geometry, self._inertia(inertia), st.cuda_stream)
        return {"f": out, "tau": tau, "flag": flag, "slip": slip_out, "disp": disp}

    def rollout_slip(self, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, ground, foot_mass, slip, land="rule",
                     drive="limited", body=None, push=None, push_ticks=None, substeps=10, gains=None, leg_substeps=0, inertia=None,
                     geometry=None, log=True, stream=None):
        """`rollout_drive` with stance feet that slide (include/mpcqp_slip.h, mpcqp_rollout_slip; the host counterpart is
        gaits.rollout_slip_host): the rule of `stance_slip` takes the place of `stance_drive`'s, and after each tick every foot that
        stays in stance is moved by how far it slid.  ground [B] and foot_mass [B] are required; slip float64 [B,4,2], the feet's
        velocities, is state next to `x`, `ref`, `feet`, `legs` and `tick`, all advanced IN PLACE (zeros: every foot at rest).  Returns
        `rollout_drive`'s dict plus "slip_log" float64 [B,T,4,2], the velocities at the start of each row, and "disp" [B,T,4,2], what
        was added to the feet after the row; "flag" has bit 128 on the rows of a sliding leg.  On a ground that never limits (1e3) it is
        `rollout_drive` on that ground, bit for bit.  Every other argument as in `rollout_drive`.  Asynchronous on `stream`."""
        B, f64 = int(x.shape[0]), _torch().float64
        return self._rollout_legs(self.engine.rollout_slip_ptr, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land, body,
                                  push, push_ticks, substeps, gains, leg_substeps, inertia, geometry, log, stream, drive,
                                  operands=(("ground", ground, (B,), self.tdtype), ("foot_mass", foot_mass, (B,), self.tdtype),
                                            ("slip", slip, (B, 4, 2), f64)),
                                  logs=(("cmd", (12,), self.tdtype), ("slip_log", (4, 2), f64), ("disp", (4, 2), self.tdtype)))

    OBSERVE_LOGS = ("imu", "q_enc", "qd_enc", "est", "feet_est", "sigma", "nis")      # what `rollout_observe` adds, in the C order

    def rollout_observe(self, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, ground, foot_mass, slip, est_state,
                        feed="estimate", est_init=None, height=None, bias=None, noise=None, enc_noise=None, estimator=None, land="rule",
                        drive="limited", body=None, push=None, push_ticks=None, substeps=10, gains=None, leg_substeps=0, inertia=None,
                        geometry=None, log=True, stream=None, gate=None, attitude=None, att_state=None, compensate=None, dist_state=None):
        """`rollout_slip` with sensors and the state estimator inside the tick loop (include/mpcqp_observe.h, mpcqp_rollout_observe,
        which has the rule; the host counterpart is gaits.rollout_observe_host): per tick the encoders and the IMU are read off the
        live state, one row of `estimate_track` runs on est_state float64 [B,131] (state next to `x`, ..., `slip`, advanced IN PLACE;
        zeros: every filter starts from est_init [B,12], None = the robot's x), and with feed="estimate" the MPC's expand and solve read
        the estimate of the torso state and of the feet; with feed="truth" the estimator only shadows the loop, which is then
        `rollout_slip`'s bit for bit.  height [B,4] as in `estimate_track`, bias [B,6] and noise [B,T,6] as in `imu_log`, enc_noise
        [B,T,4,6] the (q, qd) noise per leg, `estimator` as in `estimate_track`.  Returns `rollout_slip`'s dict (the plant's truth) plus
        "imu" [B,T,6], "q_enc", "qd_enc" [B,T,4,3], "est" [B,T,12], "feet_est" [B,T,4,3], "sigma" [B,T,6] and "nis" [B,T].  Every
        other argument as in `rollout_slip`.  gate: None, or a dict of estimator.gate_row's fields ({} = the defaults) or an
        MpcQpTrustGate for mpcqp_rollout_observe_gated (include/mpcqp_gate.h): the filter's trust is the clock's gated per leg on the
        leg's velocity innovation, and the dict gains "trust" [B,T,4].  attitude: None (today's call through today's entry point), or a
        dict of estimator.attitude_row's fields ({} = the defaults) or an MpcQpAttitude for mpcqp_rollout_observe_aided
        (include/mpcqp_attitude.h): the velocity update's correction steers the orientation and a gyro-bias state; att_state float64
        [B,8] is state like est_state, advanced IN PLACE (None: a fresh zero one), and the dict gains "gyro_bias" [B,T,3] and
        "att_state".  compensate: None (today's call through today's entry points), or a dict for
        mpcqp_rollout_observe_compensated (include/mpcqp_compensate.h, which has the rule; the host counterpart is
        disturbance.rollout_compensated_host): the wrench observer of `disturbance_track` runs inside the tick and every `hold` ticks its
        estimate becomes the engine's disturbance table.  The dict has disturbance.observer_row's fields plus "source" ("truth": the
        observer reads x, the applied forces and the feet; "sensed": the estimate, the commanded forces and the estimated feet), "hold"
        (1) and "body" ([B,7], the body the observer believes, or None: the engine's model); {} = the defaults.  dist_state float64
        [B,40] is the observer's state, advanced IN PLACE (None: a fresh zero one); the dict gains "dist", "resid" [B,T,6] and
        "dist_state".  The call sets the engine's disturbance table from dist_state[:, :6] and leaves it set (`clear_disturbance`).
        Asynchronous on `stream`."""
        from . import estimator as _est
        B, T, f64 = int(x.shape[0]), int(T), _torch().float64
        if attitude is None and att_state is not None:
            raise ValueError("att_state needs attitude")
        if compensate is None and dist_state is not None:
            raise ValueError("dist_state needs compensate")
        feeds = {"truth": _capi.FEED_TRUTH, "estimate": _capi.FEED_ESTIMATE}
        if not isinstance(feed, int) and feed not in feeds:
            raise ValueError(f"feed must be 'truth' or 'estimate', got {feed!r}")
        check_operands(self.device, (("est_state", est_state, (B, _capi.EST_STATE), f64), ("est_init", est_init, (B, 12), self.tdtype),
                                     ("height", height, (B, 4), self.tdtype), ("bias", bias, (B, 6), self.tdtype),
                                     ("noise", noise, (B, T, 6), self.tdtype), ("enc_noise", enc_noise, (B, T, 4, 6), self.tdtype),
                                     ("att_state", att_state, (B, _capi.ATT_STATE), f64)),
                       optional=("est_init", "height", "bias", "noise", "enc_noise", "att_state"))
        tail = (feed if isinstance(feed, int) else feeds[feed], est_state.data_ptr(), _ptr(est_init), _ptr(height), _ptr(bias), _ptr(noise),
                _ptr(enc_noise), _est.estimator_struct(estimator))
        leg3 = ((4, 3), self.tdtype)
        call, more = self.engine.rollout_observe_ptr, ()
        if attitude is not None and att_state is None:
            att_state, = self._alloc(stream, ((B, _capi.ATT_STATE), f64, True))
        aided = (None if gate is None else _est.gate_struct(gate), 0 if gate is None else _capi.AIDED_GATE,
                 None if attitude is None else _est.attitude_struct(attitude), _ptr(att_state))
        if compensate is not None:
            from . import disturbance as _dist
            comp, obs_body = _dist.compensate_struct(compensate, gated=gate is not None, aided=attitude is not None)
            check_operands(self.device, (("compensate body", obs_body, (B, 7), self.tdtype), ("dist_state", dist_state, (B, _capi.DIST_STATE), f64)),
                           optional=("compensate body", "dist_state"))
            if dist_state is None:
                dist_state, = self._alloc(stream, ((B, _capi.DIST_STATE), f64, True))
            call = self.engine.rollout_observe_compensated_ptr
            more = (("trust", (4,), self.tdtype), ("gyro_bias", (3,), self.tdtype), ("dist", (6,), self.tdtype), ("resid", (6,), self.tdtype))
            tail += aided + (comp, _ptr(obs_body), dist_state.data_ptr())
        elif attitude is not None:
            call, more = self.engine.rollout_observe_aided_ptr, (("trust", (4,), self.tdtype), ("gyro_bias", (3,), self.tdtype))
            tail += aided
        elif gate is not None:
            call, more, tail = self.engine.rollout_observe_gated_ptr, (("trust", (4,), self.tdtype),), tail + (_est.gate_struct(gate),)
        out = self._rollout_legs(call, x, ref, feet, legs, gait, stand, gain, tick, mu, T, step_height, land, body, push, push_ticks, substeps,
                                  gains, leg_substeps, inertia, geometry, log, stream, drive,
                                  operands=(("ground", ground, (B,), self.tdtype), ("foot_mass", foot_mass, (B,), self.tdtype),
                                            ("slip", slip, (B, 4, 2), f64)),
                                  logs=(("cmd", (12,), self.tdtype), ("slip_log", (4, 2), f64), ("disp", (4, 2), self.tdtype),
                                        ("imu", (6,), self.tdtype), ("q_enc", *leg3), ("qd_enc", *leg3), ("est", (12,), self.tdtype),
                                        ("feet_est", *leg3), ("sigma", (6,), self.tdtype), ("nis", (), self.tdtype)) + more, tail=tail)
        if attitude is not None:
            out["att_state"] = att_state
        if compensate is not None:
            out["dist_state"] = dist_state
        if "trust" in out and gate is None:
            del out["trust"]
        if "gyro_bias" in out and attitude is None:
            del out["gyro_bias"]
        return out

    def score(self, logs, score=None, rule=None, stream=None):
        """The score row of a roll-out's logs, reduced on the device (include/mpcqp_sim.h, mpcqp_rollout_score; the host counterpart is
        score.score_host, the field names are score.FIELDS, score.summarize reads the figures off the rows): `logs` is the dict
        `rollout`, `rollout_plant`, `rollout_phase` or `rollout_legs` returns ("actual", "desired", "forces" [B,T,12] and "contact_log"
        uint8 [B,T,4], which the caller adds to the logs of the first two; the leg group when "tau", "qd" [B,T,4,3] and "flag" uint8
        [B,T,4] are all there, "miss" [B,T,4] when it is).  score=None: a fresh float64 [B, len(score.FIELDS)] tensor; a given one is
        combined with these rows IN PLACE and returned, its rows + bad_rows being the global index of this piece's first row (a long
        roll-out scored piece by piece: score.scored_rollout).  `rule`: None = the header's defaults, or (z_frac, tilt_max) / a dict, as
        score.rule_pair takes it.  Asynchronous on `stream`."""
        from . import score as _score
        torch = _torch()
        actual = logs.get("actual")
        if actual is None or actual.dim() != 3:
            raise ValueError("score needs the logs of a roll-out run with log=True")
        B, T = int(actual.shape[0]), int(actual.shape[1])
        rows, leg3, leg1, mask = (B, T, 12), (B, T, 4, 3), (B, T, 4), (B, T, 4)
        group = [logs.get(k) for k in ("tau", "qd", "flag")]
        if any(t is not None for t in group) and any(t is None for t in group):
            raise ValueError("the leg group is tau, qd and flag: all three or none")
        check_operands(self.device, (("actual", actual, rows, self.tdtype), ("desired", logs.get("desired"), rows, self.tdtype),
                                     ("forces", logs.get("forces"), rows, self.tdtype), ("contact_log", logs.get("contact_log"), mask, torch.uint8),
                                     ("tau", group[0], leg3, self.tdtype), ("qd", group[1], leg3, self.tdtype), ("flag", group[2], mask, torch.uint8),
                                     ("miss", logs.get("miss"), leg1, self.tdtype), ("score", score, (B, len(_score.FIELDS)), torch.float64)),
                       optional=("tau", "qd", "flag", "miss", "score"))
        st = self._stream(stream)
        accumulate = score is not None
        if score is None:
            score, = self._alloc(stream, ((B, len(_score.FIELDS)), torch.float64))
        self.engine.rollout_score_ptr(B, T, actual.data_ptr(), logs["desired"].data_ptr(), logs["forces"].data_ptr(), logs["contact_log"].data_ptr(),
                                      *[_ptr(t) for t in group], _ptr(logs.get("miss")), int(accumulate), score.data_ptr(),
                                      _score.rule_struct(rule), st.cuda_stream)
        return score

    def imu_log(self, logs, base_acc=None, body=None, bias=None, noise=None, estimator=None, stream=None):
        """What an IMU at the CoM reads on every row of a roll-out's logs (include/mpcqp_estimate.h, mpcqp_imu_log; the host counterpart
        is estimator.imu_log_host): `logs` with "actual", "forces" [B,T,12] and "feet_log" [B,T,4,3]; base_acc [B,T,6] = (alpha, a) or
        None for the unpushed plant's right-hand side formed with body [B,7] (None = the engine's model); bias [B,6] and noise [B,T,6]
        or None, added as given (draw the noise with torch); `estimator` None, a dict of estimator.estimator_row's fields or an
        MpcQpEstimator -> imu [B,T,6] = (gyro, specific force) in the torso's axes.  Asynchronous on `stream`."""
        from . import estimator as _est
        actual, forces, feet = logs.get("actual"), logs.get("forces"), logs.get("feet_log")
        if actual is None or actual.dim() != 3:
            raise ValueError("imu_log needs the logs of a roll-out run with log=True")
        B, T = int(actual.shape[0]), int(actual.shape[1])
        rows = ((B, T, 6), self.tdtype)
        check_operands(self.device, (("actual", actual, (B, T, 12), self.tdtype), ("forces", forces, (B, T, 12), self.tdtype),
                                     ("feet_log", feet, (B, T, 4, 3), self.tdtype), ("base_acc", base_acc, *rows),
                                     ("body", body, (B, 7), self.tdtype), ("bias", bias, (B, 6), self.tdtype), ("noise", noise, *rows)),
                       optional=("base_acc", "body", "bias", "noise"))
        st = self._stream(stream)
        imu, = self._alloc(stream, rows)
        self.engine.imu_log_ptr(B, T, actual.data_ptr(), forces.data_ptr(), feet.data_ptr(), _ptr(base_acc), _ptr(body), _ptr(bias),
                                _ptr(noise), imu.data_ptr(), _est.estimator_struct(estimator), st.cuda_stream)
        return imu

    from .estimator import OUT as EST_OUT      # ("est", "feet", "sigma", "nis"): the host counterpart's names, in the C order

    def estimate_track(self, imu, q, qd, contact_log, init, trust=None, height=None, state=None, estimator=None, geometry=None,
                       want=EST_OUT, stream=None, gate=None, attitude=None, att_state=None):
        """The torso state estimated from the IMU and the leg encoders over the rows of a log (include/mpcqp_estimate.h,
        mpcqp_estimate_track, which has the rule; the host counterparts are estimator.estimate_track_host and estimate_joint_host):
        imu [B,T,6] as `imu_log` returns it, q, qd [B,T,4,3] the "q" / "qd" logs of `rollout_legs`, `rollout_drive`, `rollout_slip` or
        of `joint_rates`, contact_log uint8 [B,T,4], init [B,12] in the layout of an `actual` row; trust [B,T,4] in [0,1] or None
        (contact != 0), height [B,4] the ground under each foot or None, state float64 [B,131] advanced IN PLACE (zeros: start from
        init) or None -> {"est" [B,T,12] in the layout of `actual`, "feet" [B,T,4,3], "sigma" [B,T,6], "nis" [B,T]}; an output not in
        `want` is None.  gate: None, or a dict of estimator.gate_row's fields ({} = the defaults) or an MpcQpTrustGate for
        mpcqp_estimate_track_gated (include/mpcqp_gate.h): every row's trust is gated per leg on the leg's velocity innovation, and the
        dict gains "trust" [B,T,4], the trust the rows used.  attitude: None (today's call through today's entry point), or a dict of
        estimator.attitude_row's fields ({} = the defaults) or an MpcQpAttitude for mpcqp_estimate_track_aided
        (include/mpcqp_attitude.h); att_state float64 [B,8] goes with `state` and is advanced IN PLACE (None: a fresh zero one), and the
        dict gains "gyro_bias" [B,T,3] and "att_state".  Asynchronous on `stream`."""
        from . import estimator as _est
        torch = _torch()
        if attitude is None and att_state is not None:
            raise ValueError("att_state needs attitude")
        B, T = int(imu.shape[0]), int(imu.shape[1]) if imu.dim() == 3 else -1
        legs = ((B, T, 4, 3), self.tdtype)
        check_operands(self.device, (("imu", imu, (B, T, 6), self.tdtype), ("q", q, *legs), ("qd", qd, *legs),
                                     ("contact_log", contact_log, (B, T, 4), torch.uint8), ("init", init, (B, 12), self.tdtype),
                                     ("trust", trust, (B, T, 4), self.tdtype), ("height", height, (B, 4), self.tdtype),
                                     ("state", state, (B, _capi.EST_STATE), torch.float64),
                                     ("att_state", att_state, (B, _capi.ATT_STATE), torch.float64)),
                       optional=("trust", "height", "state", "att_state"))
        unknown = set(want) - set(self.EST_OUT)
        if unknown or not want:
            raise ValueError(f"want must name at least one of {self.EST_OUT}, got {tuple(want)}")
        st = self._stream(stream)
        spec = {"est": ((B, T, 12), self.tdtype), "feet": legs, "sigma": ((B, T, 6), self.tdtype), "nis": ((B, T), self.tdtype)}
        out = dict(zip(self.EST_OUT, self._alloc(stream, *[spec[k] if k in want else None for k in self.EST_OUT])))
        head = (B, T, imu.data_ptr(), q.data_ptr(), qd.data_ptr(), contact_log.data_ptr(), _ptr(trust), _ptr(height), init.data_ptr(), _ptr(state),
                *[_ptr(out[k]) for k in self.EST_OUT])
        if attitude is not None:
            if att_state is None:
                att_state, = self._alloc(stream, ((B, _capi.ATT_STATE), torch.float64, True))
            if gate is not None:
                out["trust"], = self._alloc(stream, ((B, T, 4), self.tdtype))
            out["gyro_bias"], = self._alloc(stream, ((B, T, 3), self.tdtype))
            out["att_state"] = att_state
            self.engine.estimate_track_aided_ptr(*head, _ptr(out.get("trust")), out["gyro_bias"].data_ptr(), _est.estimator_struct(estimator),
                                                 None if gate is None else _est.gate_struct(gate), 0 if gate is None else _capi.AIDED_GATE,
                                                 _est.attitude_struct(attitude), att_state.data_ptr(), geometry, st.cuda_stream)
        elif gate is None:
            self.engine.estimate_track_ptr(*head, _est.estimator_struct(estimator), geometry, st.cuda_stream)
        else:
            out["trust"], = self._alloc(stream, ((B, T, 4), self.tdtype))
            self.engine.estimate_track_gated_ptr(*head, out["trust"].data_ptr(), _est.estimator_struct(estimator), _est.gate_struct(gate),
                                                 geometry, st.cuda_stream)
        return out

    def last_kernel_ms(self):
        return self.engine.last_kernel_ms()
