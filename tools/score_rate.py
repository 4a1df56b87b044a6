"""Developer tool: rate of the score reduction (include/mpcqp_sim.h, mpcqp_rollout_score) on a rollout_legs log -- the named trot
(period 10) of tools/rollout_legs_rate.py, land = actual, heterogeneous bodies and pushes -- at B = 4096 and 65 536 robots x T = 50
ticks, fp32 and fp64 I/O.  Per log row the kernel reads actual, desired, forces (36 values), tau, qd (24), miss (4) and two dwords of
masks: 64 values + 8 bytes = 264 B in fp32, 520 B in fp64, and writes 33 doubles per robot.  Two figures per case, from the same logs in
the same run, each one call timed with HIP events (median and best of 20 after 3 warm-ups, the raw call: no allocation in the window):

    score          the kernel; achieved bytes/s against the 8 TB/s of the HBM3E specification (6.3 TB/s is what a copy reaches)
    torch_card     the same 33 fields composed from torch operations in float64 (what a user could do before this call; it allocates
                   its temporaries, which is part of what it costs), median of 5 after one warm-up; its result is compared with the kernel's

usage: score_rate.py [--size B] [--io f32|f64]"""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mpcqp
from mpcqp import gaits, score

T, B0, STEP_HEIGHT, HBM_TBPS = 50, 64, 0.06, 8.0
SIZES = (int(sys.argv[sys.argv.index("--size") + 1]),) if "--size" in sys.argv else (4096, 65536)
IOS = (sys.argv[sys.argv.index("--io") + 1],) if "--io" in sys.argv else ("f32", "f64")
I = score.INDEX


def timed(fn, reps=20, warm=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms))


def torch_card(logs, z_frac=score.Z_FRAC, tilt_max=score.TILT_MAX):
    """The score row from torch operations, float64 [B,33]."""
    d = lambda k: logs[k].double()
    xa, xd, f = d("actual"), d("desired"), d("forces")
    B, T = xa.shape[:2]
    fin = torch.isfinite(xa).all(-1) & torch.isfinite(xd).all(-1) & torch.isfinite(f).all(-1)
    z = torch.zeros((), dtype=torch.float64, device=xa.device)
    xa, xd, f = (torch.where(fin[..., None], a, z) for a in (xa, xd, f))
    tot = lambda v: torch.where(fin, v, z).sum(1)
    top = lambda v: torch.where(fin, v, z).amax(1).clamp_min(0)
    out = torch.zeros((B, len(score.FIELDS)), dtype=torch.float64, device=xa.device)
    out[:, I["rows"]], out[:, I["bad_rows"]] = fin.sum(1), (~fin).sum(1)
    dz = xa[..., 5] - xd[..., 5]
    out[:, I["z_sq"]], out[:, I["z_max"]] = tot(dz * dz), top(dz.abs())
    ev = ((xa[..., 9:11] - xd[..., 9:11]) ** 2).sum(-1)
    out[:, I["vel_sq"]], out[:, I["vel_max"]] = tot(ev), top(ev.sqrt())
    ea = ((xa[..., :3] - xd[..., :3]) ** 2).sum(-1)
    out[:, I["ang_sq"]], out[:, I["ang_max"]] = tot(ea), top(ea.sqrt())
    tilt = (xa[..., 0] ** 2 + xa[..., 1] ** 2).sqrt()
    out[:, I["tilt_max"]], out[:, I["vx_sum"]], out[:, I["vy_sum"]] = top(tilt), tot(xa[..., 9]), tot(xa[..., 10])
    down = ~fin | (xa[..., 5] < z_frac * xd[..., 5]) | (tilt > tilt_max)
    out[:, I["fall_row"]] = torch.where(down.any(1), down.int().argmax(1), -1)
    st = (logs["contact_log"] != 0) & fin[..., None]
    fl = f.view(B, T, 4, 3)
    out[:, I["f_sq"]] = torch.where(st, (fl ** 2).sum(-1), z).sum((1, 2))
    out[:, I["fz_max"]] = torch.where(st, fl[..., 2], z).amax((1, 2)).clamp_min(0)
    up = st & (fl[..., 2] > 0)
    out[:, I["fric_max"]] = torch.where(up, fl[..., :2].abs().amax(-1) / torch.where(up, fl[..., 2], z + 1), z).amax((1, 2))
    out[:, I["stance_rows_0"]:I["stance_rows_3"] + 1] = st.sum(1)
    out[:, I["flight_rows"]] = (fin & ~(logs["contact_log"] != 0).any(-1)).sum(1)
    tq, qd, flag = d("tau"), d("qd"), logs["flag"]
    ok = fin[..., None] & (flag != 0xff) & torch.isfinite(tq).all(-1) & torch.isfinite(qd).all(-1)
    tq, qd = torch.where(ok[..., None], tq, z), torch.where(ok[..., None], qd, z)
    p = (tq * qd).sum(-1)
    out[:, I["tau_max"]], out[:, I["tau_sq"]] = tq.abs().amax((1, 2, 3)), (tq ** 2).sum((1, 2, 3))
    out[:, I["work_pos"]], out[:, I["work_abs"]] = p.clamp_min(0).sum((1, 2)), p.abs().sum((1, 2))
    for name, bit in score.FLAG_BITS.items():
        out[:, I[name]] = (ok & ((flag & bit) != 0)).sum((1, 2))
    out[:, I["poisoned_rows"]] = (fin[..., None] & ~ok).sum((1, 2))
    m = d("miss")
    out[:, I["landings"]] = (fin[..., None] & (m != 0)).sum((1, 2))
    m = torch.where(fin[..., None] & torch.isfinite(m), m, z)
    out[:, I["miss_max"]], out[:, I["miss_sq"]] = m.amax((1, 2)).clamp_min(0), (m ** 2).sum((1, 2))
    return out


trot = gaits.make_phase_batch(B0, "trot", 10, seed=9)
for B in SIZES:
    rows = mpcqp.synth.make_plant_rows(B, seed=1, push_start=(10, 30))
    for io in IOS:
        el = 4 if io == "f32" else 8
        sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype=io, precision="mixed", warm_start=True, warm_shift=True)
        sol.engine.reserve(B)
        dt = sol.tdtype
        tiled = lambda a, d: torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * (B // B0), axis=0)), dtype=d).cuda().contiguous()
        up = lambda a, d=dt: torch.as_tensor(a, dtype=d).cuda()
        logs = sol.rollout_legs(tiled(trot["x"], dt), tiled(trot["ref"], dt), tiled(trot["feet"], dt),
                                torch.zeros((B, 4, 7), dtype=torch.float64, device="cuda"), tiled(trot["gait"], torch.int32),
                                tiled(trot["stand"], dt), tiled(trot["gain"], dt), tiled(trot["tick"], torch.int32), tiled(trot["mu"], dt), T,
                                torch.full((B,), STEP_HEIGHT, dtype=dt, device="cuda"), "actual", body=up(rows["body"]), push=up(rows["push"]),
                                push_ticks=up(rows["push_ticks"], torch.int32))
        logs = {k: logs[k] for k in ("actual", "desired", "forces", "contact_log", "tau", "qd", "flag", "miss")}   # (the rest is freed)
        out = sol.score(logs)
        torch.cuda.synchronize()
        st = torch.cuda.current_stream().cuda_stream
        ptr = [logs[k].data_ptr() for k in logs]
        med, best = timed(lambda: sol.engine.rollout_score_ptr(B, T, *ptr, 0, out.data_ptr(), stream=st))
        med_t, best_t = timed(lambda: torch_card(logs), reps=5, warm=1)
        card = torch_card(logs)
        by = B * T * (64 * el + 8) + B * 8 * len(score.FIELDS)
        exact = [n for n in score.FIELDS if n.endswith("rows") or n.startswith("stance_rows") or n in ("landings", "fall_row")]
        rel = ((out - card).abs() / torch.maximum(out.abs(), card.abs()).clamp_min(1e-300)).amax(0)
        vabs = logs["actual"][:, :, 9:11].double().abs().sum(1)                 # (the velocity sums cancel: against sum |v|)
        for j, n in enumerate(("vx_sum", "vy_sum")):
            rel[I[n]] = ((out[:, I[n]] - card[:, I[n]]).abs() / vabs[:, j].clamp_min(1e-300)).max()
        fig = score.summarize(out, 0.03, mass=sol.cfg.m)
        print(json.dumps({"call": "score", "io": io, "B": B, "T": T, "ms_median": round(med, 4), "ms_best": round(best, 4), "MB": round(by / 1e6, 1),
                          "bytes_per_row": 64 * el + 8, "TBps": round(by / med / 1e9, 3), "share_of_8TBps_roof": round(by / med / 1e9 / HBM_TBPS, 3),
                          "G_rows_per_s": round(B * T / med / 1e6, 3), "torch_card_ms_median": round(med_t, 3), "torch_card_ms_best": round(best_t, 3),
                          "times_faster_than_torch_card": round(med_t / med, 1),
                          "counts_equal_torch_card": bool(all(torch.equal(out[:, I[n]], card[:, I[n]]) for n in exact)),
                          "worst_rel_diff_to_torch_card": float(rel.max()), "fell": int(fig["fell"].sum()),
                          "z_rms_mm_median": round(float(fig["z_rms"].median()) * 1e3, 3),
                          "miss_max_mm": round(float(fig["miss_max"].max()) * 1e3, 2), "cot_median": round(float(fig["cot"].nanmedian()), 4)}),
              flush=True)
        del logs, out, card
        sol.engine.close()
