"""Developer tool: the stance rule of this tree against another build of the library (the parent commit's, built from a worktree),
bit for bit, in one process -- both opened through MPCBatch(library=...): stance_drive / stance_slip on the draws of
tests/drive_cases.py, slip_cases.py, actuator_cases.py and slip_rows_cases.py, rollout_drive (ground None and set, drive limited and ideal) and rollout_slip
(ground 0.3, 1e3 and the case's own) on the combined case of tests/slip_rows_cases.py (B = 16, T = 25), tiled to B = 2560 and cut to
B = 2557 (a ragged last block); f32 and f64 I/O, with and without an actuator table.  A value differs when any of its bytes does.
Prints one line per comparison and the totals, writes them to the report file too; exit status 1 when anything differs.
profiles/r22_stance_rule_parent.txt is its output.
usage: python tools/stance_rule_compare.py <other libmpcqp.so> <report file>"""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np, torch
import mpcqp
import actuator_cases as ac, drive_cases as dc, slip_cases as sc, slip_rows_cases as rc, models_rollout_cases as C
import test_gpu_models_rollouts as mr

parent = mpcqp.Library(sys.argv[1])
new = mpcqp.product_library()
assert os.path.abspath(parent.path) != os.path.abspath(new.path)
report = open(sys.argv[2], "w")
total = {"calls": 0, "arrays": 0, "values": 0, "differing": 0}


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True); report.write(line + "\n"); report.flush()


def t(a, dt):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def compare(tag, a, b):
    """a, b: dicts of numpy arrays from the parent and the new library."""
    assert list(a) == list(b), (tag, list(a), list(b))
    bad, n = [], 0
    for k in a:
        if a[k] is None and b[k] is None:
            continue
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (tag, k)
        w = x.view(np.uint8).reshape(-1) != y.view(np.uint8).reshape(-1)
        d = int(w.reshape(-1, x.dtype.itemsize).any(axis=1).sum()) if x.size else 0
        total["arrays"] += 1; total["values"] += x.size; total["differing"] += d; n += x.size
        if d:
            bad.append(f"{k}: {d} of {x.size}")
    total["calls"] += 1
    say(f"{'same' if not bad else 'DIFF'}  {tag}: {len(a)} outputs, {n} values" + ("" if not bad else "  " + "; ".join(bad)))


def engines(io):
    kw = dict(N=10, delta=0.03, io_dtype=io, precision="mixed", max_iter=mr._cap())
    return mpcqp.MPCBatch(library=parent, **kw), mpcqp.MPCBatch(**kw)


def numpy_of(out):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def rule(sol, c, slip, table):
    dt = sol.tdtype
    if table is not None:
        sol.set_actuators(table)
    try:
        a = [t(c["x"], dt), t(c["f"], dt), t(c["feet"], dt), t(c["contact"], torch.uint8)]
        if slip:
            return numpy_of(sol.stance_slip(*a, t(c["ground"], dt), t(c["foot_mass"], dt), t(c["slip"], torch.float64), substeps=slip))
        return numpy_of(sol.stance_drive(*a, t(c["ground"], dt)))
    finally:
        if table is not None:
            sol.clear_actuators()


def rollout(sol, K, kind, ground, table, T, drive="limited"):
    d = mr._dev(sol, K["pb"])
    sol.set_models(K["rows"])
    if table:
        sol.set_actuators(K["act"])
    try:
        a = [d[k] for k in C.LEGS_ARGS] + [T, d["step_height"]]
        g = None if ground is None else t(np.where(np.arange(len(K["ground"])) % 2 == 0, ground, K["ground"]), sol.tdtype)
        if kind == "slip":
            slip = t(K["slip"], torch.float64)
            out = numpy_of(sol.rollout_slip(*a, g, t(K["foot_mass"], sol.tdtype), slip, "actual", drive, **mr._plant(sol, K["pr"])))
            out["slip"] = slip.cpu().numpy()
        else:
            out = numpy_of(sol.rollout_drive(*a, "actual", drive, g, **mr._plant(sol, K["pr"])))
        out.update({k: d[k].cpu().numpy() for k in ("x", "ref", "feet", "legs", "tick")})
        return out
    finally:
        sol.clear_actuators(); sol.clear_models()


def tiled(K, reps):
    rep = lambda v: np.tile(v, (reps,) + (1,) * (v.ndim - 1))
    cut = lambda d: {k: (rep(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    return dict(K, pb=cut(K["pb"]), pr=cut(K["pr"]), **{k: rep(K[k]) for k in ("rows", "act", "acls", "ground", "foot_mass", "slip")})


K = rc.combined_case()
for io in ("f32", "f64"):
    sp, sn = engines(io)
    plain, moving = dc.clamp_draw(), ac.drive_draw()
    noground = dc.clamp_draw(ground=False)
    sdraw, rdraw = sc.slip_draw(), rc.rows_draw()
    for table in (None, moving["rows"]):
        tag = f"{io} table={'yes' if table is not None else 'no'}"
        for name, c in (("drive_cases.clamp_draw", plain), ("drive_cases.clamp_draw(ground=False)", noground), ("actuator_cases.drive_draw", moving)):
            compare(f"stance_drive {tag} {name}", rule(sp, c, 0, table), rule(sn, c, 0, table))
        for name, c in (("slip_cases.slip_draw", sdraw), ("slip_rows_cases.rows_draw", rdraw)):
            for n in (10, 4):
                compare(f"stance_slip {tag} substeps={n} {name}", rule(sp, c, n, table), rule(sn, c, n, table))
    for table in (False, True):
        tag = f"{io} table={'yes' if table else 'no'} B=16 T=25"
        for ground in (None, 0.3, rc.LOW_MU):
            compare(f"rollout_drive {tag} ground={ground}", rollout(sp, K, "drive", ground, table, K["T"]), rollout(sn, K, "drive", ground, table, K["T"]))
        # drive = ideal without a ground row: the log step with only_changed
        compare(f"rollout_drive(ideal) {tag} ground=None", rollout(sp, K, "drive", None, table, K["T"], "ideal"), rollout(sn, K, "drive", None, table, K["T"], "ideal"))
        compare(f"rollout_slip(ideal) {tag} ground=0.3", rollout(sp, K, "slip", 0.3, table, K["T"], "ideal"), rollout(sn, K, "slip", 0.3, table, K["T"], "ideal"))
        for ground in (0.3, 1e3, rc.LOW_MU):
            compare(f"rollout_slip {tag} ground={ground}", rollout(sp, K, "slip", ground, table, K["T"]), rollout(sn, K, "slip", ground, table, K["T"]))
    big = tiled(K, 160)        # B = 2560: ten blocks of 1024 legs, and the drive without logs' queued launch
    compare(f"rollout_slip {io} table=yes B=2560 T=4 ground={rc.LOW_MU}", rollout(sp, big, "slip", rc.LOW_MU, True, 4), rollout(sn, big, "slip", rc.LOW_MU, True, 4))
    compare(f"rollout_drive {io} table=yes B=2560 T=4 ground={rc.LOW_MU}", rollout(sp, big, "drive", rc.LOW_MU, True, 4), rollout(sn, big, "drive", rc.LOW_MU, True, 4))
    odd = {k: (v[:2557] if isinstance(v, np.ndarray) else v) for k, v in big.items() if k not in ("pb", "pr")}
    odd["pb"] = {k: (v[:2557] if isinstance(v, np.ndarray) else v) for k, v in big["pb"].items()}
    odd["pr"] = {k: (v[:2557] if isinstance(v, np.ndarray) else v) for k, v in big["pr"].items()}
    compare(f"rollout_slip {io} table=yes B=2557 T=4 ground=0.3 (ragged last block)", rollout(sp, odd, "slip", 0.3, True, 4), rollout(sn, odd, "slip", 0.3, True, 4))
    sp.engine.close(); sn.engine.close()
say(f"total: {total['calls']} comparisons, {total['arrays']} arrays, {total['values']} values, {total['differing']} differing")
sys.exit(1 if total["differing"] else 0)
