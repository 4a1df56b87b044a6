"""BASELINE configs 4 and 5 under pytest (-m gpu), at their full sizes through size-independent properties (no 65 536-QP oracle
run), plus the multi-rank bench rehearsal.

* config 4: B = 65 536 and the per-GPU shard B = 8 192 of the config-3 distribution (seed 20250810): every constraint of
  src/mpc.py:138-173, exactly zero swing forces, bitwise determinism, queued launch form == plain form on a slice, and
  oracle parity on a slice of 256.
* config 5: B = 4 096, N = 20: the same properties; all-fp64 arithmetic at N = 20 against the oracle (tolerance 1e-4 relative
  on the GRFs, as everywhere); the ADMM-only mode (OSQP termination test, no polish) in fp32-tile and fp64 arithmetic.
* `bench.py --gpus 2` as a fresh torch.distributed.run child with the gloo backend (started by conftest.py before this
  process touches the GPU): one JSON line, n_gpus = 2, whole-job value = 2 ranks x per-rank batches.
* the plain `bench.py --gpus 1` run with `--dump-outputs` (also a child started by conftest.py): its line and its last step's results.
"""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import mpcqp
import qp_spec as S
from batch_checks import check_batch
from conftest import rel_err, bench2_result, bench_plain_result
from test_gpu_parity import gpu_solve, solved

pytestmark = pytest.mark.gpu


def _check_properties(b, out, N, tol=1e-3):
    B = len(b["mu"])
    ok = solved(out["status"])
    u = out["u"].astype(np.float64).reshape(B, N, 4, 3)
    c = b["contact"].astype(bool)
    mu = b["mu"][:, None, None]
    assert np.all(u[~c] == 0)                                              # swing legs: exactly zero (src/mpc.py:139-144)
    fz = u[..., 2]
    m = c & ok[:, None, None]
    assert np.all(fz[m] >= 3 - tol) and np.all(fz[m] <= 100 + tol)         # src/mpc.py:45-46,151-157
    assert np.all((np.abs(u[..., 0]) <= mu * fz + tol)[ok]) and np.all((np.abs(u[..., 1]) <= mu * fz + tol)[ok])   # :159-173
    return ok


@pytest.mark.parametrize("B", [8192, 65536])
def test_config4_full_size_properties(oracle_solve, B):
    b = mpcqp.synth.config4(B)
    out = gpu_solve(b, io="f32", precision="mixed", want_X=False)
    ok = _check_properties(b, out, 10)
    assert ok.mean() >= 0.999, ok.mean()
    out2 = gpu_solve(b, io="f32", precision="mixed", want_X=False)
    assert np.array_equal(out["u"], out2["u"]) and np.array_equal(out["status"], out2["status"])     # bitwise repeatable
    # the queued form is a pure re-ordering: a slice solved in the plain form gives the same bits
    sl = {k: (v[1000:1256] if isinstance(v, np.ndarray) and len(v) == B else v) for k, v in b.items()}
    plain = gpu_solve(sl, io="f32", precision="mixed", want_X=False, flags=mpcqp.FLAG_POLISH | mpcqp.FLAG_NATURAL_ORDER)
    assert np.array_equal(plain["u"], out["u"][1000:1256]) and np.array_equal(plain["iters"], out["iters"][1000:1256])
    # and the slice agrees with the oracle
    ref = oracle_solve(sl)
    oks = solved(plain["status"])
    assert rel_err(plain["u"], ref["u"])[oks].max() <= 1e-4


def test_config5_full_size_properties():
    b = mpcqp.synth.config5(4096)
    out = gpu_solve(b, N=20, io="f32", precision="mixed")
    ok = _check_properties(b, out, 20)
    assert ok.mean() >= 0.999, ok.mean()      # (the ADMM block inverts S in fp64 at this horizon: 99.98 % measured, 99.78 % before)
    out2 = gpu_solve(b, N=20, io="f32", precision="mixed")
    assert np.array_equal(out["u"], out2["u"]) and np.array_equal(out["status"], out2["status"])
    # eight device-fills of four-wave workgroups: the queued form; a slice in the plain form gives the same bits
    sl = {k: (v[3000:3200] if isinstance(v, np.ndarray) and len(v) == 4096 else v) for k, v in b.items()}
    plain = gpu_solve(sl, N=20, io="f32", precision="mixed", flags=mpcqp.FLAG_POLISH | mpcqp.FLAG_NATURAL_ORDER)
    assert np.array_equal(plain["u"], out["u"][3000:3200]) and np.array_equal(plain["iters"], out["iters"][3000:3200])
    cfg = S.QPConfig(N=20, delta=0.03, alpha=1e-2)
    for i in range(0, 4096, 1024):
        X = S.predict_states(b["x0"][i], out["u"][i].astype(np.float64).reshape(-1), b["r"][i], b["contact"][i], cfg)
        assert np.abs(X - out["X"][i]).max() <= 5e-4        # fp32 outputs, 20 stages


@pytest.mark.parametrize("precision", ["mixed", "f64"])
def test_config5_precisions_against_oracle(oracle_solve, precision):
    b = mpcqp.synth.config5(256)
    ref = oracle_solve(b, N=20)
    out = gpu_solve(b, N=20, io="f64", precision=precision)
    check_batch(out, b, ref, max_iter=out["max_iter"], allowed=0, what=f"config5 {precision}")


def test_config5_f64_full_size_all_solved():
    b = mpcqp.synth.config5(4096)
    out = gpu_solve(b, N=20, io="f32", precision="f64")
    ok = _check_properties(b, out, 20)
    assert ok.mean() >= 0.9995, ok.mean()     # 100 % measured


@pytest.mark.parametrize("N", [10, 20])
def test_admm_iterate_is_the_oracles_osqp_iterate(oracle_lib, N):
    """Polish off, tolerances 0, exactly K <= 25 iterations (no rho adaptation inside): the all-fp64 engine must return the
    iterate of the oracle's OSQP loop (oracle/mpcqp_oracle.c: same rho / sigma / relaxation, dense Cholesky solves) to rounding
    -- the two share no linear algebra -- and the fp32-tile engine the same iterate to its solve accuracy."""
    b = mpcqp.synth.config3(128) if N == 10 else mpcqp.synth.config5(128)
    for K in (3, 25):
        kw = dict(flags=0, eps_abs=0.0, eps_rel=0.0, max_iter=K, check_every=K)
        cfg = oracle_lib.default_config(N=N, delta=0.03, **kw)
        ref = mpcqp.Engine(oracle_lib, cfg).solve_batch_host(b["x0"], b["r"], b["contact"], b["xdes"], b["mu"])
        assert np.all(mpcqp.split_iters(ref["iters"])[0] == K)
        for precision, tol in (("f64", 1e-9), ("mixed", 2e-3 if N == 10 else 1e-2)):
            out = gpu_solve(b, N=N, io="f64", precision=precision, **kw)
            assert np.all(mpcqp.split_iters(out["iters"])[0] == K) and np.all((out["status"] == 3) | (out["status"] == 2))   # (2: a QP whose residuals are exactly 0)
            assert rel_err(out["u"], ref["u"]).max() <= tol, (N, K, precision, rel_err(out["u"], ref["u"]).max())


@pytest.mark.parametrize("N,precision", [(10, "mixed"), (10, "f64"), (20, "mixed"), (20, "f64")])
def test_admm_only_mode(oracle_solve, N, precision):
    """Polish off (what the reference runs: OSQP with its own termination test, src/mpc.py:51-55): status 2 = residuals under
    eps_abs + eps_rel * norm.  fp64 ADMM run to 1e-8 reaches the oracle to 1e-4; fp32 tiles stall near their rounding floor,
    which is why the default mode polishes (measured floor: profiles/r02_config5_sweep.json)."""
    b = mpcqp.synth.config3(64) if N == 10 else mpcqp.synth.config5(64)
    ref = oracle_solve(b, N=N)
    eps = 1e-8 if precision == "f64" else 1e-3                    # (1e-3 = OSQP's default, what the reference runs with)
    out = gpu_solve(b, N=N, io="f64", precision=precision, flags=0, max_iter=20000, check_every=200, eps_abs=eps, eps_rel=eps)
    st = out["status"]
    assert np.all((st == 2) | (st == 3))
    conv = st == 2
    assert conv.mean() >= (0.95 if precision == "f64" else 0.5)
    tol = 1e-4 if precision == "f64" else 0.5             # OSQP-default tolerances leave the GRFs this loose (cf. the reference log)
    assert rel_err(out["u"], ref["u"])[conv].max() <= tol


def test_horizon20_warm_start_same_optimum(oracle_solve):
    """Warm start at N = 20 (per-slot multiplier record of 4 N x 5 rows): restarting from the optimum costs no ADMM block, and
    the answer is the cold one."""
    b = mpcqp.synth.config5(96)
    cold = gpu_solve(b, N=20, io="f64", precision="mixed")
    sol = mpcqp.MPCBatch(N=20, delta=0.03, io_dtype="f64", precision="mixed", warm_start=True)
    dev = sol.upload(b)
    o1 = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"]); torch.cuda.synchronize()
    u1 = o1["u"].cpu().numpy().copy(); it1 = o1["iters"].cpu().numpy().copy()
    o2 = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"]); torch.cuda.synchronize()   # seeded with its own solution
    u2 = o2["u"].cpu().numpy(); it2 = o2["iters"].cpu().numpy(); st2 = o2["status"].cpu().numpy()
    ok = check_batch(cold, b, None, max_iter=cold["max_iter"], allowed=0, what="cold") & check_batch(
        {"u": u2, "status": st2, "iters": it2}, b, None, max_iter=sol.cfg.max_iter, allowed=0, what="warm")
    assert rel_err(u1, cold["u"])[ok].max() <= 1e-6 and rel_err(u2, cold["u"])[ok].max() <= 1e-4
    assert mpcqp.split_iters(it2)[0][ok].mean() < 0.2 * mpcqp.split_iters(it1)[0][ok].mean()          # (nearly) no ADMM iterations on the restart


def test_two_rank_bench_rehearsal():
    """bench.py --gpus 2 (gloo, both ranks on this one GPU), launched as a fresh child before this process initialised HIP: the weak
    mode the driver's scaling runs use (4096 QPs per rank, one draw per rank) and the strong mode of BASELINE configs[3]
    (--global-batch: one batch in contiguous shards, here ragged: 3001 + 3000)."""
    rc, stdout, stderr = bench2_result()
    assert rc == 0, stderr[-2000:]
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 2, stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["scaling"] == "weak" and j["unit"] == "QP solves/s"
    assert j["config"]["allgather"] is True and j["config"]["batch_per_gpu"] == 4096 and j["config"]["global_batch"] == 8192
    assert "one draw per rank" in j["config"]["shards"]
    # whole-job value = units all ranks processed / max-over-ranks time; the per-rank times are reported next to it
    assert abs(j["value"] - 2 * 4096 * 3 / (j["ms_per_step"] * 3e-3)) <= 1e-6 * j["value"]
    rk = j["rank_kernel_ms"]
    assert len(rk["per_rank"]) == 2 and rk["min"] <= rk["mean"] <= rk["max"] and rk["max"] == j["roofline"]["kernel_ms"]
    assert j["config"]["solved_fraction"] >= 0.999 and "roofline" in j and "cpu_baseline" not in j
    k = json.loads(lines[1])
    assert k["n_gpus"] == 2 and k["scaling"] == "strong" and k["config"]["global_batch"] == 6001 and k["config"]["batch_per_gpu"] == 3001
    assert abs(k["value"] - 6001 * 3 / (k["ms_per_step"] * 3e-3)) <= 1e-6 * k["value"]
    assert k["config"]["solved_fraction"] >= 0.999 and len(k["rank_kernel_ms"]["per_rank"]) == 2


def test_plain_bench_line_and_dumped_outputs():
    """The plain run the benchmark is measured with (`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR`): one JSON line with
    the headline fields and none of the `--full` figures, and the results of its last timed step, as dumped, equal to a solve of the
    same seeded batch with the same settings in this process."""
    rc, stdout, stderr, d = bench_plain_result()
    try:
        assert rc == 0, stderr[-2000:]
        lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, stdout[-2000:]
        j = json.loads(lines[0])
        assert j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "QP solves/s" and j["higher_is_better"] is True
        assert j["dtype"] == "f32 tiles + f64 residuals" and j["ms_per_step"] > 0
        assert abs(j["value"] - 4096 * 3 / (j["ms_per_step"] * 3e-3)) <= 1e-6 * j["value"]
        assert "roofline" in j and "cpu_baseline" not in j and "breakdown" not in j
        got = {k: np.load(os.path.join(d, k + ".npy")) for k in ("u", "res", "status", "iters")}
        assert sorted(os.listdir(d)) == ["iters.npy", "res.npy", "status.npy", "u.npy"]
        assert got["u"].dtype == np.float32 and got["u"].shape == (4096, 10, 12)
        assert got["res"].dtype == np.float32 and got["res"].shape == (4096, 2)
        assert got["status"].dtype == np.float64 and got["iters"].dtype == np.float64 and got["status"].shape == (4096,)
        b = mpcqp.synth.make_batch(4096, 10, 0.03, 20250809, ("trot", "pronk", "amble", "gallop"), (0.3, 0.5, 0.7, 1.0))
        sol = mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed", flags=mpcqp.FLAG_POLISH | mpcqp.FLAG_NO_TIMING, first_block=0)
        dev = sol.upload(b)
        want = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"])
        torch.cuda.synchronize()
        check_batch({"u": got["u"], "status": got["status"].astype(np.int32), "iters": got["iters"].astype(np.int64)}, b, None,
                    max_iter=sol.cfg.max_iter, allowed=0, what="bench dump")
        for k in ("u", "res", "status", "iters"):
            assert np.array_equal(got[k], want[k].cpu().numpy()), k
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_one_rank_rccl_bench_rehearsal():
    """The RCCL branch of bench.py (backend "nccl": device-side process group, barrier, all-reduce, all-gather into a device
    tensor) with one rank on this box's GPU -- the calls the driver's 2/4/8-GPU runs make, which no one-GPU box can run at size."""
    from conftest import bench1_nccl_result
    rc, stdout, stderr = bench1_nccl_result()
    assert rc == 0, stderr[-2000:]
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 1 and j["config"]["allgather"] is True and j["config"]["solved_fraction"] >= 0.999
    assert abs(j["value"] - 4096 * 3 / (j["ms_per_step"] * 3e-3)) <= 1e-6 * j["value"]


def test_f32_request_is_served_with_mixed(oracle_solve):
    """MPCQP_PREC_F32 (the round-1 kernels' arithmetic) is retired: the product library serves the request with MIXED, at every horizon."""
    b = mpcqp.synth.config5(256)
    ref = oracle_solve(b, N=20)
    out = gpu_solve(b, N=20, io="f32", precision="f32")
    mix = gpu_solve(b, N=20, io="f32", precision="mixed")
    assert np.array_equal(out["u"], mix["u"]) and np.array_equal(out["status"], mix["status"])
    check_batch(out, b, ref, max_iter=out["max_iter"], allowed=0, what="f32 request")


def test_retired_kernel_flags_are_accepted_and_ignored():
    """MPCQP_FLAG_GENERAL_KERNEL / MPCQP_FLAG_TILE_KERNEL selected the round-1 kernels; a caller that still sets them gets the engine's bits."""
    b = mpcqp.synth.config3(256)
    want = gpu_solve(b, io="f32", precision="mixed")
    for fl in (4, 32, 4 | 32):
        got = gpu_solve(b, io="f32", precision="mixed", flags=mpcqp.FLAG_POLISH | fl)
        assert np.array_equal(got["u"], want["u"]) and np.array_equal(got["status"], want["status"])


def test_two_handles_on_two_streams_give_the_serial_bits():
    """include/mpcqp.h, "Handles and devices": a handle serves one stream at a time, two concurrent streams need two handles.
    Two handles solving different batches concurrently (their launches overlap on the device: ordered launch form, per-handle
    queue heads and workspaces) return the bits each returns alone."""
    G, M = ("trot", "pronk", "amble", "gallop"), (0.3, 0.5, 0.7, 1.0)
    sols = [mpcqp.MPCBatch(N=10, delta=0.03, io_dtype="f32", precision="mixed") for _ in range(2)]
    devs = [s.upload(mpcqp.synth.make_batch(4096, 10, 0.03, 31 + i, G, M)) for i, s in enumerate(sols)]
    run = lambda i, st=None: sols[i].solve_batch(devs[i]["x0"], devs[i]["r"], devs[i]["contact"], devs[i]["xdes"], devs[i]["mu"], stream=st)
    alone = []
    for i in range(2):
        o = run(i)
        torch.cuda.synchronize()
        alone.append({k: o[k].clone() for k in ("u", "status", "iters")})
    streams = [torch.cuda.Stream() for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(5):
        outs = [run(i, streams[i]) for i in range(2)]
    torch.cuda.synchronize()
    for i in range(2):
        for k in ("u", "status", "iters"):
            assert torch.equal(outs[i][k], alone[i][k]), (i, k)
    assert not torch.equal(alone[0]["u"], alone[1]["u"])
