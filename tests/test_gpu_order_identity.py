"""The dispatch-order pre-pass (csrc/mpcqp_common.h: mpcqp_order_kernel, csrc/mpcqp_order.h) changes the order of a launch and
nothing else: the ordered launch against one workgroup per QP in batch order (MPCQP_FLAG_NATURAL_ORDER), bitwise, on batches
that carry what the score must survive -- NaN and inf in x0, xdes, r and mu, entries at 1e30, QPs without a stance leg.  The status
and iteration buffers are filled with a sentinel before the solve, so a QP that the pre-pass files twice (another is then never
filed) or not at all shows as a sentinel left behind.
  B = 2304, N = 10: the smallest multiple of the pre-pass's 64-QP workgroups on a 256-CU device that takes the ordered path
                    (more than 8 resident workgroups per CU), fp32 and fp64 I/O
  B = 600,  N = 20: more than 2 per CU, and a last pre-pass workgroup that is partly empty; a lane takes two stages"""
import numpy as np
import pytest
import torch

import mpcqp

pytestmark = pytest.mark.gpu

KEYS = ("u", "X", "status", "iters", "res")
SENTINEL = -7777


def poisoned(B, N, seed):
    """The bench distribution with rows made non-finite (`bad`), rows carrying 1e30 (`huge`) and rows without a stance leg."""
    b = mpcqp.synth.make_batch(B, N, 0.03, seed, ("trot", "pronk", "amble", "gallop"), (0.3, 0.5, 0.7, 1.0))
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
    rows = np.random.default_rng(seed).permutation(B)[:24]
    bad, huge, swing = rows[:12], rows[12:18], rows[18:]
    stance = lambda i, k: int(np.argmax(b["contact"][i, k])) if b["contact"][i, k].any() else 0
    b["x0"][bad[0], 9] = np.nan; b["x0"][bad[1], 10] = np.inf; b["x0"][bad[2], 4] = -np.inf
    b["xdes"][bad[3], 3, 9] = np.nan; b["xdes"][bad[4], N, 10] = np.inf; b["xdes"][bad[5], 1, 0] = np.nan
    b["r"][bad[6], 0, stance(bad[6], 0), 0] = np.nan; b["r"][bad[7], N - 1, stance(bad[7], N - 1), 2] = np.inf; b["r"][bad[8], 2, :, :] = -np.inf
    b["mu"][bad[9]] = np.nan; b["mu"][bad[10]] = np.inf; b["mu"][bad[11]] = -np.inf
    b["x0"][huge[0], 9] = 1e30; b["x0"][huge[1], 3] = -1e30; b["xdes"][huge[2], 2, 10] = 1e30
    b["r"][huge[3], 1, :, 0] = 1e30; b["r"][huge[4], 0, :, :] = 1e30; b["mu"][huge[5]] = 1e30
    b["contact"][swing] = 0
    return b, bad, huge


def solve(batch, N, io, flags):
    sol = mpcqp.MPCBatch(N=N, delta=0.03, io_dtype=io, precision="mixed", flags=flags)
    dev = sol.upload(batch)
    B = len(batch["mu"])
    pre = sol._outputs(B, True, None)                     # the buffers the solve will write: sentinel first
    pre["status"].fill_(SENTINEL); pre["iters"].fill_(SENTINEL)
    out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True)
    torch.cuda.synchronize()
    assert out["status"].data_ptr() == pre["status"].data_ptr()
    res = {k: out[k].cpu().numpy().copy() for k in KEYS}
    sol.engine.close()
    return res


def compare(B, N, io, seed):
    batch, bad, huge = poisoned(B, N, seed)
    ordered = solve(batch, N, io, mpcqp.FLAG_POLISH)
    natural = solve(batch, N, io, mpcqp.FLAG_POLISH | mpcqp.FLAG_NATURAL_ORDER)
    for name, o in (("ordered", ordered), ("natural", natural)):
        left = np.nonzero((o["status"] == SENTINEL) | (o["iters"] == SENTINEL))[0]
        assert left.size == 0, f"{name}: QPs {left[:8].tolist()} were never solved"
    for k in KEYS:
        assert ordered[k].dtype == natural[k].dtype and ordered[k].shape == natural[k].shape, k
        diff = np.nonzero((ordered[k].reshape(B, -1).view(np.uint8) != natural[k].reshape(B, -1).view(np.uint8)).any(axis=1))[0]
        assert diff.size == 0, f"{k}: rows {diff[:8].tolist()} differ between the ordered and the plain launch"
    st = ordered["status"]
    assert np.all(st[bad] == -1), st[bad]
    plain_rows = np.setdiff1d(np.arange(B), np.concatenate([bad, huge]))       # (a row at 1e30 is finite input; what the solver makes of
    assert not np.any(st[plain_rows] == -1)                                    #  it is its own business, and the same in both launches)
    assert ((st[plain_rows] == 1) | (st[plain_rows] == 2)).mean() >= 0.99


@pytest.mark.parametrize("io", ["f32", "f64"])
def test_ordered_launch_is_a_reordering_n10(io):
    compare(2304, 10, io, 20261030)


def test_ordered_launch_is_a_reordering_n20():
    compare(600, 20, "f32", 20261031)
