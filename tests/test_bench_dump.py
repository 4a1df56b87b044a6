"""bench.py --dump-outputs without a GPU: what dump_outputs writes, and the fixed sample it keeps above its size limit."""
import os

import numpy as np
import torch

import bench

KINDS = {"u": np.float32, "res": np.float32, "status": np.float64, "iters": np.float64}


def _out(B, N=10):
    """A solve_batch result of B QPs (want_X=False), on the host."""
    g = torch.Generator().manual_seed(0)
    return {"u": torch.randn((B, N, 12), generator=g), "X": None, "status": torch.randint(0, 4, (B,), dtype=torch.int32, generator=g),
            "iters": torch.randint(0, 5000, (B,), dtype=torch.int32, generator=g), "res": torch.rand((B, 2), generator=g)}


def test_dump_writes_every_result_as_float(tmp_path):
    out = _out(64)
    bench.dump_outputs(out, str(tmp_path / "d"))
    assert sorted(os.listdir(tmp_path / "d")) == ["iters.npy", "res.npy", "status.npy", "u.npy"]
    for k, dt in KINDS.items():
        a = np.load(tmp_path / "d" / (k + ".npy"))
        assert a.dtype == dt and np.array_equal(a, out[k].numpy()), k


def test_dump_above_the_limit_keeps_one_fixed_sample(tmp_path):
    out = _out(1000)
    limit = 100 * (4 * 120 + 3 * 8 + 8)          # u + res + status + iters + the row index of 100 QPs
    for d in ("a", "b"):
        bench.dump_outputs(out, str(tmp_path / d), limit=limit)
    a, b = ({k: np.load(tmp_path / d / (k + ".npy")) for k in list(KINDS) + ["rows"]} for d in ("a", "b"))
    assert sum(v.nbytes for v in a.values()) <= limit
    rows = a["rows"].astype(np.int64)
    assert a["rows"].dtype == np.float64 and len(rows) == 100 and np.all(np.diff(rows) > 0) and rows.max() < 1000
    for k, dt in KINDS.items():
        assert a[k].dtype == dt and np.array_equal(a[k], out[k].numpy()[rows]) and np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["rows"], b["rows"])
