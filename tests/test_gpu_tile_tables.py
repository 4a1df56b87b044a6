"""The lane-order K^-1 table of the wrench engine (csrc/mpcqp_kernels.hip: lane_order_kinv, csrc/mpcqp_wrench.h: w_tile_init):
a handle's tables are built and freed correctly (two handles in one process give the same bits), both launch forms read them
alike, and -- without a GPU -- the index rule "lane t, tile row r -> (v0, v1, c0)" reproduces the dense padded K^-1."""
import numpy as np
import pytest

import mpcqp
from mpcqp import _capi

KEYS = ("u", "X", "status", "iters", "res")


def _solve_once(batch, N, io, precision, **kw):
    import torch
    sol = mpcqp.MPCBatch(N=N, delta=0.03, io_dtype=io, precision=precision, **kw)
    dev = sol.upload(batch)
    out = sol.solve_batch(dev["x0"], dev["r"], dev["contact"], dev["xdes"], dev["mu"], want_X=True)
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy().copy() for k in KEYS}
    sol.engine.close()   # mpcqp_destroy: the tables are freed before the next handle builds its own
    return res


def _same_bits(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs in {int((a[k] != b[k]).sum())} entries"


@pytest.mark.gpu
@pytest.mark.parametrize("N,precision", [(10, "mixed"), (10, "f64"), (20, "mixed"), (20, "f64")])
def test_second_handle_same_bits(N, precision):
    """create -> solve -> destroy, twice in one process: the second handle's outputs are bitwise those of the first."""
    batch = mpcqp.synth.config3(512) if N == 10 else mpcqp.synth.config5(512)
    first = _solve_once(batch, N, "f32", precision)
    second = _solve_once(batch, N, "f32", precision)
    assert np.all(np.isfinite(first["u"])) and ((first["status"] == 1) | (first["status"] == 2)).mean() >= 0.99
    _same_bits(first, second, f"N={N} {precision}")


@pytest.mark.gpu
@pytest.mark.parametrize("precision,io", [("mixed", "f32"), ("f64", "f64")])
def test_launch_forms_same_bits(precision, io):
    """2 500 QPs oversubscribe the resident workgroups, so the default handle takes the ordered launch form; with
    MPCQP_FLAG_NATURAL_ORDER the same batch runs in the plain form.  Every QP's result is bitwise the same."""
    batch = mpcqp.synth.config3(2500)
    ordered = _solve_once(batch, 10, io, precision)
    natural = _solve_once(batch, 10, io, precision, flags=_capi.FLAG_POLISH | _capi.FLAG_NATURAL_ORDER)
    _same_bits(ordered, natural, f"{precision}/{io}")


# ------------------------------------------------------------------------------------------------ the index rule, on the CPU
def _dense_padded(Ki, N, G):
    """K^-1 = (+)_q K_q^-1 in stage-major order (index 6 j + q), padded with an identity block to 8 G rows."""
    NQ, DP = 6 * N, 8 * G
    S0 = np.zeros((DP, DP))
    for q in range(6):
        S0[q:NQ:6, q:NQ:6] = Ki[q]
    S0[NQ:, NQ:] = np.eye(DP - NQ)
    return S0


def _lane_table(Ki, N, G):
    """The restatement of lane_order_kinv: per lane v0[8] | v1[8] and the tile column c0[8] of v0 (v1 goes to c0 + 6)."""
    NQ = 6 * N
    tab, c0s = np.zeros((G * G, 16)), np.zeros((G * G, 8), dtype=int)

    def entry(R, C):
        if R >= NQ or C >= NQ:
            return 1.0 if R == C else 0.0
        return Ki[R % 6][R // 6][C // 6] if R % 6 == C % 6 else 0.0

    for t in range(G * G):
        gr, gc = divmod(t, G)
        k = (gr - gc) % 3
        for r in range(8):
            c0 = (r + 2 * k) % 6
            c0s[t, r] = c0
            tab[t, r] = entry(8 * gr + r, 8 * gc + c0)
            tab[t, 8 + r] = entry(8 * gr + r, 8 * gc + c0 + 6) if c0 < 2 else 0.0
    return tab, c0s


@pytest.mark.parametrize("N,G", [(10, 8), (20, 16)])
def test_lane_layout_rule(N, G):
    rng = np.random.default_rng(7)
    Ki = rng.uniform(0.5, 2.0, (6, N, N)) * rng.choice([-1.0, 1.0], (6, N, N))   # no zero entry: every structural zero is visible
    S0 = _dense_padded(Ki, N, G)
    tab, c0s = _lane_table(Ki, N, G)
    placed = np.zeros_like(S0)
    for t in range(G * G):
        gr, gc = divmod(t, G)
        tile = np.zeros((8, 8))
        for r in range(8):
            c0 = c0s[t, r]
            # the column of a row depends on the lane only through its class (gr - gc) mod 3, as the old rule (R - 8 gc) mod 6 does
            assert c0 == (8 * gr + r - 8 * gc) % 6
            tile[r, c0] = tab[t, r]
            if c0 + 6 < 8:
                tile[r, c0 + 6] = tab[t, 8 + r]
            else:
                assert tab[t, 8 + r] == 0.0
        assert np.all(tile[(np.arange(8)[None, :] - np.arange(8)[:, None]) % 2 == 1] == 0.0)   # c - r odd => 0, for every lane
        placed[8 * gr:8 * gr + 8, 8 * gc:8 * gc + 8] = tile
    assert np.array_equal(placed, S0)
    assert np.array_equal(placed[6 * N:, 6 * N:], np.eye(8 * G - 6 * N))   # identity padding, exact
    # the runs of E that w_tile_init reads: every quad it addresses lies inside E, every E entry is added exactly once
    seen = np.zeros(36 * N, dtype=int)
    for t in range(G * G):
        gr, gc = divmod(t, G)
        for r in range(8):
            R = 8 * gr + r
            h = 3 * (R // 6) - 4 * gc if R < 6 * N else 64
            for hq in range(2):
                ins = [0 <= 2 * hq + i - h < 3 for i in range(2)]
                if not any(ins):
                    continue
                addr = 6 * R - 2 * h + 4 * hq
                assert 0 <= addr and addr + 4 <= 36 * N and addr % 2 == 0
                for i in range(4):
                    if ins[i // 2]:
                        C = 8 * gc + 4 * hq + i
                        assert addr + i == 6 * R + C - 6 * (R // 6) and 0 <= C - 6 * (R // 6) < 6
                        seen[addr + i] += 1
    assert np.all(seen == 1)
