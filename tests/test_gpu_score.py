"""The score row of a roll-out on the device (include/mpcqp_sim.h, mpcqp_rollout_score; csrc/mpcqp_score.h) against score.score_host on
the same tensors.  The inputs are synthetic logs (score_cases.synthetic_logs): the reduction can go wrong at the edges of its tick
stride (64 lanes per robot) and of its block (four robots), not at scale -- B = 33 with T = 1, 25, 64, 65, 130 -- plus one real case,
the 16-robot, 25-tick rollout_legs batch of tests/legroll_cases.py.

Bounds (derived, u = 2^-52; the observed worst is printed and quoted in DESIGN.md): counts, fall_row and bad_rows equal; maxima within
8 u relative (a few fp64 operations, sqrt and the division correctly rounded); non-negative sums within (T + 8) u relative (the
summation bound (T - 1) u in any order plus the per-term error); vx_sum, vy_sum within the same factor times sum |v|."""
import ctypes
import re

import numpy as np
import pytest

import mpcqp
from legsim_cases import DELTA, ROLL_B, ROLL_T
from mpcqp import score
from score_cases import I, agree, rule_margin, synthetic_logs, vabs_of

pytestmark = pytest.mark.gpu
B0, TICKS, NF = 33, (1, 25, 64, 65, 130), len(score.FIELDS)
NP_DT = {"f32": np.float32, "f64": np.float64}
_SOL = {}


def _sol(io):
    if io not in _SOL:
        _SOL[io] = mpcqp.MPCBatch(N=10, delta=DELTA, io_dtype=io, precision="mixed")
    return _SOL[io]


def _dev(logs):
    import torch
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in logs.items()}


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _cut(logs, rows=slice(None), robots=slice(None)):
    return {k: v[robots, rows].contiguous() if hasattr(v, "contiguous") else np.ascontiguousarray(v[robots, rows]) for k, v in logs.items()}


def _raw(sol, B, T, d, accumulate, score_t, rule=None, **swap):
    """The raw call with the operands of the device logs `d`, any of them replaced (0 = NULL)."""
    p = {k: (d[k].data_ptr() if d.get(k) is not None else 0) for k in ("actual", "desired", "forces", "contact_log", "tau", "qd", "flag", "miss")}
    p.update(swap)
    sol.engine.rollout_score_ptr(B, T, p["actual"], p["desired"], p["forces"], p["contact_log"], p["tau"], p["qd"], p["flag"], p["miss"],
                                 accumulate, score_t if isinstance(score_t, int) else score_t.data_ptr(), rule, 0)


# ------------------------------------------------------------------------------------------------------ 1. against the host, every edge
@pytest.mark.parametrize("io", ["f32", "f64"])
@pytest.mark.parametrize("T", TICKS)
def test_against_score_host(io, T):
    import torch
    sol = _sol(io)
    logs = synthetic_logs(B0, T, seed=100 + T, dtype=NP_DT[io])
    assert rule_margin(logs) > 1e-9                                             # no row within 1e-9 of the rule's thresholds
    d = _dev(logs)
    s = sol.score(d)
    assert s.shape == (B0, NF) and s.dtype == torch.float64 and s.is_cuda
    again = sol.score(d)
    host = score.score_host(logs)
    dev = _np(s)
    assert torch.equal(s, again)                                                # the same call twice
    assert np.isfinite(dev).all()
    agree(dev, host, T, vabs_of(logs))
    if T >= 25:                                                                 # the inputs reach every branch
        for n in ("bad_rows", "poisoned_rows", "flight_rows", "landings", "clamp_rows", "singular_rows", "miss_max", "fric_max"):
            assert host[:, I[n]].max() > 0, n
        assert (host[:, I["fall_row"]] >= 0).any() and (host[:, I["fall_row"]] > 0).any()


def test_float32_logs_convert_exactly():
    import torch
    logs = synthetic_logs(B0, 65, seed=7, dtype=np.float32)
    wide = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in logs.items()}
    assert torch.equal(_sol("f32").score(_dev(logs)), _sol("f64").score(_dev(wide)))


# ---------------------------------------------------------------------------------------------------------------------- 2. geometry
@pytest.mark.parametrize("T", TICKS)
def test_a_robots_row_does_not_depend_on_the_batch(T):
    import torch
    sol = _sol("f32")
    one = synthetic_logs(1, T, seed=5, dtype=np.float32)
    rows = [sol.score(_dev(one))[0]]
    for B, slot in ((33, 32), (130, 40)):
        logs = synthetic_logs(B, T, seed=B, dtype=np.float32)
        for k in logs:
            logs[k][slot] = one[k][0]
        rows.append(sol.score(_dev(logs))[slot])
    assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])


# --------------------------------------------------------------------------------------------------------------------- 3. accumulate
@pytest.mark.parametrize("io", ["f32", "f64"])
def test_two_pieces_against_one_call(io):
    import torch
    sol, T = _sol(io), 130
    logs = synthetic_logs(B0, T, seed=11, dtype=NP_DT[io])
    d = _dev(logs)
    whole = sol.score(d)
    for cut in (12, 64, 129):
        first = sol.score(_cut(d, slice(0, cut)))
        both = sol.score(_cut(d, slice(cut, T)), score=first)
        assert both.data_ptr() == first.data_ptr()                              # combined in place
        a, w = _np(both), _np(whole)
        agree(a, w, T, vabs_of(logs))
        for n in score.MAX_FIELDS:
            assert np.array_equal(a[:, I[n]], w[:, I[n]]), n
        hp = score.score_host(_cut(logs, slice(cut, T)), score=score.score_host(_cut(logs, slice(0, cut))))
        agree(a, hp, T, vabs_of(logs))
    # a fresh call ignores what the buffer held
    junk = torch.full((B0, NF), float("nan"), dtype=torch.float64, device="cuda")
    _raw(sol, B0, T, d, 0, junk)
    assert torch.equal(junk, whole)


# ----------------------------------------------------------------------------------------------------------------- 4. optional groups
def test_every_optional_group_null():
    import torch
    sol = _sol("f32")
    logs = synthetic_logs(B0, 65, seed=3, dtype=np.float32)
    d = _dev(logs)
    full = sol.score(d)
    groups = {"legs": ("tau", "qd", "flag"), "miss": ("miss",)}
    for absent in (("legs",), ("miss",), ("legs", "miss")):
        drop = sum((groups[g] for g in absent), ())
        s = sol.score({k: v for k, v in d.items() if k not in drop})
        for n in score.FIELDS:
            zero = any(n in score.GROUPS[g] for g in absent)
            assert torch.equal(s[:, I[n]], torch.zeros_like(s[:, I[n]]) if zero else full[:, I[n]]), (absent, n)
        agree(_np(s), score.score_host({k: v for k, v in logs.items() if k not in drop}), 65, vabs_of(logs))


# ------------------------------------------------------------------------------------------------------------- 5. checks and no-ops
def test_argument_checks_by_message():
    import torch
    sol = _sol("f32")
    d = _dev(synthetic_logs(4, 8, seed=1, dtype=np.float32))
    out = torch.zeros((4, NF), dtype=torch.float64, device="cuda")
    err = lambda msg: pytest.raises(mpcqp.MpcQpError, match=r"mpcqp_rollout_score failed with code -1: mpcqp_rollout_score: " + msg)
    for B, T in ((-1, 8), (4, -1), (2 ** 20, 2 ** 11), (2 ** 31, 1)):
        with err("size out of range"):
            _raw(sol, B, T, d, 0, out)
    for k in ("actual", "desired", "forces", "contact_log"):
        with err("null buffer"):
            _raw(sol, 4, 8, d, 0, out, **{k: 0})
    with err("null buffer"):
        _raw(sol, 4, 8, d, 0, 0)
    for k in ("tau", "qd", "flag"):
        with err("the leg group is tau, qd and flag: all three or none"):
            _raw(sol, 4, 8, d, 0, out, **{k: 0})
        with err("the leg group is tau, qd and flag: all three or none"):
            _raw(sol, 4, 8, d, 0, out, **{j: 0 for j in ("tau", "qd", "flag") if j != k})
    for z_frac, tilt_max in ((0.0, 0.7), (-0.5, 0.7), (0.5, 0.0), (float("nan"), 0.7), (0.5, float("inf"))):
        with err("z_frac and tilt_max must be finite and positive"):
            _raw(sol, 4, 8, d, 0, out, rule=score.rule_struct((z_frac, tilt_max)))
        with pytest.raises(mpcqp.MpcQpError, match="finite and positive"):
            sol.score(d, rule=(z_frac, tilt_max))
    short = score.rule_struct((0.5, 0.7))
    short.size = 16
    with err("rule struct size mismatch"):
        _raw(sol, 4, 8, d, 0, out, rule=short)
    with err("a log buffer is not 16-byte aligned"):                             # (the rows are read as vectors)
        _raw(sol, 4, 7, d, 0, out, actual=d["actual"].data_ptr() + 4)
    with err("contact_log / flag not 4-byte or score not 8-byte aligned"):
        _raw(sol, 4, 7, d, 0, out, flag=d["flag"].data_ptr() + 1)
    torch.cuda.synchronize()
    assert not out.any()                                                        # a refused call writes nothing
    # the Python layer's own checks
    with pytest.raises(ValueError, match="operand mismatch: score expected"):
        sol.score(d, score=torch.zeros((4, NF), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="operand mismatch: forces expected"):
        sol.score(dict(d, forces=d["forces"].double()))
    with pytest.raises(ValueError, match="all three or none"):
        sol.score({k: v for k, v in d.items() if k != "flag"})
    with pytest.raises(ValueError, match="unknown key"):
        sol.score(d, rule={"zfrac": 0.5})


def test_empty_batch_and_no_ticks():
    import torch
    sol = _sol("f32")
    ident = torch.as_tensor(score.identity(5)).cuda()
    for accumulate in (0, 1):
        _raw(sol, 0, 8, {}, accumulate, 0)                                      # B = 0: a no-op, no buffer needed
    junk = torch.full((5, NF), float("nan"), dtype=torch.float64, device="cuda")
    _raw(sol, 5, 0, {}, 0, junk)                                                # T = 0, fresh: the identity row, no log needed
    assert torch.equal(junk, ident)
    kept = torch.arange(5 * NF, dtype=torch.float64, device="cuda").reshape(5, NF)
    before = kept.clone()
    _raw(sol, 5, 0, {}, 1, kept)                                                # T = 0, accumulate: the score is left alone
    torch.cuda.synchronize()
    assert torch.equal(kept, before)
    d = _dev(synthetic_logs(5, 0, seed=2, dtype=np.float32))                    # ... and through MPCBatch.score
    assert torch.equal(sol.score(d), ident) and torch.equal(sol.score(d, score=kept), before)
    assert sol.score(_dev(synthetic_logs(0, 4, seed=2, dtype=np.float32))).shape == (0, NF)


def test_a_rule_of_ones_own():
    import torch
    sol = _sol("f64")
    logs = synthetic_logs(B0, 65, seed=21, dtype=np.float64, bad=False)
    d = _dev(logs)
    default = _np(sol.score(d))
    for rule in ((0.95, 0.12), {"z_frac": 0.2}, {"tilt_max": 1.5}):
        z_frac, tilt_max = score.rule_pair(rule)
        assert rule_margin(logs, z_frac, tilt_max) > 1e-9
        s, h = _np(sol.score(d, rule=rule)), score.score_host(logs, rule=rule)
        agree(s, h, 65, vabs_of(logs))
        assert not np.array_equal(s[:, I["fall_row"]], default[:, I["fall_row"]])   # the rule moved somebody's row ...
        others = [i for i in range(NF) if i != I["fall_row"]]
        assert np.array_equal(s[:, others], default[:, others])                  # ... and nothing else
    assert np.array_equal(_np(sol.score(d, rule=(score.Z_FRAC, score.TILT_MAX))), default)


# -------------------------------------------------------------------------------------------------------------------- 6. a real case
@pytest.mark.parametrize("io", ["f32", "f64"])
def test_the_rollout_legs_batch_and_its_pieces(io):
    import torch
    from test_gpu_rollout_legs import _Ops, _case
    sol = _sol(io)
    pb, rows = _case(io)
    ops = _Ops(sol, pb, rows)
    st = ops.state()
    logs = ops.legs(st, ROLL_T, "actual")
    s = sol.score(logs)
    host_logs = {k: _np(v) for k, v in logs.items()}
    h = score.score_host(host_logs)
    dev = _np(s)
    agree(dev, h, ROLL_T, vabs_of(host_logs))
    assert np.all(dev[:, I["rows"]] == ROLL_T) and np.all(dev[:, I["fall_row"]] == -1) and not dev[:, I["poisoned_rows"]].any()
    assert (dev[:, I["landings"]] > 0).sum() >= 14 and (dev[:, I["work_abs"]] > 0).sum() >= 14
    fig, fh = score.summarize(s, DELTA, mass=sol.cfg.m), score.summarize(h, DELTA, mass=sol.cfg.m)
    for k in ("z_rms", "distance", "duty", "cot", "miss_rms"):
        assert fig[k].is_cuda and np.allclose(_np(fig[k]), fh[k], rtol=1e-12, atol=0, equal_nan=True), k
    # the same roll-out in pieces of 12 (12 + 12 + 1), scored into one carried row: the state chains bit for bit, the score within the bounds
    st2 = ops.state()
    pieces = score.scored_rollout(lambda n: ops.legs(st2, n, "actual"), ROLL_T, 12, scorer=sol.score)
    torch.cuda.synchronize()
    for k in ("x", "feet", "legs", "tick"):
        assert torch.equal(st2[k], st[k]), k
    agree(_np(pieces), dev, ROLL_T, vabs_of(host_logs))
    for n in score.MAX_FIELDS:
        assert np.array_equal(_np(pieces)[:, I[n]], dev[:, I[n]]), n
    with pytest.raises(ValueError, match="device logs need scorer=MPCBatch.score"):
        score.scored_rollout(lambda n: logs, ROLL_T, 12)


def test_the_product_library_has_the_call():
    plib = mpcqp.product_library()
    assert plib.has_sim and plib.has_score and plib.calls["mpcqp_rollout_score"][0] is not None
    assert ctypes.sizeof(mpcqp._capi.MpcQpScoreRule) == 24 and re.fullmatch(r"mpcqp_[a-z_]+", mpcqp._capi.SCORE_SYMBOLS[0])
