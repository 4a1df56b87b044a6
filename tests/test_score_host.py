"""The score row of a roll-out on the host (mpcqp.score; include/mpcqp_sim.h, mpcqp_rollout_score), no GPU: score_host on the CPU
checker's rollout_legs logs against a direct row-by-row restatement, the figures DESIGN.md's per-gait table states read off a score
row, a roll-out scored in two pieces, bad rows, the fall rule, and the binding's gate."""
import os
import re
import types

import numpy as np
import pytest

import mpcqp
from conftest import REPO
from legroll_cases import REPORT_T, checker_engine, gait_report, host_loop
from legsim_cases import DELTA, ROLL_B, ROLL_T, STEP_HEIGHT
from mpcqp import gaits, score

from score_cases import COUNTS, I, agree, direct, logs_of, vabs_of


# ------------------------------------------------------------------------------------------------------ 1. the names and the binding
def test_fields_mirror_the_header_and_the_binding_gates_the_call(oracle_lib):
    hdr = open(os.path.join(REPO, "include", "mpcqp_sim.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define MPCQP_SCORE_([A-Z_]+) (\d+)\b(?!\.)", hdr)}
    assert defs.pop("FIELDS") == len(score.FIELDS) == 33
    names = [n for n, _ in sorted(defs.items(), key=lambda kv: kv[1])]
    want = [n.upper() for n in score.FIELDS if not re.search(r"_[123]$", n)]
    assert names == [n[:-2] if n.endswith("_0") else n for n in want]
    assert defs["STANCE_ROWS"] == I["stance_rows_0"] and defs["FLIGHT_ROWS"] == I["stance_rows_3"] + 1
    assert float(re.search(r"#define MPCQP_SCORE_RULE_Z_FRAC ([0-9.]+)", hdr).group(1)) == score.Z_FRAC == 0.5
    assert float(re.search(r"#define MPCQP_SCORE_RULE_TILT_MAX ([0-9.]+)", hdr).group(1)) == score.TILT_MAX == 0.7
    assert set(score.MAX_FIELDS) | set(score.SUM_FIELDS) | {"fall_row"} == set(score.FIELDS)
    assert sum(len(g) for g in score.GROUPS.values()) == 33
    capi = mpcqp._capi
    assert capi.ctypes.sizeof(capi.MpcQpScoreRule) == 24 and capi.MpcQpScoreRule.z_frac.offset == 8
    assert capi.SCORE_SYMBOLS == ("mpcqp_rollout_score",) and set(capi.SCORE_SYMBOLS) <= set(capi.SIM_SYMBOLS)
    plib = mpcqp.product_library()
    assert plib.has_sim and plib.has_legroll and plib.has_score and plib.version() == 0x00010301
    # the checker library has none of the header: the raw call and MPCBatch.score name it
    assert not oracle_lib.has_score and not oracle_lib.has_sim
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    gate = rf"mpcqp_rollout_score: {re.escape(oracle_lib.path)} does not export include/mpcqp_sim.h \(product library only\)"
    with pytest.raises(mpcqp.MpcQpError, match=gate):
        eng.rollout_score_ptr(1, 1, *([0] * 8), 0, 0)
    import torch
    sol = object.__new__(mpcqp.MPCBatch)                                         # (an MPCBatch on the checker: host tensors, no stream)
    sol.engine, sol.device, sol.tdtype = eng, torch.device("cpu"), torch.float64
    logs = {k: torch.as_tensor(v) for k, v in logs_of(host_loop("rule")[2]).items()}
    with pytest.raises(mpcqp.MpcQpError, match=gate):
        sol.score(logs, score=torch.zeros((ROLL_B, 33), dtype=torch.float64), stream=types.SimpleNamespace(cuda_stream=0))
    with pytest.raises(ValueError, match="operand mismatch: contact_log expected"):
        sol.score({k: v for k, v in logs.items() if k != "contact_log"})
    with pytest.raises(ValueError, match="all three or none"):
        sol.score({k: v for k, v in logs.items() if k != "qd"})


# ------------------------------------------------------------------------------------------- 2. every field, on the checker's roll-outs
@pytest.mark.parametrize("land", ["rule", "actual"])
def test_every_field_against_the_direct_restatement(land):
    logs = logs_of(host_loop(land)[2])
    s, d = score.score_host(logs), direct(logs)
    assert s.shape == (ROLL_B, 33) and s.dtype == np.float64 and np.isfinite(s).all()
    agree(s, d, ROLL_T, vabs_of(logs))
    assert np.all(s[:, I["rows"]] == ROLL_T) and not s[:, I["bad_rows"]].any() and not s[:, I["poisoned_rows"]].any()
    # the case exercises the fields: stepping robots swing and land, the stand does not; nothing is trivially zero
    assert (s[:, I["landings"]] > 0).sum() >= 14 and (s[:, I["swing_rows"]] > 0).sum() >= 14 and (s[:, I["flight_rows"]] > 0).any()
    for n in ("z_sq", "vel_sq", "ang_sq", "f_sq", "fz_max", "fric_max", "tilt_max"):
        assert np.all(s[:, I[n]] > 0), n
    for n in ("tau_sq", "work_pos", "work_abs", "miss_sq", "miss_max", "tau_max"):
        assert (s[:, I[n]] > 0).sum() >= 14, n
    # without the optional groups the other fields keep their bits and the group's fields are zero
    for drop, group in ((("tau", "qd", "flag"), "legs"), (("miss",), "miss")):
        r = score.score_host({k: v for k, v in logs.items() if k not in drop})
        for n in score.FIELDS:
            assert np.array_equal(r[:, I[n]], np.zeros(ROLL_B) if n in score.GROUPS[group] else s[:, I[n]]), n


# --------------------------------------------------------------------------------------------- 3. the figures DESIGN.md's table states
def test_summarize_reproduces_the_trot_row_of_the_design_table():
    names = tuple(gaits.GAITS)
    pb = gaits.make_phase_batch(len(names), names, 12, seed=6)                  # legroll_cases.gait_report's batch
    B = len(names)
    lib, eng = checker_engine()
    o = gaits.rollout_legs_host(eng, pb["x"], pb["ref"], pb["feet"], np.zeros((B, 4, 7)), pb["gait"], pb["stand"], pb["gain"], pb["tick"],
                                pb["mu"], REPORT_T, np.full(B, STEP_HEIGHT), "rule")
    s = score.score_host(logs_of(o))
    fig = score.summarize(s, DELTA, mass=eng.cfg.m)
    t = names.index("trot")
    print({k: np.round(np.asarray(v[t], dtype=np.float64), 6).tolist() for k, v in fig.items()})
    # DESIGN.md, "Swing legs inside the phase roll-out": trot | 6.38, 1.642 | ... | 12.36 (land = rule), to the table's digits
    assert f"{fig['z_max'][t] * 1e3:.2f}" == "6.38" and f"{fig['z_rms'][t] * 1e3:.3f}" == "1.642" and f"{fig['miss_max'][t] * 1e3:.2f}" == "12.36"
    rep = gait_report()["rule"]
    for b, n in enumerate(names):                                               # ... and the report's own numbers for every gait
        assert abs(fig["z_max"][b] - rep[n][1]) <= 1e-12 and abs(fig["z_rms"][b] - rep[n][2]) <= 1e-12, n
        assert abs(fig["miss_max"][b] - rep[n][3]) <= 1e-12 and s[b, I["clamp_rows"]] == rep[n][4], n
    assert not fig["fell"][names.index("trot")] and np.isnan(fig["fall_time"][t]) and fig["rows"][t] == REPORT_T
    # what summarize derives, against the logs
    v = o["actual"][:, :, 9:11].sum(axis=1)
    dist = np.hypot(v[:, 0], v[:, 1]) * DELTA
    assert np.allclose(fig["distance"], dist, rtol=1e-13, atol=0) and np.allclose(fig["v_mean"], dist / DELTA / REPORT_T, rtol=1e-13, atol=0)
    assert np.allclose(fig["duty"], (o["contact_log"] != 0).mean(axis=1), rtol=1e-13, atol=0)
    work = np.maximum((o["tau"] * o["qd"]).sum(-1), 0.0).sum(axis=(1, 2)) * DELTA
    assert np.allclose(fig["work_pos"], work, rtol=1e-12, atol=0)
    assert np.allclose(fig["cot"][dist > 0], (work / (eng.cfg.m * 9.81 * dist))[dist > 0], rtol=1e-12, atol=0) and fig["cot"][t] > 0
    assert np.isnan(score.summarize(s, DELTA)["cot"]).all()
    swing = s[:, I["swing_rows"]]
    assert np.array_equal(fig["clamp_share"], np.where(swing > 0, s[:, I["clamp_rows"]] / np.maximum(swing, 1), 0.0))
    assert fig["miss_rms"][names.index("stand")] == 0.0 and fig["landings"][names.index("stand")] == 0
    import torch
    ft = score.summarize(torch.as_tensor(s), DELTA, mass=eng.cfg.m)             # the same figures from a tensor
    for k, v in fig.items():
        assert np.array_equal(ft[k].numpy(), v, equal_nan=True), k


# ------------------------------------------------------------------------------------------------------------------- 4. two pieces
def test_two_pieces_against_one_call():
    o = host_loop("actual")[2]
    whole = score.score_host(logs_of(o))
    first = score.score_host(logs_of(o, slice(0, 12)))
    both = score.score_host(logs_of(o, slice(12, ROLL_T)), score=first)
    assert both is first                                                        # combined in place
    agree(both, whole, ROLL_T, vabs_of(logs_of(o)))
    for n in score.MAX_FIELDS:
        assert np.array_equal(both[:, I[n]], whole[:, I[n]]), n
    # ... and through scored_rollout, whose closure hands out the pieces in order
    at = [0]

    def step(n):
        at[0] += n
        return logs_of(o, slice(at[0] - n, at[0]))

    chained = score.scored_rollout(step, ROLL_T, 12)
    assert at[0] == ROLL_T and np.array_equal(chained, score.score_host(logs_of(o, slice(24, 25)), score=both_of(o)))
    assert np.array_equal(score.scored_rollout(lambda n: logs_of(o, slice(0, n)), 0, 12), score.identity(ROLL_B))
    with pytest.raises(ValueError, match="piece must be >= 1"):
        score.scored_rollout(step, ROLL_T, 0)


def both_of(o):
    return score.score_host(logs_of(o, slice(12, 24)), score=score.score_host(logs_of(o, slice(0, 12))))


# --------------------------------------------------------------------------------------------------------------------- 5. bad rows
def test_a_bad_row_counts_and_contributes_nothing():
    o = host_loop("actual")[2]
    clean = score.score_host(logs_of(o))
    r = 5
    bad = logs_of(o)
    bad["actual"][r, 7, 2] = np.nan
    s = score.score_host(bad)
    assert np.isfinite(s).all() and s[r, I["bad_rows"]] == 1 and s[r, I["rows"]] == ROLL_T - 1 and s[r, I["fall_row"]] == 7
    others = np.arange(ROLL_B) != r
    assert np.array_equal(s[others], clean[others])
    without = {k: np.delete(v[r:r + 1], 7, axis=1) for k, v in logs_of(o).items()}   # the clean run minus that row
    w = score.score_host(without)
    w[0, I["bad_rows"]], w[0, I["fall_row"]] = 1, 7
    agree(s[r:r + 1], w, ROLL_T, vabs_of(without))                             # (sums to the summation bound: the order of 24 and of 25 terms)
    for n in score.MAX_FIELDS + COUNTS:
        assert s[r, I[n]] == w[0, I[n]], n
    # a NaN force or reference row is a bad row too; a later piece keeps the first fall
    for key in ("desired", "forces"):
        b2 = logs_of(o)
        b2[key][r, 3, 11] = np.inf
        s2 = score.score_host(b2)
        assert s2[r, I["bad_rows"]] == 1 and s2[r, I["fall_row"]] == 3 and np.isfinite(s2).all()
    p = score.score_host({k: v[:, 12:] for k, v in bad.items()}, score=score.score_host({k: v[:, :12] for k, v in bad.items()}))
    assert p[r, I["fall_row"]] == 7 and p[r, I["bad_rows"]] == 1
    late = logs_of(o)
    late["actual"][r, 20, 0] = np.nan
    p = score.score_host({k: v[:, 12:] for k, v in late.items()}, score=score.score_host({k: v[:, :12] for k, v in late.items()}))
    assert p[r, I["fall_row"]] == 20                                            # the global index: 12 rows carried in, row 8 of the piece
    # a poisoned leg-row and a NaN miss stay out of the sums
    q = logs_of(o)
    q["flag"][r, 4, 1], q["tau"][r, 4, 1], q["miss"][r, 6, 2] = 0xff, np.nan, np.nan
    sq = score.score_host(q)
    assert np.isfinite(sq).all() and sq[r, I["poisoned_rows"]] == 1
    assert sq[r, I["landings"]] == clean[r, I["landings"]] + (o["miss"][r, 6, 2] == 0)
    agree(sq, direct(q), ROLL_T, vabs_of(q))


# ----------------------------------------------------------------------------------------------------------------- 6. the fall rule
def test_fall_rule_rows():
    logs = logs_of(host_loop("rule")[2])
    assert np.all(score.score_host(logs)[:, I["fall_row"]] == -1)               # nobody falls in the checker's roll-out
    t = np.arange(ROLL_T)
    logs["actual"][0, :, 5] = logs["desired"][0, :, 5] * (1.0 - 0.04 * t)       # robot 0 sinks: below 0.5 at row 13, below 0.7 at row 8
    logs["actual"][1, :, 0], logs["actual"][1, :, 1] = 0.06 * t, 0.0            # robot 1 tilts: past 0.7 rad at row 12, past 0.4 at row 7
    ratio = logs["actual"][..., 5] / logs["desired"][..., 5]
    tilt = np.hypot(logs["actual"][..., 0], logs["actual"][..., 1])
    for z_frac, tilt_max, rows in ((0.5, 0.7, (13, 12)), (0.7, 0.4, (8, 7)), (0.5, 0.4, (13, 7)), (0.9, 10.0, (3, -1))):
        # no row of any robot within 1e-9 of a threshold: the row is the rule's, not the rounding's
        assert np.abs(logs["actual"][..., 5] - z_frac * logs["desired"][..., 5]).min() > 1e-9 and np.abs(tilt - tilt_max).min() > 1e-9
        s = score.score_host(logs, rule=(z_frac, tilt_max))
        down = (ratio < z_frac) | (tilt > tilt_max)
        want = np.where(down.any(axis=1), down.argmax(axis=1), -1)
        assert np.array_equal(s[:, I["fall_row"]], want) and tuple(want[:2]) == rows
        assert np.all(want[2:] == -1) or z_frac > 0.5                            # (a stricter height rule also catches a gait that sags)
        assert np.array_equal(s, score.score_host(logs, rule={"z_frac": z_frac, "tilt_max": tilt_max}))
        fig = score.summarize(s, DELTA)
        assert np.array_equal(fig["fell"], want >= 0) and fig["fall_time"][0] == rows[0] * DELTA
    assert np.array_equal(score.score_host(logs), score.score_host(logs, rule=(0.5, 0.7)))
    # a fallen row is scored like any other
    assert score.score_host(logs)[0, I["rows"]] == ROLL_T and score.score_host(logs)[0, I["z_max"]] == np.abs(logs["actual"][0, :, 5] - logs["desired"][0, :, 5]).max()
    for rule in ((0.0, 0.7), (0.5, -1.0), (np.nan, 0.7), (0.5, np.inf)):
        with pytest.raises(ValueError, match="finite and positive"):
            score.score_host(logs, rule=rule)
