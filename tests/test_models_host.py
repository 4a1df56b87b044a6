"""Per-robot model rows (include/mpcqp_model.h) without a GPU: the header and its symbols, the row helpers and the host checkers of
mpcqp.models on the CPU checker library."""
import os
import re

import numpy as np
import pytest

import mpcqp
from conftest import REPO
from mpcqp import models as M

G = 9.81


def test_model_header_declares_model_symbols_product_only(oracle_lib):
    """include/mpcqp_model.h declares exactly MODEL_SYMBOLS; the product library exports them, mpcqp.h and its version are unchanged
    and the CPU checker does not have them (its binding refuses the calls)."""
    hdr = open(os.path.join(REPO, "include", "mpcqp_model.h")).read()
    syms = set(re.findall(r"^\s*int\s+(mpcqp_[a-z_]+)\s*\(", hdr, re.M))
    assert syms == set(mpcqp._capi.MODEL_SYMBOLS) and '#include "mpcqp.h"' in hdr
    lib = mpcqp.product_library()
    assert lib.has_model and all(hasattr(lib.lib, s) for s in syms) and lib.version() == 0x00010301
    base = open(os.path.join(REPO, "include", "mpcqp.h")).read()
    assert not any(s in base for s in syms)
    assert int(re.search(r"#define MPCQP_VERSION (0x[0-9a-fA-F]+)", base).group(1), 16) == 0x00010301
    assert not oracle_lib.has_model and not any(hasattr(oracle_lib.lib, s) for s in syms)
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    with pytest.raises(mpcqp.MpcQpError, match="product library only"):
        eng.set_models_ptr(1, 1)
    with pytest.raises(mpcqp.MpcQpError, match="product library only"):
        eng.clear_models()


def test_checker_with_the_configuration_row_is_the_plain_checker(oracle_lib):
    kw = dict(N=10, delta=0.03, max_iter=4000)
    b = mpcqp.synth.config3(B=12)
    cfg = oracle_lib.default_config(**kw)
    plain = mpcqp.Engine(oracle_lib, cfg).solve_batch_host(b["x0"], b["r"], b["contact"], b["xdes"], b["mu"])
    rows = M.model_rows(cfg, 12)
    assert rows.shape == (12, 6) and np.all(rows[:, 0] == cfg.m) and np.all(rows[:, 4] == cfg.f_min) and np.all(rows[:, 5] == cfg.f_max)
    got = M.solve_batch_models_host(oracle_lib, kw, rows, b)
    for k in ("u", "X", "status", "iters", "res"):
        assert np.array_equal(got[k], plain[k]), k
    assert np.all(plain["status"] == 1)


def test_checker_with_two_classes_is_two_engines_on_the_halves(oracle_lib):
    kw = dict(N=10, delta=0.03, max_iter=4000)
    b = mpcqp.synth.config3(B=12)
    rows = mpcqp.synth.make_model_rows(12, classes=2)
    assert len(np.unique(rows, axis=0)) == 2 and np.array_equal(rows[0], rows[2]) and not np.array_equal(rows[0], rows[1])
    got = M.solve_batch_models_host(oracle_lib, kw, rows, b)
    for c in range(2):
        m, ixx, iyy, izz, lo, hi = rows[c]
        eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config(m=m, Ibody_inv=(1.0 / ixx, 1.0 / iyy, 1.0 / izz), f_min=lo, f_max=hi, **kw))
        idx = np.arange(c, 12, 2)
        o = eng.solve_batch_host(b["x0"][idx], b["r"][idx], b["contact"][idx], b["xdes"][idx], b["mu"][idx])
        for k in ("u", "X", "status", "iters"):
            assert np.array_equal(got[k][idx], o[k]), (c, k)
    assert np.all(got["status"] == 1)
    assert np.abs(got["u"][0::2] - got["u"][1::2]).max() > 1e-3   # (the rows matter)


def test_row_helpers():
    body = mpcqp.plant.model_body(8.885, (1.0 / 0.24, 1.0, 1.0), 3)
    rows = M.models_from_bodies(body, 3.0, [100.0, 90.0, 80.0])
    assert rows.shape == (3, 6) and np.array_equal(rows[:, :4], body[:, :4]) and np.all(rows[:, 4] == 3.0)
    assert rows[:, 5].tolist() == [100.0, 90.0, 80.0]
    body[1, 5] = 1e-3
    with pytest.raises(ValueError, match="products of inertia"):
        M.models_from_bodies(body, 3.0, 100.0)
    with pytest.raises(ValueError, match="products of inertia"):
        M.models_from_bodies(mpcqp.synth.make_plant_rows(4)["body"], 3.0, 100.0)
    r = mpcqp.synth.make_model_rows(10)
    assert r.shape == (10, 6) and r.dtype == np.float64 and len(np.unique(r, axis=0)) == 4
    assert np.array_equal(r[:4], r[4:8]) and np.all(r[:, :4] > 0) and np.all(r[:, 4] >= 0) and np.all(r[:, 5] >= r[:, 4])
    low = 2.0 * r[:, 5] < r[:, 0] * G
    assert low[3] and low[7]   # the last class carries less than its weight on two legs
    assert np.array_equal(r, mpcqp.synth.make_model_rows(10))


def test_low_fmax_class_reaches_its_upper_bound_on_a_trot(oracle_lib):
    """The class with 2 f_max < m |g|: in two-legged (trot) support the checker's optimum has f_z = f_max."""
    B = 16
    b = mpcqp.synth.config2(B=B)
    rows = mpcqp.synth.make_model_rows(B)
    o = M.solve_batch_models_host(oracle_lib, dict(N=10, delta=0.03, max_iter=4000), rows, b)
    assert np.all(o["status"] == 1)
    fz = o["u"].reshape(B, 10, 4, 3)[:, :, :, 2]
    low = np.arange(B) % 4 == 3
    assert np.all(fz <= rows[:, 5][:, None, None] + 1e-9)
    assert np.any(np.abs(fz[low] - rows[low, 5][:, None, None]) <= 1e-9)


def test_matched_controller_holds_its_height_better(oracle_lib):
    """What the feature is for, on the checker alone: robots 1.25 x the nominal mass, the controller that knows it (matched rows)
    against the one that assumes the nominal mass.  Mean |z - z_des| over ticks 20..59 is smaller for every robot."""
    B, T = 4, 60
    kw = dict(N=10, delta=0.03, max_iter=4000)
    cfg = oracle_lib.default_config(**kw)
    rb = mpcqp.synth.make_rollout_batch(B, seed=11)
    body = mpcqp.plant.model_body(1.25 * cfg.m, list(cfg.Ibody_inv), B)
    args = (rb["x"], rb["ref"], rb["plan_pos"], rb["plan_feet_id"], rb["plan_meta"], rb["tick"], rb["mu"], T)
    matched = M.rollout_plant_models_host(oracle_lib, kw, M.models_from_bodies(body, cfg.f_min, cfg.f_max), *args, body=body)
    nominal = M.rollout_plant_models_host(oracle_lib, kw, M.model_rows(cfg, B), *args, body=body)
    assert np.all(matched["solved"] == T) and np.all(nominal["solved"] == T)
    err = lambda o: np.abs(o["actual"][:, 20:, 5] - o["desired"][:, 20:, 5]).mean(axis=1)
    em, en = err(matched), err(nominal)
    print("height error, matched / nominal rows (mm):", np.round(em * 1e3, 3).tolist(), np.round(en * 1e3, 3).tolist())
    assert np.all(em < en), (em, en)
