"""The C-ABI libraries load and export every symbol include/mpcqp.h declares (no compute without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

import mpcqp
from conftest import REPO, _have_gpu


def _declared_symbols():
    hdr = open(os.path.join(REPO, "include", "mpcqp.h")).read()
    return sorted(set(re.findall(r"\b(mpcqp_[a-z_]+)\s*\(", hdr)))


def test_header_symbols_match_binding():
    assert set(_declared_symbols()) == set(mpcqp._capi.EXPORTED_SYMBOLS)


def test_product_library_exports_all_symbols_at_version_1_3_1():
    lib = mpcqp.product_library()            # fails loudly if the HIP library has not been built
    for sym in _declared_symbols():
        assert hasattr(lib.lib, sym), sym
    hdr = open(os.path.join(REPO, "include", "mpcqp.h")).read()
    assert lib.version() == 0x00010301 == int(re.search(r"#define MPCQP_VERSION (0x[0-9a-fA-F]+)", hdr).group(1), 16)


def test_oracle_exports_same_symbols(oracle_lib):
    for sym in _declared_symbols():
        assert hasattr(oracle_lib.lib, sym), sym


def test_config_struct_layout_and_defaults(oracle_lib):
    plib = mpcqp.product_library()
    for lib in (plib, oracle_lib):
        cfg = lib.default_config()
        assert cfg.size == ctypes.sizeof(mpcqp.MpcQpConfig)
        # Lite3 constants hard-coded in the reference (src/mpc.py:45-46,71-76,122-134)
        assert cfg.N == 10 and abs(cfg.delta - 0.03) < 1e-15
        assert cfg.m == 8.885 and list(cfg.Ibody_inv) == [1 / 0.24, 1.0, 1.0]
        assert list(cfg.w) == [1e4, 2.7e4, 1e4, 2.7e5, 2.7e5, 2.7e5, 1e4, 1e4, 1e4, 1.6e4, 1.6e4, 1.6e4, 0.0]
        assert (cfg.f_min, cfg.f_max) == (3.0, 100.0)
        assert cfg.disc == mpcqp.DISC_EULER


def test_host_layer_scales_the_admm_block_with_the_horizon(oracle_lib):
    """The C default (100 iterations per block, cap 400) is tuned for N = 10; the Python host layer uses 10 N / 40 N for
    other horizons unless the caller says otherwise (include/mpcqp.h, `check_every`)."""
    for lib in (oracle_lib, mpcqp.product_library()):
        c10, c20 = lib.default_config(), lib.default_config(N=20)
        assert (c20.check_every, c20.max_iter, c20.polish_max) == (2 * c10.check_every, 2 * c10.max_iter, 2 * c10.polish_max)
        assert lib.default_config(N=20, polish_max=3).polish_max == 3
        c = lib.default_config(N=20, check_every=50)
        assert (c.check_every, c.max_iter) == (50, c10.max_iter)
        assert lib.default_config(N=20, max_iter=1000).max_iter == 1000
    p10 = mpcqp.product_library().default_config()
    assert (p10.check_every, p10.max_iter) == (100, 400)
    # other horizons run on the stage-wise engine: blocks of 5 N / 3 iterations (its first block is Anderson-accelerated), the polish budget of N = 20
    p60 = mpcqp.product_library().default_config(N=60, delta=0.01)
    assert (p60.check_every, p60.max_iter, p60.polish_max) == (100, 2400, 8)
    assert p60.accel == 0 and mpcqp.product_library().default_config(accel=-1).accel == -1     # (0 = the engine's default: on)
    flags = mpcqp.product_library().default_config(
        flags=mpcqp.FLAG_POLISH | mpcqp.FLAG_WARM_START | mpcqp.FLAG_WARM_SHIFT | mpcqp.FLAG_NATURAL_ORDER).flags
    assert flags == 1 | 2 | 16 | 8


def test_product_library_reads_no_environment():
    """Solver behaviour is a function of MpcQpConfig alone: the product library does not import getenv (round-2 review: developer
    knobs read from the environment could silently change a caller's results)."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--undefined-only", mpcqp.product_library().path], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in out


def test_product_never_falls_back_to_cpu():
    """Without a gfx950 device the product library refuses to create an engine (MPCQP_ENODEV), it does not emulate."""
    if _have_gpu():
        pytest.skip("GPU present")
    lib = mpcqp.product_library()
    with pytest.raises(mpcqp.MpcQpError, match="-4"):
        mpcqp.Engine(lib, lib.default_config())
    with pytest.raises(mpcqp.MpcQpError):
        mpcqp.MPCBatch()


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(mpcqp.MpcQpError, match="not found"):
        mpcqp.Library(str(tmp_path / "libmpcqp.so"))


def test_bad_config_rejected(oracle_lib):
    cfg = oracle_lib.default_config()
    cfg.size = 8
    with pytest.raises(mpcqp.MpcQpError):
        mpcqp.Engine(oracle_lib, cfg)
    plib = mpcqp.product_library()
    for kw in (dict(N=0), dict(N=65), dict(precision=9), dict(relax=2.5), dict(delta=-1.0), dict(disc=5)):
        with pytest.raises(mpcqp.MpcQpError, match="-1"):
            mpcqp.Engine(plib, plib.default_config(**kw))


# ---- the binding's table of the C-ABI (mpcqp._capi.ABI) against the prototypes of the five headers
_C_RETURN = {"uint32_t": ctypes.c_uint32, "const char*": ctypes.c_char_p, "int": ctypes.c_int}
_C_INTEGER = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}


def _prototypes(header):
    """{name: (return type, [parameter declarations])} of a header.  The comments name functions too, so a prototype is what starts
    with its return type at the start of a line and ends in `);`."""
    text = open(os.path.join(REPO, "include", header)).read()
    found = re.findall(r"^(uint32_t|const char\*|int) (mpcqp_[a-z_]+)\(([^;{]*)\);", text, re.M)
    return {name: (ret, [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]) for ret, name, params in found}


def _is_pointer_type(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)


@pytest.mark.parametrize("header", list(mpcqp._capi.ABI))
def test_abi_table_matches_the_header(header):
    protos = _prototypes(header)
    table = {name: (restype, argtypes) for name, restype, argtypes in mpcqp._capi.ABI[header]}
    assert len(table) == len(mpcqp._capi.ABI[header])                      # every function once
    assert set(table) == set(protos) and len(protos) >= 2
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is _C_RETURN[ret], name
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            ctype = decl.rsplit(" ", 1)[0]                                     # the declaration without the parameter's name
            if "*" in ctype or ctype == "mpcqp_handle":
                assert _is_pointer_type(t), (name, i, decl, t)
            else:
                assert t is _C_INTEGER[ctype], (name, i, decl, t)          # (a by-value type the table does not know is a KeyError)


def test_abi_table_is_what_a_library_binds(oracle_lib):
    """The symbol tuples are the table's names, and a loaded library carries the table's types (the product library: all five headers)."""
    capi = mpcqp._capi
    families = (capi.EXPORTED_SYMBOLS, capi.PLAN_SYMBOLS, capi.SIM_SYMBOLS, capi.MODEL_SYMBOLS, capi.JOINTS_SYMBOLS)
    assert [tuple(r[0] for r in rows) for rows in capi.ABI.values()] == list(families) and list(capi.ABI)[0] == "mpcqp.h"
    plib = mpcqp.product_library()
    assert plib.has_plan and plib.has_sim and plib.has_model and plib.has_joints
    for lib, headers in ((plib, list(capi.ABI)), (oracle_lib, ["mpcqp.h"])):
        for header in headers:
            for name, restype, argtypes in capi.ABI[header]:
                fn = getattr(lib.lib, name)
                assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name


def test_call_names_the_missing_header_and_reports_the_librarys_message(oracle_lib):
    """Engine._call, the one path into the library, on the checker: an extension call says which header is missing; a failing core
    call carries the return code and the library's own message; a 0 address is NULL."""
    eng = mpcqp.Engine(oracle_lib, oracle_lib.default_config())
    for call, header in ((lambda: eng.plan_footsteps_ptr(1, 2, 0, 0, 0, 0, 0, 0), "mpcqp_plan.h"),
                         (lambda: eng.plant_step_ptr(1, 0, 0, 0, 0, 0, 0, 10, 0), "mpcqp_sim.h"),
                         (lambda: eng.clear_models(), "mpcqp_model.h"),
                         (lambda: eng.joint_log_ptr(1, 1, 0, 0, 0, 0, 0, 0), "mpcqp_joints.h")):
        with pytest.raises(mpcqp.MpcQpError, match=rf"{re.escape(oracle_lib.path)} does not export include/{header} \(product library only\)"):
            call()
    buf = np.zeros(2048)
    a = buf.ctypes.data
    with pytest.raises(mpcqp.MpcQpError, match=r"mpcqp_solve_batch failed with code -1: mpcqp_solve_batch: null buffer or negative batch"):
        eng.solve_batch_ptr(-1, a, a, a, a, a, a, a, a, a, a)
    with pytest.raises(mpcqp.MpcQpError, match=r"mpcqp_solve_batch failed with code -1: mpcqp_solve_batch: null buffer or negative batch"):
        eng.solve_batch_ptr(1, 0, a, a, a, a, a, a, a, a, a)                   # x0 = 0 arrives as NULL
    with pytest.raises(mpcqp.MpcQpError, match=r"mpcqp_solve_batch_gait_steps failed with code -1: mpcqp_solve_batch_gait: .*no plan step"):
        eng.solve_batch_gait_steps_ptr(1, 0, a, a, a, a, a, a, a, a, a, a, a, a)
    eng.solve_batch_ptr(0, 0, 0, 0, 0, 0, 0, None, 0, 0, None)                 # the empty batch needs no buffer: 0 and None alike
    with pytest.raises(TypeError, match="mpcqp_reserve takes 1 arguments"):   # one too many is not cut off
        eng._call("mpcqp_reserve", 4, 0)
    eng.reserve(4)
    assert buf.sum() == 0.0


# ---- the operand check of every MPCBatch method (mpcqp.engine.check_operands), on CPU tensors
def test_operand_check():
    import torch
    check = mpcqp.engine.check_operands
    cpu = torch.device("cpu")
    x, c = torch.zeros(5, 13), torch.zeros(5, 4, dtype=torch.uint8)
    rows = lambda x=x, c=c: [("x0", x, (5, 13), torch.float32), ("contact", c, (5, 4), torch.uint8)]
    check(cpu, rows())
    check(cpu, rows(c=None), optional=("contact",))                            # an optional operand that is not given
    check(cpu, [("x0", torch.zeros(0, 13), (0, 13), torch.float32)])             # the empty batch
    bad = {"shape": torch.zeros(5, 12), "dtype": torch.zeros(5, 13, dtype=torch.float64), "layout": torch.zeros(13, 5).t(),
           "device": torch.zeros(5, 13, device="meta"), "required": None}
    assert tuple(bad["layout"].shape) == (5, 13) and not bad["layout"].is_contiguous()
    said = {}
    for what, t in bad.items():
        with pytest.raises(ValueError, match=r"operand mismatch: x0 expected \(5, 13\) torch.float32 contiguous on cpu, got ") as e:
            check(cpu, rows(x=t), optional=("contact",))
        said[what] = str(e.value).split("got ")[1]
    assert said == {"shape": "(5, 12) torch.float32 on cpu", "dtype": "(5, 13) torch.float64 on cpu",
                    "layout": "(5, 13) torch.float32 non-contiguous on cpu", "device": "(5, 13) torch.float32 on meta", "required": "None"}
    with pytest.raises(ValueError, match="operand mismatch: contact expected"):   # the second row, by its own name
        check(cpu, rows(c=torch.zeros(5, 4)))
    with pytest.raises(ValueError, match="operand mismatch: contact expected .* got None"):
        check(cpu, rows(c=None), optional=("x0",))
