"""The state estimator on the device (include/mpcqp_estimate.h, mpcqp_imu_log / mpcqp_estimate_track) against its host counterparts
(mpcqp.estimator); the cases and the band are in tests/estimate_cases.py.  Every test calls the entry points unconditionally: a library
without them fails here, it does not skip.

  1. Device against host, both I/O dtypes: estimate_track on the real case, the exact case and every synthetic edge (outputs and the
     returned state), imu_log likewise.  NaN pattern and band; the band times the recorded growth where a state is carried over rows.
  2. The same call twice gives the same bits; the real case tiled to 2560 robots and shuffled equals the unshuffled rows bit for bit.
  3. Two pieces chained through `state` are one call bit for bit, with the cut after 13 rows and with the cut on a flight row.
  4. Wrong-index probes: one robot's init row, height row, one of its trust rows, its live state changed in turn.
  5. Poison: a NaN in each operand kind on one robot.
  6. trust = None is trust = (contact_log != 0); height = None leaves the x and y filters alone and changes z.
  7. The ABI: argument checks leave the outputs untouched and name the operand, no-ops, the struct size, live written as 1.
"""
import ctypes
import re

import numpy as np
import pytest

import estimate_cases as C
import mpcqp
from legsim_cases import DELTA
from mpcqp import estimator

pytestmark = pytest.mark.gpu

_ENGINES = {}
ROWWISE = ("imu", "q", "qd", "contact_log", "trust")                            # operands with a T axis


def _sol(io):
    if io not in _ENGINES:
        _ENGINES[io] = mpcqp.MPCBatch(N=10, delta=DELTA, io_dtype=io)
    return _ENGINES[io]


def _t(a, dt):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _track(sol, ops, state=None, **kw):
    """estimate_track on host operands -> numpy outputs; `state` (numpy [B,131]) comes back advanced as "state"."""
    import torch
    d = {k: _t(v, torch.uint8 if k == "contact_log" else sol.tdtype) for k, v in ops.items()}
    st = None if state is None else _t(state, torch.float64)
    out = sol.estimate_track(d["imu"], d["q"], d["qd"], d["contact_log"], d["init"], trust=d["trust"], height=d["height"], state=st, **kw)
    torch.cuda.synchronize()
    res = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    res["state"] = None if st is None else st.cpu().numpy()
    return res


def _imu(sol, case, **kw):
    import torch
    logs = {k: _t(case[k], sol.tdtype) for k in ("actual", "forces", "feet_log")}
    out = sol.imu_log(logs, **{k: _t(v, sol.tdtype) for k, v in C.imu_operands(case).items()}, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _case(kind, key):
    return {"real": C.real_case, "exact": C.exact_case, "edge": C.edge_case}[kind](*key)


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in estimator.OUT + ("state",) if a.get(k) is not None or b.get(k) is not None)


ALL_CASES = [("real", ()), ("exact", ())] + [("edge", k) for k in C.edge_cases()]


@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("kind,key", ALL_CASES)
def test_track_against_host(io, kind, key):
    sol = _sol(io)
    case = C.as_io(_case(kind, key), io)
    B = case["imu"].shape[0]
    host = C.host_result(kind, io, *key)
    dev = _track(sol, C.operands(case), state=np.zeros((B, estimator.EST_STATE)))
    g = C.growth()
    for k in estimator.OUT:
        err, band = C.error(dev[k], host[k], io)
        print(f"{kind} {key} {io} {k}: error {err:.3e}, band {band * g:.3e} (growth {g:.1f})")
        assert err <= band * g, k
    err, band = C.error(dev["state"], host["state"], "f64")                     # (fp64 in both I/O dtypes)
    print(f"{kind} {key} {io} state: error {err:.3e}, band {band * g:.3e}")
    assert err <= band * g and (dev["state"][:, 130] == 1.0).all()


@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("kind,key", ALL_CASES)
def test_imu_against_host(io, kind, key):
    sol = _sol(io)
    case = C.as_io(_case(kind, key), io)
    host = estimator.imu_log_host(case["actual"], case["forces"], case["feet_log"], **C.imu_operands(case))
    dev = _imu(sol, case)
    err, band = C.error(dev, host, io)
    print(f"{kind} {key} {io} imu: error {err:.3e}, band {band:.3e}")
    assert err <= band


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_imu_flight_and_poison(io):
    sol = _sol(io)
    case = dict(C.as_io(C.edge_case(65, 25, False), io))
    case["forces"] = case["forces"].copy()
    case["forces"][3, 4] = 0.0                                                  # a flight row: zero specific force before bias and noise
    plain = _imu(sol, dict(case, bias=None, noise=None))
    assert np.array_equal(plain[3, 4, 3:6], np.zeros(3))
    clean = _imu(sol, case)
    for name, idx in (("actual", (9, 7, 1)), ("actual", (9, 7, 7)), ("forces", (9, 7, 5)), ("noise", (9, 7, 2)), ("bias", (9, 4)), ("body", (9, 0))):
        bad = dict(case, **{name: case[name].copy()})
        bad[name][idx] = np.nan
        out = _imu(sol, bad)
        rows = np.zeros((65, 25), bool)
        rows[9, 7 if len(idx) == 3 else slice(None)] = True
        assert np.isnan(out[rows]).all() and np.array_equal(out[~rows], clean[~rows]), name
    feet = dict(case, feet_log=np.full_like(case["feet_log"], np.nan))          # the feet are not read
    assert np.array_equal(_imu(sol, feet), clean)


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_repeat_and_shuffle(io):
    sol = _sol(io)
    ops = C.operands(C.as_io(C.real_case(), io))
    a, b = _track(sol, ops, state=np.zeros((16, 131))), _track(sol, ops, state=np.zeros((16, 131)))
    assert _same(a, b)
    perm = np.random.default_rng(5).permutation(2560)
    src = perm % 16                                                             # robot i of the big batch is robot src[i] of the case
    big = {k: (None if v is None else np.ascontiguousarray(v[src])) for k, v in ops.items()}
    o = _track(sol, big, state=np.zeros((2560, 131)))
    for k in estimator.OUT + ("state",):
        assert np.array_equal(o[k], a[k][src]), k


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_pieces(io):
    sol = _sol(io)
    ops = C.operands(C.as_io(C.real_case(), io))
    flight = (ops["contact_log"].sum(axis=-1) == 0).any(axis=0)                 # rows on which some robot has no foot down
    cuts = [13, int(np.flatnonzero(flight[5:21])[0]) + 5]
    assert flight[cuts[1]]
    whole = _track(sol, ops, state=np.zeros((16, 131)))
    for cut in cuts:
        part = lambda s: {k: (v[:, s] if k in ROWWISE and v is not None else v) for k, v in ops.items()}
        a = _track(sol, part(slice(0, cut)), state=np.zeros((16, 131)))
        b = _track(sol, part(slice(cut, 25)), state=a["state"])
        for k in estimator.OUT:
            assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), whole[k]), (cut, k)
        assert np.array_equal(b["state"], whole["state"])
    nostate = _track(sol, ops)                                                  # state = NULL starts from init as zeros do
    assert all(np.array_equal(nostate[k], whole[k]) for k in estimator.OUT)


def _live_state(sol, ops):
    """A live state for the probes: the state after the case's first 5 rows."""
    head = {k: (v[:, :5] if k in ROWWISE and v is not None else v) for k, v in ops.items()}
    return _track(sol, head, state=np.zeros((ops["imu"].shape[0], 131)))["state"]


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_wrong_index_probes(io):
    sol = _sol(io)
    ops = C.operands(C.as_io(C.edge_case(65, 25, True), io))
    B, who = 65, 41
    others = np.arange(B) != who
    for name in ("init", "height", "trust", "state"):
        state = _live_state(sol, ops) if name == "state" else np.zeros((B, 131))
        clean = _track(sol, ops, state=state.copy())
        probe, st = dict(ops), state.copy()
        if name == "state":
            st[who, 4:22] += 0.01
            st[who, [22, 58, 94]] += 1e-3                                       # ... and the p variance of each axis
        elif name == "trust":
            probe["trust"] = ops["trust"].copy()
            probe["trust"][who, 0] = 1.0 - probe["trust"][who, 0]
        else:
            probe[name] = ops[name].copy()
            probe[name][who] += 0.01
        out = _track(sol, probe, state=st)
        for k in estimator.OUT + ("state",):
            assert np.array_equal(out[k][others], clean[k][others]), (name, k)
            if k != "sigma" or name in ("trust", "state"):                      # (P, and so sigma, does not depend on init or height)
                assert not np.array_equal(out[k][who], clean[k][who]), (name, k)
            else:
                assert np.array_equal(out[k][who], clean[k][who]), (name, k)


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_poison(io):
    sol = _sol(io)
    ops = C.operands(C.as_io(C.edge_case(65, 25, True), io))
    B, who, row = 65, 23, 11
    others = np.arange(B) != who
    live = _live_state(sol, ops)
    for name in ("imu", "q", "qd", "trust", "height", "init", "state"):
        state = live.copy() if name == "state" else np.zeros((B, 131))
        clean = _track(sol, ops, state=state.copy())
        probe, st = dict(ops), state.copy()
        if name == "state":
            st[who, 30] = np.nan                                                # an entry of P[x]'s upper triangle
            first = 0
        else:
            probe[name] = ops[name].copy()
            probe[name][(who, row, 2, 1)[:probe[name].ndim] if name in ROWWISE else (who, 1)] = np.nan
            first = row if name in ROWWISE else 0
        out = _track(sol, probe, state=st)
        for k in estimator.OUT:
            assert np.array_equal(out[k][others], clean[k][others]), (name, k)
            assert np.array_equal(out[k][who, :first], clean[k][who, :first]) and np.isnan(out[k][who, first:]).all(), (name, k)
        assert not np.isfinite(out["state"][who]).any() and np.array_equal(out["state"][others], clean["state"][others]), name


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_trust_and_height_defaults(io):
    sol = _sol(io)
    ops = C.operands(C.as_io(C.real_case(), io))
    a = _track(sol, ops, state=np.zeros((16, 131)))
    b = _track(sol, dict(ops, trust=(ops["contact_log"] != 0).astype(np.float64)), state=np.zeros((16, 131)))
    assert _same(a, b)
    h = _track(sol, dict(ops, height=np.zeros((16, 4))), state=np.zeros((16, 131)))
    assert np.array_equal(h["est"][..., [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]], a["est"][..., [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]])
    assert np.array_equal(h["feet"][..., :2], a["feet"][..., :2]) and np.array_equal(h["sigma"][..., [0, 1, 3, 4]], a["sigma"][..., [0, 1, 3, 4]])
    assert np.array_equal(h["state"][:, :16], a["state"][:, :16]) and np.array_equal(h["state"][:, 22:94], a["state"][:, 22:94])
    for k, sl in (("est", 5), ("est", 11), ("feet", 2), ("sigma", 2), ("sigma", 5)):
        assert not np.array_equal(h[k][..., sl], a[k][..., sl]), (k, sl)
    assert not np.array_equal(h["nis"], a["nis"])


def _par(**kw):
    par = mpcqp._capi.product_library().default_estimator()
    for k, v in kw.items():
        setattr(par, k, v)
    return par


def test_abi_estimate_track():
    import torch
    sol = _sol("f64")
    eng = sol.engine
    B, T = 3, 2
    ops = C.operands(C.edge_case(63, 2, True))
    d = {k: _t(v[:B], torch.uint8 if k == "contact_log" else torch.float64) for k, v in ops.items()}
    outs = [torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((B, T, 12), (B, T, 4, 3), (B, T, 6), (B, T))]
    state = torch.zeros((B, 131), dtype=torch.float64, device="cuda")
    p = lambda t: t.data_ptr()
    good = dict(B=B, T=T, imu=p(d["imu"]), q=p(d["q"]), qd=p(d["qd"]), contact_log=p(d["contact_log"]), trust=p(d["trust"]),
                height=p(d["height"]), init=p(d["init"]), state=p(state), est=p(outs[0]), feet_est=p(outs[1]), sigma=p(outs[2]), nis=p(outs[3]))
    geo = mpcqp._capi.MpcQpLegGeometry()
    bad = [(dict(B=-1), "size out of range"), (dict(T=-1), "size out of range"), (dict(B=0x20000000, T=1), "size out of range"),
           (dict(imu=0), r"null buffer \(imu, q, qd\)"), (dict(q=0), r"null buffer \(imu, q, qd\)"), (dict(qd=0), r"null buffer \(imu, q, qd\)"),
           (dict(init=0), "null init buffer"), (dict(trust=0, contact_log=0), "null contact_log buffer without trust"),
           (dict(est=0, feet_est=0, sigma=0, nis=0), "no output buffer"),
           (dict(estimator=_par(size=8)), "estimator struct size mismatch"), (dict(estimator=_par(r_v=float("nan"))), "estimator: kappa, q_"),
           (dict(estimator=_par(gravity=0.0)), "estimator: gravity"), (dict(estimator=_par(q_f=-1.0)), "estimator: kappa, q_"),
           (dict(estimator=_par(kappa=-0.5)), "estimator: kappa, q_"), (dict(geometry=geo), "geometry struct size mismatch")]
    for change, text in bad:
        with pytest.raises(mpcqp.MpcQpError, match="mpcqp_estimate_track: " + text):
            eng.estimate_track_ptr(**dict(good, **change))
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((state == 0.0).all())
    for change in (dict(B=0), dict(T=0)):                                       # no-ops, with or without buffers
        eng.estimate_track_ptr(**dict(good, **change))
        eng.estimate_track_ptr(**{k: (v if k in ("B", "T") or k == "est" else 0) for k, v in dict(good, **change).items()})
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((state == 0.0).all())
    state[1, 130] = 0.0
    eng.estimate_track_ptr(**good)
    torch.cuda.synchronize()
    assert bool((state[:, 130] == 1.0).all()) and all(bool(torch.isfinite(o).all()) and not bool((o == 7.0).all()) for o in outs)
    assert mpcqp._capi.product_library().has_estimate and ctypes.sizeof(mpcqp._capi.MpcQpEstimator) == 104
    par = mpcqp._capi.product_library().default_estimator()
    assert {k: getattr(par, k) for k in estimator.DEFAULTS} == estimator.DEFAULTS and par.size == 104


def test_abi_imu_log():
    import torch
    sol = _sol("f64")
    eng = sol.engine
    B, T = 3, 2
    case = C.edge_case(63, 2, True)
    d = {k: _t(case[k][:B], torch.float64) for k in ("actual", "forces", "feet_log")}
    imu = torch.full((B, T, 6), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t: t.data_ptr()
    good = dict(B=B, T=T, actual=p(d["actual"]), forces=p(d["forces"]), feet=p(d["feet_log"]), base_acc=0, body=0, bias=0, noise=0, imu=p(imu))
    bad = [(dict(B=-1), "size out of range"), (dict(T=-1), "size out of range"), (dict(B=0x20000000, T=1), "size out of range"),
           (dict(actual=0), "null buffer"), (dict(forces=0), "null buffer"), (dict(feet=0), "null buffer"), (dict(imu=0), "null imu buffer"),
           (dict(estimator=_par(size=8)), "estimator struct size mismatch"), (dict(estimator=_par(gravity=float("inf"))), "estimator: gravity")]
    for change, text in bad:
        with pytest.raises(mpcqp.MpcQpError, match="mpcqp_imu_log: " + re.escape(text)):
            eng.imu_log_ptr(**dict(good, **change))
    eng.imu_log_ptr(**dict(good, B=0))
    eng.imu_log_ptr(**dict(good, T=0))
    torch.cuda.synchronize()
    assert bool((imu == 7.0).all())
    eng.imu_log_ptr(**good)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(imu).all())
