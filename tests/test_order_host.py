"""The dispatch-order score (csrc/mpcqp_order.h: order_stage, cost_class) on the host: tools/order_check.cpp, compiled with the host
compiler (-ffp-contract=off), against a restatement in numpy float32 scalars written from the description of the score, on 256
synthetic horizon-10 QPs: all 16 support patterns x mu in {0.3, 1.0} x zero and large state offsets x four ways of placing the
pattern in the horizon (every stage; after j four-legged stages; for the first j stages; mixed with its complement).  Classes, stage
masks and the stance count must be EQUAL, the two maxima equal to the last bit.  A second, short file carries non-finite and 1e30
entries: those QPs must land in class 0.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mpc-for-dynamic-locomotion-in-the-mit-cheetah-3_amd", "csrc")
N = 10
F = np.float32
COEF = [F(v) for v in (-9.2251, 1.0399, 1.0684, 0.14989, 0.11830, 1.1557, 2.2787, -0.013650)]


def synthetic():
    """256 QPs as float32 arrays x0 [B,13], r [B,N,4,3], contact [B,N,4], xdes [B,N+1,13], mu [B]."""
    import mpcqp
    base = mpcqp.synth.make_batch(256, N, 0.03, 20261021, ("trot",), (1.0,))
    x0, r, xdes = base["x0"].copy(), base["r"].copy(), base["xdes"].copy()
    contact = np.ones((256, N, 4), np.uint8)
    mu = np.empty(256)
    rng = np.random.default_rng(7)
    b = 0
    for pat in range(16):
        legs = np.array([(pat >> l) & 1 for l in range(4)], np.uint8)
        for m in (0.3, 1.0):
            for big in (False, True):
                for place in range(4):
                    j = int(rng.integers(1, 6))
                    if place == 0:
                        contact[b, :] = legs
                    elif place == 1:
                        contact[b, j:] = legs
                    elif place == 2:
                        contact[b, :j] = legs
                    else:
                        contact[b] = np.where(rng.integers(0, 2, (N, 1)) == 1, legs[None, :], 1 - legs[None, :])
                    if big:      # a large commanded correction: velocity, position and attitude far from the reference
                        x0[b, 9:12] += rng.normal(0.0, 1.5, 3); x0[b, 3:6] += rng.normal(0.0, 0.3, 3); x0[b, 0:2] += rng.normal(0.0, 0.4, 2)
                    else:        # none at all: the state sits on the reference
                        x0[b, 9:12] = xdes[b, 0, 9:12]; x0[b, 3:6] = xdes[b, 0, 3:6]; x0[b, 0:2] = 0.0; x0[b, 6:9] = 0.0
                    mu[b] = m
                    b += 1
    assert b == 256
    return x0.astype(F), r.astype(F), contact, xdes.astype(F), mu.astype(F)


def write_file(path, x0, r, contact, xdes, mu):
    B = len(mu)
    with open(path, "wb") as f:
        np.array([N, B], np.int32).tofile(f)
        for b in range(B):
            np.concatenate([x0[b].ravel(), r[b].ravel(), contact[b].astype(F).ravel(), xdes[b].ravel(), mu[b:b + 1]]).astype(F).tofile(f)


def restated(x0, r, contact, xdes, mu):
    """(class, two mask, saturated mask, stance leg-stages, max demand, max hv) of one QP, in float32 scalar arithmetic."""
    bad = not np.isfinite(mu)
    inv_mu = F(1) / max(abs(mu), F(1e-3))
    two = sat = 0
    dmax = hvmax = cnt = F(0)
    with np.errstate(all="ignore"):
        for k in range(N):
            st = [l for l in range(4) if contact[k, l]]
            fx, fy, fz = r[k, :, 0], r[k, :, 1], r[k, :, 2]
            dem = F(0)
            if len(st) == 2:
                a, b = st
                dx, dy = fx[a] - fx[b], fy[a] - fy[b]
                n2, cr, hz = dx * dx + dy * dy, abs(fx[a] * fy[b] - fy[a] * fx[b]), F(-0.5) * (fz[a] + fz[b])
                dem = cr / max(np.sqrt(n2), F(1e-6)) / max(hz, F(1e-3)) if np.isfinite(n2 + cr + abs(hz)) else F(np.nan)
            elif len(st) == 1:
                a = st[0]
                n2 = fx[a] * fx[a] + fy[a] * fy[a]
                dem = np.sqrt(n2) / max(-fz[a], F(1e-3)) if np.isfinite(n2 + abs(fz[a])) else F(np.nan)
            dem = F(dem * inv_mu)
            evx, evy = x0[9] - xdes[k + 1, 9], x0[10] - xdes[k + 1, 10]
            hv = F(np.sqrt(evx * evx + evy * evy) * inv_mu)
            is_two = len(st) in (1, 2)
            two |= int(is_two) << k
            sat |= int(is_two and dem > 1) << k
            bad = bad or not (np.isfinite(dem) and np.isfinite(hv))
            dmax = dem if dem > dmax else dmax       # fmaxf(dmax, dem): a NaN on the right is dropped
            hvmax = hv if hv > hvmax else hvmax
            cnt = F(cnt + F(len(st)))
        bits = lambda m: [(m >> k) & 1 for k in range(N)]
        tb, sb = bits(two), bits(sat)
        lead = next((k for k in range(N) if not sb[k]), N)
        s = next((k for k in range(N) if tb[k]), N)
        L = next((k for k in range(s, N) if not tb[k]), N) - s
        nsat = sum(sb[s:s + L])
        late = F(L * 2.0 ** (1 - s)) if s >= 1 else F(0)
        late_sat = F(F(late * F(nsat)) / F(max(L, 1)))
        has_late = F(1 if s >= 1 and L >= 1 else 0)
        swing10 = F(F(40) - F(cnt * F(F(10) / F(N))))
        z = COEF[0]
        for c, t in zip(COEF[1:], (F(min(lead, 6)), min(dmax, F(2)), late, late_sat, hvmax, has_late, swing10)):
            z = F(z + F(c * t))
        cls = 0 if bad or not np.isfinite(z) else int(min(max(F(F(z + F(9.5)) * F(2)), F(0)), F(15)))
    return cls, two, sat, float(cnt), dmax, hvmax


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++ / g++ / clang++) on PATH")
    exe = str(tmp_path_factory.mktemp("order") / "order_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(REPO, "tools", "order_check.cpp"), "-o", exe], check=True)

    def run(path):
        out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert out.returncode == 0, out.stdout[-2000:]
        return [ln.split() for ln in out.stdout.splitlines()]
    return run


def test_host_score_equals_the_numpy_restatement(checker, tmp_path):
    q = synthetic()
    path = str(tmp_path / "qps.bin")
    write_file(path, *q)
    lines = checker(path)
    assert len(lines) == 256
    seen = set()
    for b, ln in enumerate(lines):
        cls, two, sat, cnt, dmax, hvmax = restated(*(a[b] for a in q))
        got = (int(ln[0]), int(ln[1], 16), int(ln[2], 16), float(ln[3]))
        assert got == (cls, two, sat, cnt), (b, got, (cls, two, sat, cnt))
        assert F(ln[4]) == dmax and F(ln[5]) == hvmax, (b, ln, dmax, hvmax)
        seen.add(cls)
    assert len(seen) >= 8, f"the synthetic QPs reach only classes {sorted(seen)}: the check does not cover the score's range"


def test_non_finite_terms_select_class_zero(checker, tmp_path):
    x0, r, contact, xdes, mu = (a[:8].copy() for a in synthetic())
    contact[:] = np.array([1, 0, 1, 0], np.uint8)      # two-legged, same side, every stage: class 15 at mu = 0.3 when finite
    mu[:] = F(0.3)
    ref = restated(x0[0], r[0], contact[0], xdes[0], mu[0])[0]
    x0[1, 9] = np.nan; x0[2, 10] = np.inf; xdes[3, 4, 9] = -np.inf; r[4, 2, 0, 1] = np.nan; r[5, 7, 2, 0] = F(1e30); mu[6] = np.nan; mu[7] = np.inf
    path = str(tmp_path / "bad.bin")
    write_file(path, x0, r, contact, xdes, mu)
    got = [int(ln[0]) for ln in checker(path)]
    assert got[0] == ref and ref >= 12
    assert got[1:] == [0] * 7, got
