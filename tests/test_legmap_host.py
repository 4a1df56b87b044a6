"""The structured leg maps (csrc/mpcqp_legmap.h) against the dense expressions they replace, on the host: tools/legmap_check.cpp is
compiled with the host compiler (-ffp-contract=off, explicit fma) and run.  It checks, in fp32 and fp64 and for both kinds of map
(ADMM, polish), on random legs, swing legs, zeros of both signs, denormals and magnitudes up to 1e30: every output equal as a value,
bit patterns different only where both results are zeros, and the 21 entries of E bitwise equal once added to a +0 or non-zero K^-1
entry; the rows handed to the polish's staging records bitwise.  No GPU.  The host build does not exercise `LEGMAP_EXACT` (the pragma
that forbids fp contraction inside the maps is defined for clang only, and the host is compiled with -ffp-contract=off): its effect in
the device compile is covered by tests/test_gpu_accel_identity.py and tests/test_gpu_legmap_identity.py alone."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mpc-for-dynamic-locomotion-in-the-mit-cheetah-3_amd", "csrc")


def test_structured_maps_equal_the_dense_expressions(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++ / g++ / clang++) on PATH")
    exe = str(tmp_path / "legmap_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(REPO, "tools", "legmap_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    checked, zeros, failures = (int(w) for w in r.stdout.split() if w.isdigit())
    assert failures == 0 and checked > 500000
    assert zeros > 0, "the inputs never produced a zero of the other sign: the check does not reach what it is for"
