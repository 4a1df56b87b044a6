"""tools/rs8_forms.hip: the select form and the banked form of the reduce-scatter's first step (csrc/mpcqp_leg.h: rs8, rs8_banked),
result words compared on the device over every lane of a wave (all eight grid rows: both bank parities) and operand sets of random
values, signed zeros, denormals, +-inf and a NaN in a single lane and element.  The two forms add the same operands in the other
order, so the set of differing words is EMPTY; the device test holds the program's DIFF lines against that.  The host test holds the
program's copies of the two functions against the text of csrc/mpcqp_leg.h, so that the forms compared are the forms the kernels run."""
import os
import re
import subprocess

import pytest

from conftest import REPO

TOOL = os.path.join(REPO, "tools", "rs8_forms.hip")
CSRC = os.path.join(REPO, "mpc-for-dynamic-locomotion-in-the-mit-cheetah-3_amd", "csrc")


def read(path):
    with open(path) as f:
        return f.read()


def between(text, begin, end):
    return text.split(begin, 1)[1].split("\n", 1)[1].split(end, 1)[0]


def test_the_programs_forms_are_textually_those_of_the_kernels():
    tool, leg = read(TOOL), read(os.path.join(CSRC, "mpcqp_leg.h"))
    select = re.search(r"template <typename T>\n__device__ __forceinline__ T rs8\(.*?\n}\n", leg, re.S).group(0)
    banked = re.search(r"__device__ __forceinline__ float rs8_banked\(.*?\n}\n", leg, re.S).group(0)
    assert between(tool, "// BEGIN RS8 ", "// END RS8\n") == select
    assert between(tool, "// BEGIN RS8_BANKED", "// END RS8_BANKED\n") == banked
    assert "hi ? v[4 + m] : v[m]" in select and "bank_mask:0x5" in banked and "bank_mask:0xa" in banked and "row_half_mirror" in banked
    # the lane move of the program is the library's
    mov = re.search(r"template <int CTRL>\n__device__ __forceinline__ float dpp_mov\(float v\) \{.*?\n}\n", read(os.path.join(CSRC, "mpcqp_device.h")), re.S).group(0)
    assert mov in tool
    # ... and the mat-vec takes the banked form where the switch says so, the select form elsewhere
    wrench = read(os.path.join(CSRC, "mpcqp_wrench.h"))
    assert wrench.count("rs8_banked(acc, gc & 7)") == 1 and wrench.count("rs8<TM>(acc, gc & 7)") == 1
    assert "template <int N, bool MIXED> constexpr bool W_TRIM_RS8 = N == 10 && MIXED;" in wrench


def test_the_operand_sets_listed_in_the_tool_are_the_ones_it_runs():
    src = read(TOOL)
    for token in ('"random"', '"zeros"', '"zeros_and_values"', '"denormals"', '"denormals_and_values"', '"inf_sparse"', '"inf_dense"', '"nan_l"',
                  "0x7fc00000u", "0xffc00000u", "INFINITY : -INFINITY", "dim3(1), dim3(64)", "rs8<float>(v, lane & 7)", "rs8_banked(v, lane & 7)"):
        assert token in src, token
    nan_lanes = {(13 * k + 5) % 64 for k in range(16)}
    assert {(l >> 3) & 1 for l in nan_lanes} == {0, 1} and {(l >> 2) & 1 for l in nan_lanes} == {0, 1}   # both row parities, both halves of a group


@pytest.mark.gpu
def test_the_two_forms_give_the_same_words(tmp_path):
    exe = str(tmp_path / "rs8_forms")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-o", exe, TOOL], check=True, cwd=str(tmp_path))
    r = subprocess.run(["timeout", "-k", "10", "60", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    total = re.search(r"^rs8_forms: (\d+) words, (\d+) differ \((\d+) sets, (\d+) NaN and (\d+) inf results\)$", r.stdout, re.M)
    assert total and int(total[1]) == 64 * int(total[3]) and int(total[3]) >= 26
    assert int(total[4]) >= 16 and int(total[5]) > 0   # the NaN and inf operands reached results
    diffs = set(re.findall(r"^DIFF (\w+) lane=(\d+) ", r.stdout, re.M))
    assert len(diffs) == int(total[2])
    assert diffs == set(), sorted(diffs)
