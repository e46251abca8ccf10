"""CPU: the arithmetic of the exhaustive sweep (csrc/exh_arith.hpp) as the very source text k_move_pos and k_exh compile, built
with the host compiler (tests/exh_arith_check.cpp) and compared with integer arithmetic.

The rounded roots: for k from 0 to 2^21 - 2 (dense at both ends, sampled between; about 2e5 values), s at k^2 + k + {-1..2},
k^2 + {-1..2}, 10 k^2 + {-1..2} and 10 k^2 + 5k + {-1..2} -- both sides of every rounding boundary of EUC_2D (nint), CEIL_2D and
ATT, wherever the root stays below the 2^21 the integer-coordinate metrics guarantee -- each with g = sqrt(s) (1 + delta),
delta in {0, +-2^-25, +-2^-23}: the hardware root's measured and documented relative error.  Zero mismatches.
The squared distance from norms: bit-equal to dx^2 + dy^2 and to the integer on random relative coordinates up to +-(2^21 - 1),
extremes and the pad position included.
The strips: exh_strip and exh_total_rows, the helpers the kernel and the host share."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsp_optimization_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("exh_arith") / "exh_arith_check")
    # -ffp-contract=off as in csrc/Makefile: the fmas of the header are the only fused operations
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "exh_arith_check.cpp"), "-lm"])
    return exe


def _run(exe, *args):
    return subprocess.run([exe, *args], check=True, capture_output=True, text=True, timeout=900).stdout


def test_rounded_roots_equal_integer_arithmetic_on_every_boundary(driver):
    out = _run(driver, "sweep")
    last = dict(f.split("=") for f in out.strip().splitlines()[-1].split()[1:])
    print(out[-2000:])
    assert int(last["k_values"]) >= 150000 and int(last["cases"]) >= 2 * 10**7
    assert int(last["mismatches"]) == 0, out[:3000]


def _ref(mode, s):
    k = math.isqrt(s)
    if mode == 0:
        return k + 1 if s > k * k + k else k           # nint(sqrt(s))
    if mode == 1:
        return k if k * k == s else k + 1             # ceil(sqrt(s))
    k = math.isqrt(s // 10)
    while 10 * k * k < s:                             # the smallest k with 10 k^2 >= s
        k += 1
    return k


def test_a_sample_of_the_roots_against_math_isqrt(driver):
    """The driver's own reference is integer arithmetic in C; a second opinion on every 97th case from Python's integers."""
    rows = [tuple(int(v) for v in line.split()) for line in _run(driver, "sample", "97").splitlines()]
    assert len(rows) > 200000
    assert {r[0] for r in rows} == {0, 1, 2} and {r[2] for r in rows} == {0, 1, 2, 3, 4}
    assert max(r[1] for r in rows) > 4 * 10**13
    bad = [(m, s, d, got) for m, s, d, got in rows if got != _ref(m, s)]
    assert not bad, bad[:10]


def test_squared_distance_from_norms_is_the_same_number(driver):
    out = _run(driver, "norms")
    last = dict(f.split("=") for f in out.strip().splitlines()[-1].split()[1:])
    assert int(last["cases"]) == 2000000 and int(last["mismatches"]) == 0, out[:3000]


def test_strips_are_right_aligned_and_cover_every_pair(driver):
    """exh_strip / exh_total_rows (the helpers k_exh and the host's share arithmetic call): enumerating the pairs the way the kernel
    walks its strips meets every pair p' < q' <= n - 1 at twenty sizes around the strip boundaries, pairs are met twice only where
    the clamped strip 0 overlaps strip 1, the total never exceeds that of strips laid out from column 0 and is n - 1 below one
    strip -- and the row units at n = 10 000 are 201 060 (208 860 with the slack in the last strip)."""
    out = _run(driver, "strips")
    last = dict(f.split("=") for f in out.strip().splitlines()[-1].split()[1:])
    assert int(last["sizes"]) == 20 and int(last["pairs"]) > 5 * 10**6
    assert int(last["uncovered"]) == 0 and int(last["bad_totals"]) == 0, out
    assert int(last["total10000"]) == 201060
