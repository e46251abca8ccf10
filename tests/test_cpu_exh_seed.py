"""CPU: the seed form of the exhaustive sweep's integer root (csrc/exh_arith.hpp: exh_seed_arg, exh_seed_ki, exh_seed_k and the
one-sided fix-up exh_e / exh_up / exh_d) as the very source text k_exh compiles, built with the host compiler
(tests/exh_seed_check.cpp) and compared with integer arithmetic.

For k from 0 to 2^21 - 2 (dense at both ends, sampled between; about 1.9e5 values), s at k^2 + k + {-1..2}, k^2 + {-1..2},
10 k^2 + {-1..2} and 10 k^2 + 5k + {-1..2} -- both sides of every rounding boundary of EUC_2D (nint), CEIL_2D and ATT, wherever
the root stays below the 2^21 the integer-coordinate metrics guarantee, s = 0 included -- each with the seed
sqrtf((float) argument) moved by 0, +-1 and +-2 fp32 ulps (the hardware's fp32 root is within 1 ulp): zero mismatches.
The sweep can fail: over roots in (2^21, 2.9e6], where an fp32 ulp is 0.25 and +-2 ulps reach the fix-up's margin of 0.5, the
same driver reports mismatches."""
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
    exe = str(tmp_path_factory.mktemp("exh_seed") / "exh_seed_check")
    # -ffp-contract=off as in csrc/Makefile: the fmas of the header are the only fused operations
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "exh_seed_check.cpp"), "-lm"])
    return exe


def _run(exe, *args):
    return subprocess.run([exe, *args], check=True, capture_output=True, text=True, timeout=900).stdout


def _last(out):
    return dict(f.split("=") for f in out.strip().splitlines()[-1].split()[1:])


def test_seed_form_equals_integer_arithmetic_with_the_seed_two_ulps_off(driver):
    out = _run(driver, "sweep")
    last = _last(out)
    print(out[-2000:])
    assert int(last["k_values"]) >= 150000 and int(last["cases"]) >= 2 * 10**7
    assert int(last["zero_cases"]) >= 3                # s = 0 with the seed 0, every metric
    assert int(last["mismatches"]) == 0, out[:3000]


def test_the_sweep_can_fail_past_two_to_the_21(driver):
    out = _run(driver, "beyond")
    last = _last(out)
    print(out[-2000:])
    assert int(last["cases"]) >= 10**7
    assert int(last["mismatches"]) > 0, out


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


def test_a_sample_of_the_seed_form_against_math_isqrt(driver):
    """The driver's own reference is integer arithmetic in C; a second opinion on every 97th case from Python's integers."""
    rows = [tuple(int(v) for v in line.split()) for line in _run(driver, "sample", "97").splitlines()]
    assert len(rows) > 200000
    assert {r[0] for r in rows} == {0, 1, 2} and {r[2] for r in rows} == {0, 1, -1, 2, -2}
    assert max(r[1] for r in rows) > 4 * 10**13
    bad = [(m, s, d, got) for m, s, d, got in rows if got != _ref(m, s)]
    assert not bad, bad[:10]
