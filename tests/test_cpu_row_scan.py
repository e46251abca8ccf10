"""CPU: the host pieces of the row-scan toolkit (csrc/row_scan.hpp: scan_chunks, write_sorted_edges, Carver, pi_finite), as
the very source text the kernels' host code compiles, built with the host compiler (tests/row_scan_check.cpp).

scan_chunks is held against the four chunk formulas the callers had before the toolkit, transcribed here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsp_optimization_amd", "csrc")

SIZES = list(range(3, 5001)) + [9999, 10000, 20011, 100003, 200000]
# the callers' constants: (target waves, most chunks, fewest columns)
HK, ALPHA, KNN = (8192, 64, 32), (4096, 16, 1), (4096, 16, 1)
GE = (32, 32)   # (most chunks, fewest columns)
NONE = object()


def hk_formula(n):
    waves = (n + 63) // 64
    want = max(1, min(64, (8192 + waves - 1) // waves))
    CH = max(32, (n + want - 1) // want)
    return CH, (n + CH - 1) // CH


def alpha_formula(n):
    waves = (n + 63) // 64
    Cc0 = max(1, min(16, (4096 + waves - 1) // waves))
    CH = (n + Cc0 - 1) // Cc0
    return CH, (n + CH - 1) // CH


knn_formula = alpha_formula   # the KNN build carried the same lines with constants of its own, equal to alpha's


def ge_formula(n):
    want = max(1, min(32, n // 32))
    CH = (n + want - 1) // want
    return CH, (n + CH - 1) // CH


@pytest.fixture(scope="module")
def sources():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # plain C++17, nothing of HIP: row_scan.hpp as the kernels include it; -ffp-contract=off as in csrc/Makefile
    return [cxx, "-std=c++17", "-ffp-contract=off", "-I", CSRC], os.path.join(ROOT, "tests", "row_scan_check.cpp")


@pytest.fixture(scope="module")
def cases():
    """(command text, expected answer or a checker) in the order they are run"""
    out = []
    for n in SIZES:
        out.append(("chunks %d %d %d %d" % ((n,) + HK), ("chunks", n, hk_formula(n), HK[1])))
        out.append(("chunks %d %d %d %d" % ((n,) + ALPHA), ("chunks", n, alpha_formula(n), ALPHA[1])))
        out.append(("chunks %d %d %d %d" % ((n,) + KNN), ("chunks", n, knn_formula(n), KNN[1])))
        out.append(("fewrows %d %d %d" % ((n,) + GE), ("chunks", n, ge_formula(n), GE[0])))
    rng = np.random.default_rng(20240611)
    out.append(("edges 6 5 3 9 0 2 -1 0 0 1 3 4 1 2", ("raw", "5 0 1 0 2 1 2 3 4 3 9")))   # an empty slot in the middle
    out.append(("edges 4 4 3 9 0 2 -1 0 0 1", ("raw", "3 -7 -7 -7 -7 -7 -7 -7 -7")))           # one edge short: nothing is written
    out.append(("edges 0 0", ("raw", "0")))
    for k in (0, 1, 12, 17):
        spec = [(int(rng.choice([1, 4, 8, 16, 32])), int(rng.choice([0, 1, 3, 31, 32, 33, 257, 1500]))) for _ in range(k)]
        out.append(("carve %d %s" % (k, " ".join("%d %d" % s for s in spec)), ("carve", spec)))
    out.append(("finite 0", ("raw", "1")))
    out.append(("finite 3 0.5 -1e300 7", ("raw", "1")))
    out.append(("finite 3 0.5 inf 7", ("raw", "0")))
    out.append(("finite 2 nan 1", ("raw", "0")))
    return out


@pytest.fixture(scope="module")
def results(sources, cases, tmp_path_factory):
    cmd, src = sources
    exe = str(tmp_path_factory.mktemp("row_scan") / "row_scan_check")
    subprocess.check_call(cmd + ["-O2", "-o", exe, src])
    text = "".join(c[0] + "\n" for c in cases)
    res = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=300)
    lines = res.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    return lines, res.stdout, text


def picked(cases, results, kind):
    return [(c[0], c[1], line) for c, line in zip(cases, results[0]) if c[1][0] == kind]


def test_scan_chunks_returns_the_callers_formulas_for_every_size(cases, results):
    rows = picked(cases, results, "chunks")
    assert len(rows) == 4 * len(SIZES)
    for text, (_, n, want, most), line in rows:
        CH, Cc = (int(t) for t in line.split())
        assert (CH, Cc) == want, text
        assert Cc * CH >= n and (Cc - 1) * CH < n and 1 <= Cc <= most, text


def test_the_sizes_named_in_the_design_have_their_chunks():
    assert hk_formula(257) == (32, 9) and ge_formula(257) == (33, 8) and alpha_formula(1500)[1] > 1
    assert ge_formula(4097) == (129, 32)


def test_write_sorted_edges_pi_finite(cases, results):
    for text, (_, want), line in picked(cases, results, "raw"):
        assert line == want, text


def test_carved_ranges_are_aligned_disjoint_and_add_up(cases, results):
    for text, (_, spec), line in picked(cases, results, "carve"):
        vals = [int(t) for t in line.split()]
        total, offs, base_mod = vals[0], vals[1:-1], vals[-1]
        sizes = [(s * c + 255) // 256 * 256 for s, c in spec]
        assert base_mod == 0 and all(o % 256 == 0 for o in offs), text
        assert total == sum(sizes), text
        assert offs == [sum(sizes[:i]) for i in range(len(sizes))], text   # in the order named, each behind the last: no overlap
        assert all(o + s * c <= total for o, (s, c) in zip(offs, spec)), text


def test_the_driver_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(sources, results, tmp_path):
    """A program of its own, built with the sanitizers and run once on every case: the same answers, no report."""
    cmd, src = sources
    exe = str(tmp_path / "row_scan_check_san")
    subprocess.check_call(cmd + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    res = subprocess.run([exe], input=results[2], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    assert res.stdout == results[1]
