"""CPU: the exhaustive sweep's records by permutation (csrc/exh_arith.hpp: exh_mirror, exh_perm, exh_perm_rec), as the very
source text k_move_pos's hot path compiles, built with the host compiler (tests/exh_permute_check.cpp).

A 2-opt move only permutes positions.  For the new position k in [0, n], a = mirror((k - 1) mod n) and b = mirror(k mod n) are
old positions; the new record takes -2x, -2y, the norm and the node id from old record b, and its `eprev` is
  * 0 at position 0;
  * the old eprev at unwrapped index a + 1 when b = a + 1 (mod n)   (forward: outside the reversed segment);
  * the old eprev at unwrapped index b + 1 when a = b + 1 (mod n)   (backward: inside it, the edge walked the other way);
  * exh_dist of the two old records otherwise: a cut point, two per move.
Unwrapped index n is old record n's eprev, the closing edge (position n repeats position 0).  Pads are copied.

The check: for every move, records permuted from the old tour's records equal, field for field and bit for bit, the records built
from scratch from the reversed tour (reversal by swaps, edge lengths from an integer square root: nothing of the rule in them)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsp_optimization_amd", "csrc")

SMALL = tuple(range(5, 13))
LARGE = (255, 256, 257)
MODES = (0, 1, 2)   # EXH_NINT, EXH_CEIL, EXH_ATT
COLS = ("bad", "zero", "fwd", "bwd", "wrap_fwd", "wrap_bwd", "cut_lo", "cut_hi", "pads")
PADS = 9            # kPads of the driver


def _moves(n):
    """Every ordered (pa, pb) with 2 <= (pb - pa) mod n <= n - 1; at the large n a seeded sample of 2 000 of them plus all
    with pa or pb in {0, 1, n - 2, n - 1}."""
    every = [(pa, pb) for pa in range(n) for pb in range(n) if 2 <= (pb - pa) % n <= n - 1]
    if n in SMALL:
        return every
    edge = {0, 1, n - 2, n - 1}
    rng = np.random.default_rng(1000 + n)
    pick = rng.choice(len(every), size=2000, replace=False)
    return sorted({every[i] for i in pick} | {m for m in every if m[0] in edge or m[1] in edge})


@pytest.fixture(scope="module")
def sources():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # plain C++17, nothing of HIP: exh_arith.hpp as the kernels include it; -ffp-contract=off as in csrc/Makefile
    return [cxx, "-std=c++17", "-ffp-contract=off", "-I", CSRC], os.path.join(ROOT, "tests", "exh_permute_check.cpp")


@pytest.fixture(scope="module")
def case_list():
    out = []
    for n in SMALL + LARGE:
        for mode in MODES:
            # wide coordinates (edge lengths up to 1.4e6) and narrow ones (equal nodes, zero-length edges, many equal lengths)
            for hi, seed in ((1000000, 7 * n + mode), (12, 11 * n + mode)):
                if n in LARGE and hi == 12:
                    continue
                for pa, pb in _moves(n):
                    out.append(dict(mode=mode, n=n, pa=pa, pb=pb, hi=hi, seed=seed))
    return out


def _text(cases):
    return "".join("%d %d %d %d %d %d\n" % (c["mode"], c["n"], c["pa"], c["pb"], c["hi"], c["seed"]) for c in cases)


@pytest.fixture(scope="module")
def results(sources, case_list, tmp_path_factory):
    """One run of the driver for every case: an (cases, 9) table of its answers, and its output as text."""
    cmd, src = sources
    exe = str(tmp_path_factory.mktemp("exh_permute") / "exh_permute_check")
    subprocess.check_call(cmd + ["-O2", "-o", exe, src])
    res = subprocess.run([exe], input=_text(case_list), check=True, capture_output=True, text=True, timeout=300)
    tab = np.array([line.split() for line in res.stdout.strip().splitlines()], dtype=np.int64)
    assert tab.shape == (len(case_list), len(COLS))
    return tab, res.stdout


def _col(tab, name):
    return tab[:, COLS.index(name)]


def test_the_cases_are_the_sizes_modes_and_moves_asked_for(case_list):
    for n in SMALL:
        for mode in MODES:
            got = {(c["pa"], c["pb"]) for c in case_list if c["n"] == n and c["mode"] == mode}
            assert len(got) == n * (n - 2)   # every ordered pair but pb = pa and pb = pa + 1
    for n in LARGE:
        for mode in MODES:
            got = {(c["pa"], c["pb"]) for c in case_list if c["n"] == n and c["mode"] == mode}
            assert len(got) >= 2000
            for e in (0, 1, n - 2, n - 1):
                assert sum(1 for pa, _ in got if pa == e) == n - 2 and sum(1 for _, pb in got if pb == e) == n - 2
    assert any(c["pa"] > c["pb"] for c in case_list)   # wrapping segments


def test_permuted_records_equal_the_records_built_from_scratch_bit_for_bit(case_list, results):
    tab, _ = results
    bad = np.flatnonzero(_col(tab, "bad"))
    assert bad.size == 0, [case_list[i] for i in bad[:10]]


def test_every_position_is_served_by_exactly_one_rule(case_list, results):
    tab, _ = results
    n = np.array([c["n"] for c in case_list])
    L = np.array([(c["pb"] - c["pa"]) % c["n"] for c in case_list])
    assert (_col(tab, "zero") == 1).all() and (_col(tab, "pads") == PADS - 1).all()
    rules = sum(_col(tab, k) for k in ("fwd", "bwd", "wrap_fwd", "wrap_bwd", "cut_lo", "cut_hi"))
    assert (rules == n).all()   # positions 1 .. n
    # a reversal of L positions walks L - 1 old edges backwards; the two edges at its ends are new -- unless L = n - 1, where
    # the segment's two ends were neighbours already and the rule finds their old edge
    cuts = _col(tab, "cut_lo") + _col(tab, "cut_hi")
    assert (cuts[L < n - 1] == 2).all() and (cuts[L == n - 1] == 0).all()
    back = _col(tab, "bwd") + _col(tab, "wrap_bwd")
    assert (back[L < n - 1] == L[L < n - 1] - 1).all()


def test_the_cases_hit_both_rules_both_wrap_indices_and_both_cut_points(case_list, results):
    tab, _ = results
    for n in SMALL + LARGE:
        for mode in MODES:
            rows = np.array([c["n"] == n and c["mode"] == mode for c in case_list])
            for k in ("fwd", "bwd", "wrap_fwd", "wrap_bwd", "cut_lo", "cut_hi"):
                assert _col(tab, k)[rows].sum() > 0, (n, mode, k)
    # the closing edge is reached from either side, and a cut point falls on position n (new position 0 has no edge before it)
    assert ((_col(tab, "wrap_fwd") == 1) & (_col(tab, "wrap_bwd") == 0)).any()
    assert ((_col(tab, "wrap_bwd") == 1) & (_col(tab, "wrap_fwd") == 0)).any()
    pa0 = np.array([(c["pa"] + 1) % c["n"] == 0 for c in case_list])
    assert (_col(tab, "cut_lo")[pa0 & (_col(tab, "cut_lo") + _col(tab, "cut_hi") == 2)] == 1).all() and pa0.any()


def test_the_driver_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(sources, case_list, results, tmp_path):
    """A program of its own, built with the sanitizers and run once on every case: the same answers, no report."""
    cmd, src = sources
    exe = str(tmp_path / "exh_permute_check_san")
    subprocess.check_call(cmd + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    res = subprocess.run([exe], input=_text(case_list), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    assert res.stdout == results[1]
