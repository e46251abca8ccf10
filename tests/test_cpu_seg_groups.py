"""Windowed iterated local search with groups (extension): csrc/seg_groups.hpp as the very source text k_seg_commit compiles, built
with the host compiler (tests/seg_groups_check.cpp), enumerated there against a brute-force statement of the rule and sampled here
against the tests' CPU reference (tests/seg_groups_ref.py); the reference against seg_ils3_ref.py where G = 1 and against the
properties of the definition; the new names of the C ABI.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ils_ref as IR
import nl_opt_ref as NL
import seg_groups_ref as SG
import seg_ils3_ref as S3
import seg_ils_ref as SR
from helpers import load_instance, random_tour
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsp_optimization_amd", "csrc")
W_CHECK, STRIDE = 9, 997


# ---- the header -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sources():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return [cxx, "-std=c++17", "-ffp-contract=off", "-I", CSRC], os.path.join(ROOT, "tests", "seg_groups_check.cpp")


@pytest.fixture(scope="module")
def results(sources, tmp_path_factory):
    cmd, src = sources
    exe = str(tmp_path_factory.mktemp("seg_groups") / "seg_groups_check")
    subprocess.check_call(cmd + ["-O2", "-o", exe, src])
    return subprocess.run([exe, str(W_CHECK), str(STRIDE)], capture_output=True, text=True, timeout=300)


def test_the_header_gives_the_commits_of_the_definition(results):
    """every placement of up to 4 offers in a window of 9 slots, gains -1 and -2: the program's own brute force over all of them,
    and the reference's rule over the printed sample"""
    assert results.returncode == 0 and "MISMATCH" not in results.stdout, results.stdout[-2000:]
    lines = results.stdout.split("\n")[:-1]
    states = 1 + 2 * (W_CHECK - 2) * (W_CHECK - 1) // 2            # no offer, or an interval 1 <= lo <= hi <= W - 2 with one of two gains
    total = sum(states ** G for G in range(1, 5))
    assert lines[-1] == "cases %d" % total
    assert len(lines) - 1 == (total + STRIDE - 1) // STRIDE
    sizes, losers, several, ties = set(), 0, 0, 0
    for line in lines[:-1]:
        left, right = line.split(":")
        f = left.split()
        G = int(f[0])
        got = [int(x) for x in right.split()]
        assert len(f) == 1 + 4 * G and len(got) == G, line
        offers = []
        for g in range(G):
            offer, lo, hi, gain = int(f[1 + 4 * g]), int(f[2 + 4 * g]), int(f[3 + 4 * g]), float(f[4 + 4 * g])
            if offer:
                assert 1 <= lo <= hi <= W_CHECK - 2
                offers.append((gain, g, lo, hi))
        keep = SG.committed(offers)
        assert got == [int(g in keep) for g in range(G)], line
        sizes.add(G)
        losers += len(offers) > len(keep)
        several += len(keep) >= 2
        ties += len({o[0] for o in offers}) < len(offers)
    assert sizes == {1, 2, 3, 4} and losers > 0 and several > 0 and ties > 0


def test_the_header_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(sources, results, tmp_path):
    """A program of its own, built with the sanitizers and run once on every case: the same answers, no report."""
    cmd, src = sources
    exe = str(tmp_path / "seg_groups_check_san")
    subprocess.check_call(cmd + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    res = subprocess.run([exe, str(W_CHECK), str(STRIDE)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    assert res.stdout == results.stdout


def test_the_rule_on_hand_made_offers():
    # (gain, g, lo, hi); the changed edges are those of slots lo - 1 .. hi
    assert SG.committed([]) == set()
    assert SG.committed([(-1.0, 0, 1, 3), (-5.0, 1, 5, 7)]) == {0, 1}            # edges 0 .. 3 and 4 .. 7: apart
    assert SG.committed([(-1.0, 0, 1, 3), (-5.0, 1, 4, 7)]) == {1}               # edges 0 .. 3 and 3 .. 7 share edge 3
    assert SG.committed([(-5.0, 0, 1, 3), (-5.0, 1, 4, 7)]) == {0}               # equal gains: the lower group
    # 1 loses to 0, 2 loses to 1 and to nobody that commits: it still does not commit
    assert SG.committed([(-9.0, 0, 1, 2), (-8.0, 1, 3, 4), (-7.0, 2, 5, 6)]) == {0}
    assert SG.committed([(-9.0, 0, 1, 2), (-8.0, 1, 4, 4), (-7.0, 2, 6, 6)]) == {0, 1, 2}
    assert SG.default_groups(10000, 1024) == 64 and SG.default_groups(100003, 1024) == 10 and SG.default_groups(100003, 2048) == 21
    assert SG.default_groups(100003, 9) == 1 and SG.default_groups(10, 9) == 64


# ---- the symbol -----------------------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_exported_and_bound():
    from tsp_optimization_amd import engine as E
    from tsp_optimization_amd.build import lib_path
    assert "tsp_dev_seg_ils_groups" in E.EXPORTED and hasattr(E.lib(), "tsp_dev_seg_ils_groups")
    assert hasattr(E.Instance, "seg_ils_groups") and E.SEG_ILS_MAX_GROUPS == SG.MAX_GROUPS == 64
    fields = [k for k, _ in E.SegIlsGroupsStats._fields_]
    assert fields[:len(E.SegIls3Stats._fields_)] == [k for k, _ in E.SegIls3Stats._fields_]
    assert fields[len(E.SegIls3Stats._fields_):] == ["groups", "offers", "commits"]
    assert C.sizeof(E.SegIlsGroupsStats) == C.sizeof(E.SegIls3Stats) + 24
    hip = open(os.path.join(ROOT, "include", "tsp_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "tsp_host.h")).read()
    assert re.search(r"int tsp_dev_seg_ils_groups\(tsp_dev_inst \*inst, int kinds, int groups, int B,", hip)
    assert "} tsp_seg_ils_groups_stats;" in hip and "#define TSP_SEG_ILS_MAX_GROUPS 64" in hip
    L = C.CDLL(lib_path("libtsp_host.so"))
    for name in ("tsp_host_set_seg_ils_groups", "tsp_host_last_seg_ils_groups_stats"):
        assert name in host and hasattr(L, name), name
    try:
        for bad in (-1, 65, 1000):
            assert L.tsp_host_set_seg_ils_groups(bad) == E.E_ARG
        for good in (0, 2, 64, 1):
            assert L.tsp_host_set_seg_ils_groups(good) == 0
    finally:
        L.tsp_host_set_seg_ils_groups(1)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

def test_with_one_group_the_reference_is_that_of_seg_ils3():
    xy, wt = load_instance("att48")
    D = O.dist_matrix(xy, wt, 1)
    nbr = NL.knn(D, 5)
    start = random_tour(48, np.random.default_rng(48))
    moved = 0
    for kinds in (3, 4, 7):
        s3, c3, st3 = S3.run(D, start, nbr, kinds, 5, 0, 3, 12, 8, 3)
        s, c, st = SG.run(D, start, nbr, kinds, 5, 0, 3, 1, 12, 8, 3)
        assert (s == s3).all() and np.float64(c).tobytes() == np.float64(c3).tobytes()
        assert all(st[k] == st3[k] for k in S3.COUNTERS + ("start_cost",))
        assert st["groups"] == 1 and 0 < st["offers"] == st["commits"] <= st["accepted"]
        moved += st["moves"]
    assert moved > 0


def test_every_commit_leaves_a_tour_that_is_strictly_cheaper():
    """kroA100 (integer costs), two windows of 49, six groups, no repair: a window's commits together gain the sum of their gains"""
    xy, wt = load_instance("kroA100")
    D = O.dist_matrix(xy, wt, 1)
    nbr = NL.knn(D, 5)
    succ = random_tour(100, np.random.default_rng(100))
    G, T, W, S = 6, 1, 49, 8
    c = SG.new_counters()
    several = lost = 0
    for it in range(2):
        for w, seq in enumerate(SR.windows(succ, 5, 0, it, W)):
            offers, fins = SG.window_groups(D, succ, nbr, 7, seq, 5, 0, it, w, G, T, S, 0, c)
            keep = SG.committed(offers)
            assert bool(keep) == bool(offers)
            if offers:
                assert min(offers)[1] in keep                          # the best offer of a window commits
            new = list(seq)
            for gain, g, lo, hi in offers:
                if g in keep:
                    new[lo:hi + 1] = fins[g][lo:hi + 1]
            after = SR.set_path(succ, new)
            assert O.is_tour(after) and new[0] == seq[0] and new[-1] == seq[-1] and sorted(new) == sorted(seq)
            assert set(np.flatnonzero(after != succ).tolist()) <= set(seq[1:-1]) | {seq[0]}   # no successor outside the window
            gained = sum(o[0] for o in offers if o[1] in keep)
            assert IR.cost(D, after) - IR.cost(D, succ) == gained and (gained < 0) == bool(keep)
            several += len(keep) >= 2
            lost += len(offers) > len(keep)
            succ = after
    assert several > 0 and lost > 0
    ref, cost, st = SG.run(D, random_tour(100, np.random.default_rng(100)), nbr, 7, 5, 0, 2, G, W, S, T, max_moves=0)
    assert (ref == succ).all() and cost == IR.cost(D, succ) < st["start_cost"]
    assert st["trials"] == 2 * 2 * G * T == c["trials"] and st["accepted"] == c["accepted"] == st["offers"] > st["commits"] > 0
