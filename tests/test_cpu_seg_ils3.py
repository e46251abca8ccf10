"""Windowed iterated local search with the 3-opt kind (extension): csrc/seg_move3.hpp as the very source text the kernel compiles,
built with the host compiler (tests/seg_move3_check.cpp) and compared with nl3_opt_ref.apply_three_opt; the tests' CPU reference
(tests/seg_ils3_ref.py) against the definition in include/tsp_hip.h and against seg_ils_ref.py where the third kind is off; the
smallest shapes reach every (r, type) of the relabel table; the new names of the C ABI.  No GPU needed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ils_ref as IR
import nl3_opt_ref as N3
import nl_opt_ref as NL
import seg_ils3_ref as S3
import seg_ils_ref as SR
from helpers import load_instance, rand_instance, random_tour
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsp_optimization_amd", "csrc")
W_CHECK = 9


# ---- the header -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sources():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return [cxx, "-std=c++17", "-ffp-contract=off", "-I", CSRC], os.path.join(ROOT, "tests", "seg_move3_check.cpp")


@pytest.fixture(scope="module")
def results(sources, tmp_path_factory):
    cmd, src = sources
    exe = str(tmp_path_factory.mktemp("seg_move3") / "seg_move3_check")
    subprocess.check_call(cmd + ["-O2", "-o", exe, src])
    res = subprocess.run([exe, str(W_CHECK)], capture_output=True, text=True, timeout=300)
    return res


def _definition(W, i, j, k, r, T):
    """the window after the move (a, b, c, T), a at the r-th of the slots i < j < k, on the tour 0 .. W + 1 whose window is 0 .. W - 1:
    nl3_opt_ref's apply, the tour turned back when the outside came out reversed"""
    n = W + 2
    succ = np.roll(np.arange(n, dtype=np.int32), -1)
    t = (i, j, k)
    new = N3.apply_three_opt(succ, t[r], t[(r + 1) % 3], t[(r + 2) % 3], T)
    if int(new[n - 1]) != 0:
        back = np.empty(n, dtype=np.int32)
        back[new] = np.arange(n, dtype=np.int32)
        new = back
    assert int(new[W - 1]) == W and int(new[W]) == W + 1 and int(new[W + 1]) == 0
    return SR.walk(new, 0, W)


def test_the_header_gives_the_permutation_of_the_definition(results):
    assert results.returncode == 0 and "MISMATCH" not in results.stdout, results.stdout[-2000:]
    lines = results.stdout.split("\n")[:-1]
    W = W_CHECK
    cases = [(i, j, k, r, T) for i in range(W - 1) for j in range(i + 1, W - 1) for k in range(j + 1, W - 1) for r in range(3)
             for T in range(4)]
    assert len(lines) == len(cases) == 56 * 12
    forms, one_node = set(), 0
    for (i, j, k, r, T), line in zip(cases, lines):
        f = [int(x) for x in line.split()]
        assert f[:5] == [i, j, k, r, T], line
        assert f[5] == (0 if T == 0 else 1 + (T - 1 + 2 * r) % 3), line
        want = _definition(W, i, j, k, r, T)
        assert want[:i + 1] == list(range(i + 1)) and want[k + 1:] == list(range(k + 1, W)), line
        assert f[6:] == want[i + 1:k + 1], (line, want)
        forms.add((r, T, f[5]))
        one_node += j == i + 1 or k == j + 1
    assert len(forms) == 12 and one_node > 0


def test_the_header_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(sources, results, tmp_path):
    """A program of its own, built with the sanitizers and run once on every case: the same answers, no report."""
    cmd, src = sources
    exe = str(tmp_path / "seg_move3_check_san")
    subprocess.check_call(cmd + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    res = subprocess.run([exe, str(W_CHECK)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    assert res.stdout == results.stdout


# ---- the symbol -----------------------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_exported_and_bound():
    from tsp_optimization_amd import engine as E
    assert "tsp_dev_seg_ils3" in E.EXPORTED and hasattr(E.lib(), "tsp_dev_seg_ils3")
    assert hasattr(E.Instance, "seg_ils3") and "tsp_dev_seg_ils" in E.EXPORTED
    fields = [k for k, _ in E.SegIls3Stats._fields_]
    assert fields[:len(E.SegIlsStats._fields_)] == [k for k, _ in E.SegIlsStats._fields_]
    assert fields[len(E.SegIlsStats._fields_):] == ["moves_3opt", "moves_by_type"]
    hip = open(os.path.join(ROOT, "include", "tsp_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "tsp_host.h")).read()
    assert re.search(r"int tsp_dev_seg_ils3\(tsp_dev_inst \*inst, int kinds, int B,", hip) and "} tsp_seg_ils3_stats;" in hip
    for name in ("tsp_host_set_seg_ils_kinds", "tsp_host_last_seg_ils3_stats"):
        assert name in host, name


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

def test_without_the_third_kind_the_reference_is_the_older_one():
    xy, wt = load_instance("att48")
    D = O.dist_matrix(xy, wt, 1)
    nbr = NL.knn(D, 5)
    start = random_tour(48, np.random.default_rng(48))
    for kinds in (1, 2, 3):
        s, c, st = SR.run(D, start, nbr, kinds, 5, 0, 3, 12, 8, 3)
        s3, c3, st3 = S3.run(D, start, nbr, kinds, 5, 0, 3, 12, 8, 3)
        assert (s3 == s).all() and np.float64(c3).tobytes() == np.float64(c).tobytes()
        assert all(st3[k] == st[k] for k in SR.COUNTERS + ("start_cost",))
        assert st3["moves_3opt"] == 0 and st3["moves_by_type"] == [0, 0, 0, 0] and st["moves"] > 0


def _tiny(n, K, q, kinds, log=None):
    xy = rand_instance(n, seed=n, hi=1000)
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    start = random_tour(n, np.random.default_rng(10 * n + q))
    return D, start, S3.run(D, start, NL.knn(D, K), kinds, q, 0, 6, 9, 0, 2, log=log)


def test_the_smallest_shapes_apply_every_case_of_the_relabel_table():
    seen = {}
    for n in (10, 11):
        for K in (n - 1, 3):
            acc = 0
            for q in range(4):
                log = []
                D, start, (s, c, st) = _tiny(n, K, q, 4, log)
                assert O.is_tour(s) and c == IR.cost(D, s) <= st["start_cost"]
                assert st["moves"] == st["moves_3opt"] == sum(st["moves_by_type"]) and st["reversed"] == st["moves_2opt"] == 0
                assert st["trials"] == 12 == len(log)
                for r in log:
                    for rt in r["three"]:
                        seen[rt] = seen.get(rt, 0) + 1
                acc += st["accepted"]
            assert 0 < acc < 48, (n, K, acc)
    assert sorted(seen) == [(r, T) for r in range(3) for T in range(4)], seen


def test_a_window_three_opt_move_permutes_the_interior_of_its_window():
    xy, wt = load_instance("kroA100")
    D = O.dist_matrix(xy, wt, 1)
    n = len(xy)
    nbr = NL.knn(D, 5)
    start = random_tour(n, np.random.default_rng(n))
    cases, through_outside = set(), 0
    for seq in SR.windows(start, 5, 0, 0, 30):
        inside = np.zeros(n, dtype=bool)
        inside[seq] = True
        out = int(start[seq[-1]])
        own, delta, kind, key = S3.window_candidates(D, start, nbr, 4, inside, seq)
        assert len(own) > 0 and (kind == 2).all() and (delta < 0).all() and inside[own].all()
        for dl, k in set(zip(delta.tolist(), key.tolist())):
            d = (dl, 2, k)
            c = S3.new_counters()
            new = S3.apply_window_move(start, d, seq, c)
            assert O.is_tour(new)
            changed = np.flatnonzero(new != start)
            assert inside[changed].all() and seq[-1] not in changed
            after = SR.walk(new, seq[0], 30)
            assert after[0] == seq[0] and after[-1] == seq[-1] and int(new[seq[-1]]) == out and sorted(after) == sorted(seq)
            assert IR.cost(D, new) - IR.cost(D, start) == dl            # integer metrics: the delta is the tour's
            assert SR.window_cost(D, after) - SR.window_cost(D, seq) == dl
            r, T = S3.relabel(seq, start, d)
            assert c["moves"] == c["moves_3opt"] == 1 and c["moves_by_type"][T] == 1 and c["reversed"] == 0
            cases.add((r, T))
            through_outside += r != 0
    assert len(cases) == 12 and through_outside > 0
    # a tail at slot W - 1 or outside the window is no window move
    seq = SR.walk(start, 7, 30)
    slot = SR._slots(n, seq)
    a, b, c = sorted((seq[3], seq[10], seq[28]))
    assert S3.is_window_move(start, slot, 30, 2, N3.key(a, b, c, 1, n))
    a, b, c = sorted((seq[3], seq[10], seq[29]))
    assert not S3.is_window_move(start, slot, 30, 2, N3.key(a, b, c, 1, n))
    a, b, c = sorted((seq[3], seq[10], int(start[seq[29]])))
    assert not S3.is_window_move(start, slot, 30, 2, N3.key(a, b, c, 1, n))
