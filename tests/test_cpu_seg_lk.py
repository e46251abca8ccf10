"""Windowed iterated local search with Lin-Kernighan chains (extension): csrc/seg_lk.hpp as the very source text k_seg_ils compiles,
built with the host compiler (tests/seg_lk_check.cpp), run there against a brute-force statement of the chain and sampled here
against the tests' CPU reference (tests/seg_lk_ref.py); the reference against the properties of the definition on att48 and
kroA100 and against seg_groups_ref.py where the chain kind is off; the new names of the C ABI.  No GPU needed."""
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
import seg_ils_ref as SR
import seg_lk_ref as SL
from helpers import load_instance, random_tour
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsp_optimization_amd", "csrc")
CASES, STRIDE = 4000, 197
N_CHECK, W_CHECK = 11, 9


# ---- the header -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sources():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return [cxx, "-std=c++17", "-ffp-contract=off", "-I", CSRC], os.path.join(ROOT, "tests", "seg_lk_check.cpp")


@pytest.fixture(scope="module")
def results(sources, tmp_path_factory):
    cmd, src = sources
    exe = str(tmp_path_factory.mktemp("seg_lk") / "seg_lk_check")
    subprocess.check_call(cmd + ["-O2", "-o", exe, src])
    return subprocess.run([exe, str(CASES), str(STRIDE)], capture_output=True, text=True, timeout=300)


def test_the_header_gives_the_chains_of_the_definition(results):
    """every slot, both sides and four depths of 4000 windows of nine slots: the program's own brute force over all of them, and
    the reference's chain over the printed sample"""
    assert results.returncode == 0 and "MISMATCH" not in results.stdout, results.stdout[-2000:]
    lines = results.stdout.split("\n")[:-1]
    m = re.fullmatch(r"cases (\d+) chains (\d+) deepest (\d+)", lines[-1])
    assert m and int(m.group(1)) == CASES and int(m.group(2)) == CASES * W_CHECK * 2 * 4 and int(m.group(3)) >= 3
    shown = (CASES + STRIDE - 1) // STRIDE
    assert len(lines) - 1 == shown * (4 + 2 * W_CHECK)
    offered = deep = cut = none = 0
    for c in range(shown):
        blk = lines[c * (4 + 2 * W_CHECK):(c + 1) * (4 + 2 * W_CHECK)]
        assert [b[0] for b in blk[:4]] == list("CSDN")
        K = int(blk[0].split()[2])
        seq = [int(x) for x in blk[1].split()[1:]]
        D = np.array([float(x) for x in blk[2].split()[1:]]).reshape(N_CHECK, N_CHECK)
        nbr = np.array([int(x) for x in blk[3].split()[1:]], dtype=np.int64).reshape(N_CHECK, K)
        assert len(seq) == W_CHECK and (D == D.T).all()
        for line in blk[4:]:
            f = line.split()
            i, s, first, steps, hstar = (int(x) for x in f[1:6])
            ch, iv = SL.side_chain(D, nbr, seq, seq[i], s, 16)
            assert (ch is not None) == bool(first), line
            if ch is None:
                none += 1
                continue
            assert (ch["steps"], ch["hstar"], ch["best"]) == (steps, hstar, float(f[6])), line
            assert ch["j"][1:] == [int(x) for x in f[7:]], line
            offered += hstar >= 1
            deep += hstar >= 2
            cut += steps > hstar >= 1
    assert offered > 0 and deep > 0 and cut > 0 and none == 2 * shown   # slot 8 on side 0 and slot 0 on side 1 have no first edge


def test_the_header_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(sources, results, tmp_path):
    """A program of its own, built with the sanitizers and run once on every case: the same answers, no report."""
    cmd, src = sources
    exe = str(tmp_path / "seg_lk_check_san")
    subprocess.check_call(cmd + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    res = subprocess.run([exe, str(CASES), str(STRIDE)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    assert res.stdout == results.stdout


# ---- the symbol -----------------------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_exported_and_bound():
    from tsp_optimization_amd import engine as E
    from tsp_optimization_amd.build import lib_path
    assert "tsp_dev_seg_ils_lk" in E.EXPORTED and hasattr(E.lib(), "tsp_dev_seg_ils_lk")
    assert hasattr(E.Instance, "seg_ils_lk") and E.NL_LK == SL.NL_LK == 8
    assert E.SEG_LK_MAX_DEPTH == SL.MAX_DEPTH == 16 and E.SEG_LK_DEFAULT_DEPTH == SL.DEFAULT_DEPTH
    fields = [k for k, _ in E.SegIlsLkStats._fields_]
    assert fields[:len(E.SegIlsGroupsStats._fields_)] == [k for k, _ in E.SegIlsGroupsStats._fields_]
    assert fields[len(E.SegIlsGroupsStats._fields_):] == list(SL.LK_COUNTERS)
    assert C.sizeof(E.SegIlsLkStats) == C.sizeof(E.SegIlsGroupsStats) + 40
    hip = open(os.path.join(ROOT, "include", "tsp_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "tsp_host.h")).read()
    assert re.search(r"int tsp_dev_seg_ils_lk\(tsp_dev_inst \*inst, int kinds, int lk_depth, int groups, int B,", hip)
    assert "} tsp_seg_ils_lk_stats;" in hip and "enum { TSP_NL_LK = 8 };" in hip and "#define TSP_SEG_LK_MAX_DEPTH 16" in hip
    assert "#define TSP_SEG_LK_DEFAULT_DEPTH %d" % E.SEG_LK_DEFAULT_DEPTH in hip
    L = C.CDLL(lib_path("libtsp_host.so"))
    for name in ("tsp_host_set_seg_ils_lk", "tsp_host_last_seg_ils_lk_stats"):
        assert name in host and hasattr(L, name), name
    try:
        for bad in (-2, 17, 1000, -100):
            assert L.tsp_host_set_seg_ils_lk(bad) == E.E_ARG
        for good in (0, 1, 16, -1, 8):
            assert L.tsp_host_set_seg_ils_lk(good) == 0
        for bad in (8, 15, 9, 0, 16):                      # the kinds setter keeps refusing the chain kind
            assert L.tsp_host_set_seg_ils_kinds(bad) == E.E_ARG
    finally:
        L.tsp_host_set_seg_ils_lk(0)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

def _inst(name, K=5):
    xy, wt = load_instance(name)
    D = O.dist_matrix(xy, wt, 1)
    return D, NL.knn(D, K)


@pytest.mark.parametrize("name,W", [("att48", 23), ("kroA100", 49)])
def test_every_chain_is_a_window_move_with_the_delta_of_its_reversals(name, W):
    """integer costs: G after h reversals is the cost the tour lost by them, the chain keeps the first prefix of largest G, makes
    no more than D reversals, leaves slots 0 and W - 1 and every successor outside the window, and side 1 is side 0 mirrored"""
    D, nbr = _inst(name)
    n = D.shape[0]
    succ = random_tour(n, np.random.default_rng(n))
    offered = deeper = cut = full = 0
    for depth in (1, 3, 16):
        for it in range(2):
            for seq in SR.windows(succ, 5, 0, it, W):
                before = IR.cost(D, succ)
                for v in seq:
                    mirror, _ = SL.side_chain(D, nbr, seq[::-1], v, 0, depth)
                    for s in (0, 1):
                        ch, iv = SL.side_chain(D, nbr, seq, v, s, depth)
                        i = seq.index(v) if s == 0 else W - 1 - seq.index(v)
                        assert (ch is None) == (i > W - 2)
                        if s == 1:
                            assert (ch is None) == (mirror is None)
                            assert ch is None or all(ch[k] == mirror[k] for k in ("steps", "hstar", "best", "e", "y", "p", "j"))
                        if ch is None:
                            continue
                        assert ch["steps"] <= depth and ch["hstar"] <= ch["steps"]
                        full += ch["steps"] == depth
                        path = seq if s == 0 else seq[::-1]
                        gains = []
                        for h in range(1, ch["steps"] + 1):
                            assert i + 3 <= ch["j"][h] <= W - 1
                            step = [(i + 1, ch["j"][q] - 1) for q in range(1, h + 1)]
                            if s == 1:
                                step = [(W - 1 - hi, W - 1 - lo) for lo, hi in step]
                            new = SL.apply_intervals(seq, step)
                            after = SR.set_path(succ, new)
                            assert O.is_tour(after) and new[0] == seq[0] and new[-1] == seq[-1] and sorted(new) == sorted(seq)
                            assert set(np.flatnonzero(after != succ).tolist()) <= set(seq[:-1])
                            assert before - IR.cost(D, after) == ch["G"][h]
                            assert path[i] == ch["t1"] and len({ch["e"][h], ch["y"][h], ch["p"][h], ch["t1"]}) >= 3
                            gains.append(ch["G"][h])
                            if h == ch["hstar"]:
                                assert step == iv and all(1 <= lo < hi <= W - 2 for lo, hi in iv)
                        top = max(gains + [0.0])
                        assert ch["best"] == top and ch["hstar"] == (gains.index(top) + 1 if top > 0 else 0)
                        for h in range(1, ch["steps"] + 1):     # no y was an e or a y of a step before
                            assert ch["y"][h] not in ch["e"][1:h] + ch["y"][1:h] and ch["y"][h] != ch["e"][h]
                        offered += ch["hstar"] >= 1
                        deeper += ch["hstar"] >= 2
                        cut += ch["steps"] > ch["hstar"] >= 1
    assert offered > 0 and deeper > 0 and cut > 0 and full > 0


def test_without_the_chain_kind_the_reference_is_that_of_the_groups():
    D, nbr = _inst("att48")
    start = random_tour(48, np.random.default_rng(48))
    moved = 0
    for kinds in (3, 4, 7):
        for G in (1, 3):
            sg, cg, stg = SG.run(D, start, nbr, kinds, 5, 0, 2, G, 12, 8, 2)
            s, c, st = SL.run(D, start, nbr, kinds, 5, 0, 2, 6, G, 12, 8, 2)
            assert (s == sg).all() and np.float64(c).tobytes() == np.float64(cg).tobytes()
            assert all(st[k] == stg[k] for k in SG.COUNTERS + ("start_cost",))
            assert st["lk_depth"] == 6 and all(st[k] == 0 for k in SL.LK_COUNTERS[1:])
            moved += st["moves"]
    assert moved > 0


@pytest.mark.parametrize("name,W,S,T", [("ulysses22", 11, 8, 2), ("att48", 23, 8, 2), ("kroA100", 49, 12, 3)])
def test_runs_of_the_reference_apply_chains_of_several_depths(name, W, S, T):
    """KNN-5 lists, D = 6, three iterations, seed 5: every set of kinds with the chain kind applies chains, some deeper than one
    reversal; the counters add up and the tour gets cheaper by what the commits gained"""
    D, nbr = _inst(name)
    n = D.shape[0]
    start = random_tour(n, np.random.default_rng(n))
    for kinds in (15, 8, 9):
        log = []
        s, cost, st = SL.run(D, start, nbr, kinds, 5, 0, 3, 6, 1, W, S, T, log=log)
        assert O.is_tour(s) and cost == IR.cost(D, s) < st["start_cost"]
        assert st["moves"] == st["moves_2opt"] + st["moves_oropt"] + st["moves_3opt"] + st["moves_lk"]
        applied = [r for r in log if r[0] == "chain"]
        assert len(applied) == st["moves_lk"] > 0 and sum(r[3] for r in applied) == st["lk_flips"] > st["moves_lk"]
        assert all(1 <= r[3] <= 6 and len(r[4]) == r[3] for r in applied)
        assert st["lk_steps"] >= st["lk_flips"] and st["lk_chains"] <= 2 * st["active_nodes"]
        assert sum(r[1] for r in log if r[0] == "decision") == st["active_nodes"]
        assert st["lk_depth"] == 6 and st["groups"] == 1
        if kinds == 8:
            assert st["moves"] == st["moves_lk"] and st["reversed"] == 0
    assert SL.resolve_depth(0) == SL.resolve_depth(-3) == SL.DEFAULT_DEPTH and SL.resolve_depth(16) == 16
    assert SL.resolve_depth(17) is None
