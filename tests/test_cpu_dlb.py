"""Don't-look bits (extension): the tests' CPU reference (tests/dlb_ref.py) against the definition in include/tsp_hip.h -- the
candidates of all nodes are the list neighbourhood, a TSP_DLB_CLOSE result is a local optimum of it, a descent behind a kick
looks at a handful of nodes, the recorded chains of tests/golden/dlb_runs.json -- and the new names of the C ABI.  No GPU
needed."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import dlb_ref as DR
import ils_ref as IR
import nl3_opt_ref as N3
import nl_opt_ref as NL
from helpers import GOLDEN, golden, load_instance, random_tour
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(name, K, integer_cost=1):
    xy, wt = load_instance(name)
    D = O.dist_matrix(xy, wt, integer_cost)
    return xy, wt, D, NL.knn(D, K)


@pytest.mark.parametrize("name,K", [("att48", 5), ("kroA100", 5), ("burma14", 13), ("ulysses22", 3)])
def test_with_every_node_active_a_decision_is_the_list_neighbourhoods(name, K):
    xy, wt, D, nbr = _case(name, K)
    n = len(xy)
    rng = np.random.default_rng(n)
    all_on = np.ones(n, dtype=bool)
    for start in (random_tour(n, rng), O.greedy(xy, wt)[1]):
        succ = np.array(start, dtype=np.int32)
        for step in range(6):
            for kinds in (7, 3, 4, 1, 2):
                d, hit = DR.decide(D, succ, nbr, kinds, all_on)
                assert d == N3.decide_sparse(D, succ, nbr, kinds), (name, step, kinds)
                assert (d is None) == (not hit.any())
            d, _ = DR.decide(D, succ, nbr, 7, all_on)
            if d is None:
                break
            succ = N3.apply_decision(succ, d, N3.new_counters())


def test_small_instances_have_the_same_first_decision():
    xy, wt = load_instance("att48")
    for n in (5, 6, 7, 8, 9):
        D = O.dist_matrix(xy[:n], wt, 1)
        nbr = NL.knn(D, n - 1)
        for q in range(4):
            succ = random_tour(n, np.random.default_rng(10 * n + q))
            d, _ = DR.decide(D, succ, nbr, 7, np.ones(n, dtype=bool))
            assert d == N3.decide_sparse(D, succ, nbr, 7) == N3.decide(D, succ, nbr, 7), (n, q)


def test_candidates_of_a_subset_are_a_subset_and_the_owners_partition_them():
    xy, wt, D, nbr = _case("att48", 5)
    n = len(xy)
    succ = random_tour(n, np.random.default_rng(2))
    own, delta, kind, key = DR.candidates(D, succ, nbr, 7, np.ones(n, dtype=bool))
    everything = set(zip(own.tolist(), delta.tolist(), kind.tolist(), key.tolist()))
    A = np.zeros(n, dtype=bool)
    A[[3, 17, 40]] = True
    o2, d2, k2, y2 = DR.candidates(D, succ, nbr, 7, A)
    part = set(zip(o2.tolist(), d2.tolist(), k2.tolist(), y2.tolist()))
    assert part and part == {c for c in everything if c[0] in (3, 17, 40)}
    assert DR.decide(D, succ, nbr, 7, np.zeros(n, dtype=bool))[0] is None


@pytest.mark.parametrize("name", ["att48", "kroA100"])
def test_a_closed_descent_ends_in_a_local_optimum_of_the_whole_neighbourhood(name):
    xy, wt, D, nbr = _case(name, 5)
    n = len(xy)
    start = random_tour(n, np.random.default_rng(7))
    for kinds in (7, 3):
        s2, c2, A2 = DR.descent(D, start, nbr, kinds, DR.CLOSE)
        assert N3.decide_sparse(D, s2, nbr, kinds) is None and N3.decide(D, s2, nbr, kinds) is None
        assert A2.all() and c2["closing_scans"] >= 1 and c2["decisions"] == c2["moves"] + c2["closing_scans"] + 1
        s1, c1, A1 = DR.descent(D, start, nbr, kinds, DR.ON)
        assert c1["closing_scans"] == 0 and c1["decisions"] == c1["moves"] + 1
        assert c1["active_nodes"] < n * c1["decisions"]
        # until the first decision without a move the two modes are one trajectory
        t1, t2 = [], []
        DR.descent(D, start, nbr, kinds, DR.ON, trace=t1)
        DR.descent(D, start, nbr, kinds, DR.CLOSE, trace=t2)
        assert t2[:len(t1)] == t1
        # an empty set: one decision and the end, or the full set at once
        s, c, _ = DR.descent(D, start, nbr, kinds, DR.ON, active=np.zeros(n))
        assert (s == start).all() and c["decisions"] == 1 and c["moves"] == 0 and c["active_nodes"] == 0
        s, c, _ = DR.descent(D, start, nbr, kinds, DR.CLOSE, active=np.zeros(n))
        assert (s == s2).all() and c["closing_scans"] == c2["closing_scans"] + 1 and c["decisions"] == c2["decisions"] + 1
    s0, c0, _ = DR.descent(D, start, nbr, 7, DR.OFF)
    ref, cr = N3.descent(D, start, nbr, 7)
    assert (s0 == ref).all() and all(c0[k] == cr[k] for k in IR.NL_COUNTERS) and c0["active_nodes"] == 0


def test_after_a_kick_from_a_local_optimum_only_a_few_nodes_are_looked_at():
    xy, wt, D, nbr = _case("kroA100", 5)
    n = len(xy)
    opt = N3.descent(D, O.greedy(xy, wt)[1], nbr, 7)[0]
    moved = 0
    for it in range(6):
        A = DR.kick_nodes(opt, 5, 0, it, 30)
        kicked = IR.kick(opt, 5, 0, it, 30)
        assert 4 <= A.sum() <= 8 and set(np.flatnonzero(kicked != opt)) <= set(np.flatnonzero(A))
        trace = []
        s, c, _ = DR.descent(D, kicked, nbr, 7, DR.ON, active=A, trace=trace)
        assert trace[0][1] == A.sum() and all(na < n for _, na in trace)
        assert c["active_nodes"] == sum(na for _, na in trace) < n * c["decisions"]
        assert O.is_tour(s) and IR.cost(D, s) <= IR.cost(D, kicked)
        moved += c["moves"]
    assert moved > 0


def test_chain_counts_and_mode_off():
    xy, wt, D, nbr = _case("att48", 5)
    start = random_tour(len(xy), np.random.default_rng(7))
    s0, c0, st0 = DR.chain(D, start, nbr, 7, 8, 0, 10, 0, mode=DR.OFF)
    s, c, st = IR.chain(D, start, nbr, 7, 8, 0, 10, 0)
    assert (s0 == s).all() and c0 == c and all(st0[k] == st[k] for k in st) and st0["active_nodes"] == 0
    for mode in (DR.ON, DR.CLOSE):
        s1, c1, st1 = DR.chain(D, start, nbr, 7, 8, 0, 10, 0, mode=mode)
        assert O.is_tour(s1) and c1 == IR.cost(D, s1) == O.succ_cost(xy, wt, s1) <= st1["start_cost"]
        assert st1["iterations"] == 10 and st1["active_nodes"] < len(xy) * st1["decisions"]
        assert (st1["closing_scans"] > 0) == (mode == DR.CLOSE)
        if mode == DR.CLOSE:
            assert N3.decide_sparse(D, s1, nbr, 7) is None


def test_reference_reproduces_the_recorded_chains():
    rec = golden("dlb_runs.json")["runs"]
    sys.path.insert(0, GOLDEN)
    import make_golden_dlb as G
    assert [(r["name"], r["K"], r["seed"], r["iterations"], r["span"], r["mode"]) for r in rec] == G.RUNS
    r = rec[0]                                   # one of the two: each takes a few seconds
    xy, wt = load_instance(r["name"])
    D = O.dist_matrix(xy, wt, 1)
    succ, cost, st = DR.chain(D, O.greedy(xy, wt)[1], NL.knn(D, r["K"]), 7, r["seed"], 0, r["iterations"], r["span"], mode=r["mode"])
    assert (succ == np.array(r["succ"])).all() and cost == r["cost"] and st == r["stats"]
    for r in rec:
        assert r["cost"] <= r["stats"]["start_cost"] and r["stats"]["active_nodes"] < len(r["succ"]) * r["stats"]["decisions"]


def test_headers_libraries_and_python_declare_the_new_entry_points():
    hip = open(os.path.join(ROOT, "include", "tsp_hip.h")).read()
    assert re.search(r"int\s+tsp_dev_nl_3opt_dlb\s*\(", hip) and re.search(r"int\s+tsp_dev_ils_dlb\s*\(", hip)
    assert re.search(r"\}\s*tsp_nl_dlb_stats\s*;", hip) and re.search(r"\}\s*tsp_ils_dlb_stats\s*;", hip)
    assert re.search(r"TSP_DLB_OFF\s*=\s*0\s*,\s*TSP_DLB_ON\s*=\s*1\s*,\s*TSP_DLB_CLOSE\s*=\s*2", hip)
    host = open(os.path.join(ROOT, "include", "tsp_host.h")).read()
    assert re.search(r"\btsp_host_set_dlb\s*\(", host)
    from tsp_optimization_amd import engine as E
    from tsp_optimization_amd.build import lib_path
    for name in ("tsp_dev_nl_3opt_dlb", "tsp_dev_ils_dlb"):
        assert name in E.EXPORTED and hasattr(E.lib(), name), name
    assert (E.DLB_OFF, E.DLB_ON, E.DLB_CLOSE) == (DR.OFF, DR.ON, DR.CLOSE) == (0, 1, 2)
    extra = ["active_nodes", "closing_scans"]
    for new, old in ((E.NlDlbStats, E.Nl3OptStats), (E.IlsDlbStats, E.IlsStats)):
        assert [f for f, _ in new._fields_] == [f for f, _ in old._fields_] + extra
    H = C.CDLL(lib_path("libtsp_host.so"))
    assert hasattr(H, "tsp_host_set_dlb") and hasattr(H, "tsp_host_last_dlb_stats")
    # the setting is checked before anything touches a device
    assert H.tsp_host_set_dlb(3) == E.E_ARG and H.tsp_host_set_dlb(-1) == E.E_ARG
    assert H.tsp_host_set_dlb(2) == 0 and H.tsp_host_set_dlb(0) == 0
