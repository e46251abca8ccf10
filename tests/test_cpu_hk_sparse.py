"""CPU: the reference of the sparse Held-Karp definitions (tests/hk_sparse_ref.py) against itself and against the dense
reference (tests/held_karp_ref.py), the stability of the step-by-step cases (tests/hk_sparse_cases.py) under the summation
order.  (The C ABI of the new entry points: test_cpu_hk_sparse_abi.py.)"""
import os

import numpy as np
import pytest

import held_karp_ref as HK
import hk_sparse_cases as SC
import hk_sparse_ref as S
import hk_trace_cases as T
from helpers import INSTANCES
from oracle import oracle as O


def matrix(name, wt_as=None, integer_cost=1):
    xy, wt = O.parse_tsplib(os.path.join(INSTANCES, name + ".tsp"))
    return O.dist_matrix(xy, wt if wt_as is None else wt_as, integer_cost)


def penalties(D, seed):
    n = len(D)
    return np.random.default_rng(seed).uniform(-0.5, 0.5, n) * D[np.triu_indices(n, 1)].mean()


SMALL = [("burma14", None, 1), ("ulysses22", None, 0), ("att48", None, 1), ("berlin52", None, 1), ("berlin52", O.CEIL_2D, 0),
         ("berlin52", O.MAN_2D, 1), ("berlin52", O.MAX_2D, 0), ("eil51", None, 0)]


@pytest.mark.parametrize("name,wt_as,ic", SMALL)
def test_complete_lists_give_the_dense_tree_edge_for_edge(name, wt_as, ic):
    D = matrix(name, wt_as, ic)
    n = len(D)
    full = S.knn_lists(D, n - 1)
    for pi in (None, penalties(D, 3)):
        e, d, v, w, comps = S.one_tree_sparse(D, full, pi)
        re_, rd, rv, rw = HK.one_tree(D, pi)
        assert (e == re_).all() and (d == rd).all() and v == rv and (w == rw).all() and comps == 1
        rs, rc, bc, be, bd, bv, _ = S.boruvka_sparse(D, full, pi)
        assert (be == re_).all() and bv == rv and rc == 0 and bc == 1 and rs == HK.boruvka_rounds(D, pi)


@pytest.mark.parametrize("K", [1, 2, 3, 5, 10])
@pytest.mark.parametrize("name,wt_as,ic", SMALL)
def test_kruskal_and_boruvka_agree_and_the_sparse_value_is_no_smaller(name, wt_as, ic, K):
    D = matrix(name, wt_as, ic)
    nbr = S.knn_lists(D, K)
    for pi in (None, penalties(D, 11 + K)):
        e, d, v, w, comps = S.one_tree_sparse(D, nbr, pi)
        rs, rc, bc, be, bd, bv, bw = S.boruvka_sparse(D, nbr, pi)
        assert (e == be).all() and (d == bd).all() and v == bv and comps == bc
        assert (rc == 0) == (comps == 1) and rs >= 1
        assert d.sum() == 2 * len(D) and d[0] == 2
        dense = HK.one_tree(D, pi)[2]
        assert v >= dense - 1e-12 * abs(dense)   # W_C >= W: T_C is a 1-tree, T the minimum one


def test_the_completion_joins_two_halves_by_their_cheapest_edge():
    """Two cliques of three nodes far apart (nodes 1-3 and 4-6), lists confined to each: the completion adds exactly the
    cheapest edge between them; node 0's lists name nodes 1 and 4."""
    xy = np.array([[0, 50], [0, 0], [1, 0], [0, 2], [100, 0], [103, 0], [100, 4]], dtype=np.float64)
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    nbr = np.array([[1, 4], [2, 3], [1, 3], [1, 2], [5, 6], [4, 6], [4, 5]], dtype=np.int32)
    e, d, v, w, comps = S.one_tree_sparse(D, nbr)
    assert comps == 2
    cross = [(a, b) for a, b in e.tolist() if 1 <= a <= 3 and b >= 4]
    assert cross == [(2, 4)]   # d = 99, the smallest between the halves
    assert [(a, b) for a, b in e.tolist() if a == 0] == [(0, 1), (0, 4)]   # the candidates, although (0, 3) is shorter than (0, 4)
    rs, rc, bc, be = S.boruvka_sparse(D, nbr)[:4]
    assert (be == e).all() and (rs, rc, bc) == (1, 1, 2)


def test_node_0_falls_back_to_all_its_edges_with_fewer_than_two_candidates():
    xy = np.array([[0, 0], [10, 0], [1, 0], [2, 0], [10, 1]], dtype=np.float64)
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    one = np.array([[1], [4], [3], [2], [1]], dtype=np.int32)      # {0,1} is node 0's only candidate edge
    e = S.one_tree_sparse(D, one)[0]
    assert [(a, b) for a, b in e.tolist() if a == 0] == [(0, 2), (0, 3)]   # the two nearest of all
    two = np.array([[1], [4], [3], [2], [0]], dtype=np.int32)      # {0,1} and {0,4}: named from either end
    e = S.one_tree_sparse(D, two)[0]
    assert [(a, b) for a, b in e.tolist() if a == 0] == [(0, 1), (0, 4)]
    dup = np.array([[1], [0], [3], [2], [1]], dtype=np.int32)      # {0,1} named twice is still one edge
    e = S.one_tree_sparse(D, dup)[0]
    assert [(a, b) for a, b in e.tolist() if a == 0] == [(0, 2), (0, 3)]


def test_the_sparse_phase_rules():
    D = matrix("berlin52")
    nbr = S.knn_lists(D, 5)
    # W_C >= ub ends the phase before the step: a ub below W_C(0)
    w0 = S.one_tree_sparse(D, nbr)[2]
    tr = S.ascent_trace_sparse(D, nbr, w0 - 1.0, 10, 2, patience=3)
    assert tr.ended == "ub" and len(tr.sparse) == 1 and tr.lam == 2.0 and tr.best == w0
    assert (tr.pi_best == 0).all() and len(tr.dense) == 2
    # no sparse iteration: the dense reference alone
    tr0 = S.ascent_trace_sparse(D, nbr, 8069.94, 0, 7, patience=3)
    ref = HK.ascent_trace(D, 8069.94, 7, 2.0, 3)
    assert tr0.sparse == [] and [s.W for s in tr0.dense] == [s.W for s in ref] and tr0.bound == ref[-1].best
    # complete lists: the sparse phase follows the dense ascent step for step
    D14 = matrix("burma14")
    full = S.knn_lists(D14, 13)
    sp = S.sparse_phase(D14, full, 3555.61, 25, 2.0, 3)[0]
    de = HK.ascent_trace(D14, 3555.61, 25, 2.0, 3)
    assert len(sp) == len(de) and all(a.W == b.W and a.lam == b.lam and (a.deg == b.deg).all() for a, b in zip(sp, de))


def test_a_sparse_tree_that_is_a_tour_proves_nothing():
    """Lists that hold a tour's edges and nothing else: the first sparse tree... is a path plus node 0's two edges, a tour;
    the phase ends there without a step, and tour_found is the dense phase's word alone."""
    D = matrix("ulysses22")
    n = len(D)
    order = np.arange(n)
    nbr = np.stack([np.roll(order, 1), np.roll(order, -1)], axis=1).astype(np.int32)   # v-1, v+1: the tour 0, 1, ..., n-1
    tr = S.ascent_trace_sparse(D, nbr, 1e6, 10, 1, patience=3)
    assert tr.ended == "tour" and len(tr.sparse) == 1 and tr.sparse[0].g2 == 0.0
    assert not tr.tour_found and tr.bound < tr.best   # the dense tree at the same penalties is cheaper and no tour


def test_case_list_is_large_and_covers_every_metric_and_cost_setting():
    assert len(SC.CASES) >= 20
    seen = {(c.load()[1], c.integer_cost) for c in SC.CASES}
    assert seen >= {(wt, ic) for wt in (O.EUC_2D, O.MAX_2D, O.MAN_2D, O.CEIL_2D, O.GEO, O.ATT) for ic in (0, 1)}
    assert all(name in T.IDS for name in SC.UNSTABLE) and all(SC.UNSTABLE.values())
    assert any(c.name.startswith("clustered") for c in SC.CASES)


@pytest.mark.parametrize("case", SC.CASES, ids=SC.IDS)
def test_every_case_is_stable_under_the_summation_order(case):
    """What test_cpu_held_karp.py asks of the dense cases: under 10 seeded summation orders the trees and lambda of every
    iteration (40 sparse, 5 dense behind them) are the reference's, and best / pi_best stay within 1e-14."""
    D = case.matrix()
    nbr = SC.lists(case, D)
    ref = SC.trace(case, D, nbr)
    steps = ref.sparse + ref.dense
    worst_b = worst_p = 0.0
    for seed in range(10):
        got = SC.trace(case, D, nbr, sum_order=np.random.default_rng(100 + seed))
        assert got.ended == ref.ended and len(got.sparse) == len(ref.sparse) and len(got.dense) == len(ref.dense)
        for r, s in zip(steps, got.sparse + got.dense):
            assert (r.deg == s.deg).all() and r.lam == s.lam, (seed, r.k)
            b, p = T.deviation(r, s.best, s.pi_best)
            worst_b, worst_p = max(worst_b, b), max(worst_p, p)
    print("%s: best moves by %.1e, pi_best by %.1e" % (case.id, worst_b, worst_p))
    assert worst_b <= 1e-14 and worst_p <= 1e-14


def test_the_clustered_cases_have_a_completion_in_every_tree():
    for case in SC.CASES:
        if case.name.startswith("clustered"):
            D = case.matrix()
            tr = SC.trace(case, D, SC.lists(case, D), sparse_iters=6, dense_iters=1, rounds=True)
            assert all(rc >= 1 and rs >= 1 for rs, rc in tr.tree_rounds)
