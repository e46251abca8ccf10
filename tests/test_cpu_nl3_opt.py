"""Candidate-list 3-opt (extension): the tests' CPU reference (tests/nl3_opt_ref.py) against the definition in
include/tsp_hip.h -- the number of moves, every move's new tour, the walk over the list entries against the brute force over
all triples, K = n - 1 as the whole neighbourhood -- and the new names of the C ABI.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import nl3_opt_ref as N3
import nl_opt_ref as NL
from helpers import rand_instance, random_tour
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _instance(n, seed, ic, dup=True):
    """random nodes, a quarter of them on the coordinates of another one: equal distances, so ties"""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 60, size=(n, 2)).astype(np.float64)
    if dup:
        xy[rng.choice(n, size=n // 4, replace=False)] = xy[rng.choice(n, size=n // 4, replace=False)]
    return xy, O.dist_matrix(xy, O.EUC_2D, ic)


def _edge_set(succ):
    return {frozenset((v, int(succ[v]))) for v in range(len(succ))}


@pytest.mark.parametrize("n", range(3, 13))
def test_move_count(n):
    xy, D = _instance(n, n, 1, dup=False)
    for seed in range(3):
        succ = random_tour(n, np.random.default_rng(seed))
        delta, key = N3.moves(D, succ)
        assert len(key) == len(set(key.tolist())) == N3.n_moves(n)
    assert [N3.n_moves(m) for m in (4, 5, 6, 7, 9, 12)] == [0, 10, 32, 70, 210, 640]


@pytest.mark.parametrize("n", [5, 6, 7, 8, 11])
def test_every_move_is_a_tour_with_its_three_new_edges(n):
    xy, D = _instance(n, 100 + n, 1, dup=False)
    succ = random_tour(n, np.random.default_rng(n))
    old = _edge_set(succ)
    pos = np.empty(n, dtype=np.int64)
    pos[NL.R.tour_order(succ)] = np.arange(n)
    delta, key = N3.moves(D, succ)
    for dl, k in zip(delta, key.tolist()):
        a, b, c, T = N3.decode(k, n)
        assert a < b and a < c and 0 < (pos[b] - pos[a]) % n < (pos[c] - pos[a]) % n
        a1, b1, c1 = int(succ[a]), int(succ[b]), int(succ[c])
        new = N3.apply_three_opt(succ, a, b, c, T)
        assert O.is_tour(new)
        E = N3.new_edges(T, a, a1, b, b1, c, c1)
        added = {frozenset(e) for e in E}
        removed = {frozenset((a, a1)), frozenset((b, b1)), frozenset((c, c1))}
        assert len(added) == 3 and not (added & old)
        assert _edge_set(new) == (old - removed) | added
        assert O.succ_cost(xy, O.EUC_2D, new) - O.succ_cost(xy, O.EUC_2D, succ) == dl
        # forward orientation: S3 = c1 .. a keeps its direction
        v = c1
        while v != a:
            assert new[v] == succ[v]
            v = int(succ[v])


@pytest.mark.parametrize("ic", [1, 0])
@pytest.mark.parametrize("n", [5, 6, 7, 8, 9, 10, 13, 17, 24, 31, 40])
def test_sparse_walk_equals_brute_force(n, ic):
    xy, D = _instance(n, 200 + n, ic)
    rng = np.random.default_rng(n * 2 + ic)
    for K in sorted({1, 2, min(5, n - 1), n - 1}):
        lists = [NL.knn(D, K)]
        off = rng.integers(1, n, size=(n, K))                       # directed lists without any symmetry, duplicates happen
        lists.append(((np.arange(n)[:, None] + off) % n).astype(np.int32))
        for nbr in lists:
            for _ in range(3):
                succ = random_tour(n, rng)
                bd, bk = N3.moves(D, succ, nbr)
                sd, sk = N3.sparse_moves(D, succ, nbr)
                want = dict(zip(bk.tolist(), bd.tolist()))
                got = dict(zip(sk.tolist(), sd.tolist()))
                assert len(want) == len(bk)
                assert got == want, (n, K)
                for kinds in (4, 5, 6, 7):
                    assert N3.decide_sparse(D, succ, nbr, kinds) == N3.decide(D, succ, nbr, kinds)


@pytest.mark.parametrize("n", [5, 6, 9, 14])
def test_full_lists_are_the_whole_neighbourhood(n):
    xy, D = _instance(n, 300 + n, 1)
    succ = random_tour(n, np.random.default_rng(n))
    nbr = NL.knn(D, n - 1)
    md, mk = N3.moves(D, succ)
    ld, lk = N3.moves(D, succ, nbr)
    assert len(mk) == N3.n_moves(n) and (mk == lk).all() and (md == ld).all()
    sd, sk = N3.sparse_moves(D, succ, nbr)
    assert set(sk.tolist()) == set(mk.tolist())


def test_descent_ends_in_a_tour_no_kind_improves_and_low_kinds_follow_nl_opt_ref():
    n = 30
    xy, D = _instance(n, 7, 1)
    succ = random_tour(n, np.random.default_rng(7))
    nbr = NL.knn(D, 5)
    for kinds in (1, 2, 3):
        s, c = N3.descent(D, succ, nbr, kinds)
        s0, c0 = NL.descent(D, succ, nbr, kinds)
        assert (s == s0).all() and all(c[k] == c0[k] for k in c0) and c["moves_3opt"] == 0
    s7, c7 = N3.descent(D, succ, nbr, 7)
    sb, cb = N3.descent(D, succ, nbr, 7, sparse=False)
    assert (s7 == sb).all() and c7 == cb and c7["moves_3opt"] > 0 and sum(c7["moves_by_type"]) == c7["moves_3opt"]
    assert O.is_tour(s7) and N3.decide(D, s7, nbr, 7) is None
    for m in (3, 4):
        st = random_tour(m, np.random.default_rng(m))
        s, c = N3.descent(D[:m, :m], st, NL.knn(D[:m, :m], m - 1), 7 if m == 4 else 4)
        assert c["moves_3opt"] == 0


def test_headers_and_python_declare_the_new_entry_point():
    hip = open(os.path.join(ROOT, "include", "tsp_hip.h")).read()
    assert re.search(r"TSP_NL_3OPT\s*=\s*4", hip)
    assert re.search(r"int\s+tsp_dev_nl_3opt\s*\(", hip) and "tsp_nl3_opt_stats" in hip
    host = open(os.path.join(ROOT, "include", "tsp_host.h")).read()
    for name in ("alg_3opt", "tsp_host_last_nl3_stats"):
        assert re.search(r"\b%s\s*\(" % name, host), name
    from tsp_optimization_amd import engine as E
    assert E.NL_3OPT == 4 and "tsp_dev_nl_3opt" in E.EXPORTED and hasattr(E.Instance, "nl_3opt")
    old = [f for f, _ in E.NlOptStats._fields_]
    new = [f for f, _ in E.Nl3OptStats._fields_]
    assert new[:len(old)] == old and new[len(old):] == ["moves_3opt", "moves_by_type"]
