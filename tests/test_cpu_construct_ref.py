"""CPU: the matrix references of greedy / grasp / extra-mileage (tests/construct_ref.py) against the oracle's coordinate forms, and
the oracle's fast extra-mileage against its O(n^3) loop.  Everything is compared bit for bit: tour and cost."""
import numpy as np
import pytest

import construct_ref as R
from oracle import oracle as O

METRICS = [O.EUC_2D, O.MAX_2D, O.MAN_2D, O.CEIL_2D, O.GEO, O.ATT]
SIZES = [3, 4, 5, 33, 257]


def points(kind, n, wt):
    rng = np.random.default_rng(7000 + 31 * n + wt)
    if kind == "lattice":       # 3 x 3 lattice: nearly every distance is tied, many nodes coincide
        return rng.integers(0, 3, size=(n, 2)).astype(np.float64)
    if kind == "coincident":
        return np.full((n, 2), 7.0)
    if wt == O.GEO:             # degrees.minutes, well apart
        return np.round(rng.uniform(-60.0, 60.0, size=(n, 2)), 2)
    return rng.uniform(0.0, 3000.0, size=(n, 2))


CASES = [("uniform", n) for n in SIZES] + [("lattice", 40), ("coincident", 12)]


def matrix(xy, wt, ic):
    D = O.dist_matrix(xy, wt, ic)
    assert np.isfinite(D).all()
    return D


def starts_of(n):
    return sorted({0, n - 1, n // 2})


@pytest.mark.parametrize("ic", [1, 0])
@pytest.mark.parametrize("wt", METRICS)
@pytest.mark.parametrize("kind,n", CASES)
def test_matrix_greedy_equals_the_oracle(kind, n, wt, ic):
    xy = points(kind, n, wt)
    D = matrix(xy, wt, ic)
    for s in starts_of(n):
        st, es, eo = O.greedy(xy, wt, start=s, integer_cost=ic)
        succ, obj = R.greedy(D, s)
        assert st == 0 and (succ == es).all() and obj == eo, (kind, n, wt, ic, s, obj, eo)


@pytest.mark.parametrize("ic", [1, 0])
@pytest.mark.parametrize("wt", METRICS)
@pytest.mark.parametrize("kind,n", CASES)
def test_matrix_grasp_equals_the_oracle(kind, n, wt, ic):
    xy = points(kind, n, wt)
    D = matrix(xy, wt, ic)
    for s in starts_of(n):
        # the oracle's own stream: the n values its grasp() draws from libc random()
        O.srandom(100 + s)
        u = np.array([O.urand() for _ in range(n)])
        O.srandom(100 + s)
        st, es, eo = O.grasp(xy, wt, start=s, integer_cost=ic)
        succ, obj = R.grasp(D, s, u)
        assert st == 0 and (succ == es).all() and obj == eo, (kind, n, wt, ic, s, "stream", obj, eo)
        # the runner-up in every step that has one; the winner in every step (then grasp is greedy + one more closing edge)
        for val in (0.95, 0.0):
            u = np.full(n, val)
            st, es, eo = O.grasp(xy, wt, start=s, integer_cost=ic, urand=u)
            succ, obj = R.grasp(D, s, u)
            assert st == 0 and (succ == es).all() and obj == eo, (kind, n, wt, ic, s, val, obj, eo)
            if val == 0.0:
                gs, go = R.greedy(D, s)
                assert (succ == gs).all()


@pytest.mark.parametrize("ic", [1, 0])
@pytest.mark.parametrize("wt", METRICS)
@pytest.mark.parametrize("kind,n", CASES)
def test_matrix_and_fast_extramileage_equal_the_oracle(kind, n, wt, ic):
    xy = points(kind, n, wt)
    D = matrix(xy, wt, ic)
    st, es, eo = O.extramileage(xy, wt, integer_cost=ic)
    succ, obj = R.extramileage(D)
    assert st == 0 and (succ == es).all() and obj == eo, (kind, n, wt, ic, obj, eo)
    st, fs, fo = O.extramileage_fast(xy, wt, integer_cost=ic)
    assert st == 0 and (fs == es).all() and fo == eo, (kind, n, wt, ic, fo, eo)
    assert O.is_tour(es)
    if kind == "coincident":
        # every distance is 0 (GEO: 1): the tour starts from nodes 0 and 1 (heuristics.c:214-215), and every tie goes to the first
        # node and slot 0, which holds (0, c) from then on: 0 -> n-1 -> ... -> 2 -> 1 -> 0
        assert list(es) == [n - 1] + list(range(n - 1))


def test_runner_up_is_not_the_second_nearest():
    """cur = 0; distances to 1, 2, 3 are 5, 1, 2: the winner is 2, the true second nearest is 3, the reference's runner-up is 1."""
    D = np.array([[0, 5, 1, 2], [5, 0, 9, 9], [1, 9, 0, 9], [2, 9, 9, 0]], dtype=np.float64)
    succ, obj = R.grasp(D, 0, np.full(4, 0.95))
    assert succ[0] == 1
    # 0 -> 1 (runner-up of 2), then from 1 both are 9: the winner 2 is the first candidate, no runner-up; 2 -> 3; 3 -> 0 twice
    assert list(succ) == [1, 2, 3, 0] and obj == 5 + 9 + 9 + 2 + 2


def test_extramileage_takes_a_negative_extra():
    """nint() breaks the triangle inequality on a small lattice: (0,0), (2,2), (1,1) give 1 + 1 - 3 = -1 under EUC_2D."""
    xy = np.array([[0, 0], [2, 2], [1, 1], [5, 0]], dtype=np.float64)
    assert O.dist(xy, 0, 2, O.EUC_2D) + O.dist(xy, 2, 1, O.EUC_2D) - O.dist(xy, 0, 1, O.EUC_2D) == -1.0
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    st, es, eo = O.extramileage(xy, O.EUC_2D)
    succ, obj = R.extramileage(D)
    _, fs, fo = O.extramileage_fast(xy, O.EUC_2D)
    assert (succ == es).all() and (fs == es).all() and obj == eo == fo


@pytest.mark.parametrize("kind,wt,ic", [("uniform", O.EUC_2D, 1), ("lattice", O.EUC_2D, 1), ("lattice", O.ATT, 1), ("lattice", O.MAN_2D, 1),
                                        ("lattice", O.MAX_2D, 1), ("uniform", O.EUC_2D, 0)])
def test_fast_extramileage_at_300(kind, wt, ic):
    xy = points(kind, 300, wt)
    st, es, eo = O.extramileage(xy, wt, integer_cost=ic)
    st, fs, fo = O.extramileage_fast(xy, wt, integer_cost=ic)
    assert (fs == es).all() and fo == eo


def test_fast_extramileage_at_700():
    xy = np.random.default_rng(700).integers(0, 3000, size=(700, 2)).astype(np.float64)
    st, es, eo = O.extramileage(xy, O.EUC_2D)
    st, fs, fo = O.extramileage_fast(xy, O.EUC_2D)
    assert O.is_tour(es) and (fs == es).all() and fo == eo
