"""The cases of tests/golden/nl_batch_runs.json: instances, lists, start tours and the reference's batched descent taken decision by
decision, shared by the recorder (tests/golden/make_golden_nl_batch.py), tests/test_cpu_nl_batch_golden.py and
tests/test_gpu_nl_batch_golden.py.  A helper of the tests, not collected by pytest.

A1: rand_instance(8000), EUC_2D, integer costs, K = 6; the oracle's greedy tour with the nodes at positions p and p + 1 swapped for
    p = 1, 6, 11, ...; kinds 7, max_arc 8, two rounds: a first decision of more moves than k_nlb_apply has workgroups.
A2: rand_instance(2600), EUC_2D, integer costs, K = 8, from a random tour: arcs of more than 1024 positions.
A3: u724 with non-integer costs, K = 10, from the oracle's greedy tour.

At n = 8000 the reference takes its distances from Euc, which is indexed as the n x n matrix is and holds only the coordinates."""
import copy
import hashlib

import numpy as np

import nl3_opt_ref as N3
import nl_batch_ref as NB
from helpers import load_instance, rand_instance, random_tour
from oracle import oracle as O

NL = N3.NL
R = NL.R

FIXTURE = "nl_batch_runs.json"
A1 = {"n": 8000, "K": 6, "kinds": 7, "max_arc": 8, "rounds": 2}
A1_MIN_MOVES = 1100          # k_nlb_apply has 1024 workgroups
A1_PREFIX = 16               # decisions whose states are recorded one by one
A1_THREE = 3                 # the decisions of the recorded descent
A2 = {"n": 2600, "K": 8, "kinds": 7, "seed": 2600}
A2_DECISIONS = 12
A2_PLAIN = {"max_arc": 2, "rounds": 2, "max_moves": 40}
A2_LONG = 1024               # nl_apply_move<1024>: a longer path is reversed in more than one trip
A3 = {"name": "u724", "K": 10, "kinds": 7}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


class Euc:
    """The oracle's integer EUC_2D distances, indexed with two arrays of nodes as its matrix is."""

    def __init__(self, xy):
        self.xy = np.asarray(xy, dtype=np.float64)

    def __getitem__(self, at):
        a, b = at
        return NL._euc(self.xy, np.asarray(a), np.asarray(b), 1)


def euc_knn(xy, K, rows=500):
    """nl_opt_ref.knn of the integer EUC_2D matrix without the matrix: (distance, id) as one exact float64 key per pair"""
    n = len(xy)
    E = Euc(xy)
    cols = np.arange(n)
    out = np.empty((n, K), dtype=np.int32)
    for r0 in range(0, n, rows):
        r = np.arange(r0, min(r0 + rows, n))
        key = E[r[:, None], cols[None, :]] * n + cols[None, :]
        assert key.max() < 2.0 ** 52
        key[r - r0, r] = np.inf
        part = np.argpartition(key, K, axis=1)[:, :K]
        out[r] = np.take_along_axis(part, np.argsort(np.take_along_axis(key, part, axis=1), axis=1), axis=1)
    return out


def order_to_succ(order):
    succ = np.empty(len(order), dtype=np.int32)
    succ[order] = np.roll(order, -1)
    return succ


def a1_instance(lists=True):
    """-> (xy, wt, the distances, the lists, the start tour); lists = False: (xy, wt, the start tour), as for the two below"""
    n = A1["n"]
    xy = rand_instance(n)
    order = R.tour_order(O.greedy(xy, O.EUC_2D)[1])
    for p in range(1, n - 1, 5):
        order[p], order[p + 1] = order[p + 1], order[p]
    start = order_to_succ(order)
    return (xy, O.EUC_2D, Euc(xy), euc_knn(xy, A1["K"]), start) if lists else (xy, O.EUC_2D, start)


def a2_instance(lists=True):
    n = A2["n"]
    xy = rand_instance(n)
    start = random_tour(n, np.random.default_rng(A2["seed"]))
    if not lists:
        return xy, O.EUC_2D, start
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    return xy, O.EUC_2D, D, NL.knn(D, A2["K"]), start


def a3_instance(lists=True):
    xy, wt = load_instance(A3["name"])
    start = O.greedy(xy, wt, integer_cost=0)[1]
    if not lists:
        return xy, wt, start
    D = O.dist_matrix(xy, wt, 0)
    return xy, wt, D, NL.knn(D, A3["K"]), start


def state(xy, wt, ic, succ, c, per_decision):
    """what the fixture keeps of a tour: no tour, its hash"""
    return {"sha": sha(succ), "cost": O.succ_cost(xy, wt, succ, ic), "counters": copy.deepcopy(c),
            "decision_moves": [int(v) for v in per_decision]}


def kept(c):
    """a device stats dict or a recorded state's counters, as the reference keeps them"""
    return {k: (list(v) if isinstance(v, (list, tuple)) else int(v)) for k, v in c.items() if k in N3.new_counters()}


def decisions(D, succ, nbr, kinds, max_arc, rounds, limit):
    """The loop of nl_batch_ref.descent one decision at a time: yields (the decision's moves, the tour's pos before it, the tour
    after it, the counters after it), `limit` decisions at the most; a decision without a move ends it with moves = []."""
    succ = np.array(succ, dtype=np.int32, copy=True)
    c = N3.new_counters()
    for _ in range(limit):
        c["decisions"] += 1
        moves = NB.decision(D, succ, nbr, kinds, max_arc, rounds)
        pos = NB.tour(succ)[2]
        for m in moves:
            succ = N3.apply_decision(succ, m, c)
        yield moves, pos, succ, copy.deepcopy(c)
        if not moves:
            return


def capped(succ, moves, caps):
    """the first decision under each cap <= len(moves): its first `cap` moves in (delta, key) order -> {cap: (tour, counters)}"""
    succ = np.array(succ, dtype=np.int32, copy=True)
    c = N3.new_counters()
    c["decisions"] = 1
    out = {}
    for q, m in enumerate(moves):
        succ = N3.apply_decision(succ, m, c)
        if q + 1 in caps:
            out[q + 1] = (succ, copy.deepcopy(c))
    return out


def a1_caps(A):
    return sorted({A, A - 1, 1025, 1024, 1})


def long_arcs(moves, pos, n, longer_than):
    return sum(1 for m in moves if NB.arc(m, pos, n)[1] > longer_than)


def wraps(moves, pos, n):
    return sum(1 for m in moves if sum(NB.arc(m, pos, n)) > n)
