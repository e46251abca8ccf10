"""CPU: tests/golden/nl_batch_runs.json cannot drift from the reference that recorded it (tests/nl_batch_ref.py through
tests/nl_batch_golden_cases.py): the first decision of case A1 and its five caps and the max_arc = 2 record of case A2 are
recomputed here, the latter is the plain descent of nl3_opt_ref move for move, and the fixture's own numbers meet the conditions
that make its cases worth their name (a decision wider than k_nlb_apply's grid, all three kinds, a wrapping arc, arcs longer than
a workgroup)."""
import numpy as np
import pytest

import nl3_opt_ref as N3
import nl_batch_golden_cases as G
import nl_batch_ref as NB
from helpers import golden, random_tour
from oracle import oracle as O

NL = N3.NL


@pytest.fixture(scope="module")
def runs():
    return golden(G.FIXTURE)


def _states(rec):
    if isinstance(rec, dict):
        if "sha" in rec:
            yield rec
        for v in rec.values():
            yield from _states(v)
    elif isinstance(rec, list):
        for v in rec:
            yield from _states(v)


def test_the_fixture_meets_the_conditions_of_its_cases(runs):
    a1, a2, a3 = runs["A1"], runs["A2"], runs["A3"]
    A = a1["A"]
    assert A >= G.A1_MIN_MOVES > 1024
    assert sum(a1["first"]["by_kind"]) == A and all(k >= 1 for k in a1["first"]["by_kind"]) and a1["first"]["wraps"] >= 1
    assert sorted(int(k) for k in a1["caps"]) == G.a1_caps(A) == [1, 1024, 1025, A - 1, A]
    for cap, rec in a1["caps"].items():
        assert rec["counters"]["decisions"] == 1 and rec["counters"]["moves"] == int(cap)
    assert len(a1["prefix"]) == G.A1_PREFIX and a1["prefix"][0] == a1["caps"][str(A)]
    assert [p["counters"]["decisions"] for p in a1["prefix"]] == list(range(1, G.A1_PREFIX + 1))
    three = a1["descent"]
    assert three["decisions"] == G.A1_THREE and three["max_moves"] == sum(three["decision_moves"])
    assert {k: three[k] for k in a1["prefix"][2]} == a1["prefix"][2]
    assert a2["default"]["long_arcs"] >= 1 and a2["plain"]["long_arcs"] >= 1
    assert len(a2["default"]["decision_moves"]) == G.A2_DECISIONS and a2["default"]["max_moves"] == sum(a2["default"]["decision_moves"])
    assert a2["plain"]["decision_moves"] == [1] * G.A2_PLAIN["max_moves"] and a2["plain"]["max_arc"] == G.A2_PLAIN["max_arc"] < 4
    assert a3["descent"]["decision_moves"][-1] == 0 and a3["params"]["integer_cost"] == 0
    states = list(_states(runs))
    assert len(states) == 5 + G.A1_PREFIX + 1 + 2 + 1
    for rec in states:
        c = rec["counters"]
        assert sorted(c) == sorted(N3.new_counters())
        assert len(rec["decision_moves"]) == c["decisions"] and sum(rec["decision_moves"]) == c["moves"]
        assert c["moves"] == c["moves_2opt"] + c["moves_oropt"] + c["moves_3opt"]
        assert sum(c["moves_by_len"]) == c["moves_oropt"] and sum(c["moves_by_type"]) == c["moves_3opt"]


def test_the_helpers_take_the_references_descent_apart():
    """decisions() and capped() against nl_batch_ref.descent, and the lists without the matrix against nl_opt_ref.knn"""
    n = 120
    xy = np.random.default_rng(3).integers(0, 2000, (n, 2)).astype(np.float64)
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    nbr = NL.knn(D, 6)
    assert (G.euc_knn(xy, 6, rows=50) == nbr).all()
    rows = np.arange(n)
    assert (G.Euc(xy)[rows[:, None], rows[None, :]] == D).all()
    start = random_tour(n, np.random.default_rng(4))
    trace = []
    ref, c = NB.descent(D, start, nbr, 7, 16, 2, trace=trace)
    got = list(G.decisions(G.Euc(xy), start, nbr, 7, 16, 2, 10 ** 6))
    assert [g[0] for g in got] == trace + [[]] and (got[-1][2] == ref).all() and got[-1][3] == c
    assert len(got[0][0]) >= 3
    for cap, (succ, cc) in G.capped(start, got[0][0], {1, len(got[0][0]) - 1, len(got[0][0])}).items():
        ref, c = NB.descent(D, start, nbr, 7, 16, 2, max_moves=cap)
        assert (succ == ref).all() and cc == c


def test_the_wide_decision_and_its_caps_are_the_references(runs):
    rec = runs["A1"]
    p = rec["params"]
    xy, wt, D, nbr, start = G.a1_instance()
    assert len(xy) == p["n"] and G.sha(nbr) == rec["lists_sha"] and G.sha(start) == rec["start_sha"]
    moves = NB.decision(D, start, nbr, p["kinds"], p["max_arc"], p["rounds"])
    assert len(moves) == rec["A"]
    assert [sum(1 for m in moves if m[1] == k) for k in range(3)] == rec["first"]["by_kind"]
    assert G.wraps(moves, NB.tour(start)[2], len(xy)) == rec["first"]["wraps"]
    got = G.capped(start, moves, set(G.a1_caps(len(moves))))
    assert sorted(got) == sorted(int(k) for k in rec["caps"])
    for cap, (succ, c) in got.items():
        assert G.state(xy, wt, 1, succ, c, [cap]) == rec["caps"][str(cap)], cap


def test_arcs_too_short_for_any_move_record_the_plain_descent(runs):
    rec = runs["A2"]
    r = rec["plain"]
    xy, wt, D, nbr, start = G.a2_instance()
    n = len(xy)
    assert G.sha(nbr) == rec["lists_sha"] and G.sha(start) == rec["start_sha"]
    trace = []
    got, c = NB.descent(D, start, nbr, rec["params"]["kinds"], r["max_arc"], r["rounds"], max_moves=r["max_moves"], trace=trace)
    assert G.state(xy, wt, 1, got, c, [len(t) for t in trace]) == {k: r[k] for k in ("sha", "cost", "counters", "decision_moves")}
    # the 2-opt and Or-opt kinds from the list entries alone (nl_opt_ref.decide_sparse, which tests/test_cpu_nl_opt.py holds to
    # the masked matrices): at n = 2600 the matrices take seconds per decision
    plain = []
    ref, cp = N3.descent(D, start, nbr, rec["params"]["kinds"], max_moves=r["max_moves"], trace=plain,
                         low=lambda D_, succ, nbr_, kinds: NL.decide_sparse(xy, succ, nbr_, kinds))
    assert (got == ref).all() and c == cp and [[m] for m in plain] == trace
    succ, long_arcs = start, 0
    for m in plain:
        long_arcs += G.long_arcs([m], NB.tour(succ)[2], n, G.A2_LONG)
        succ = N3.apply_decision(succ, m, N3.new_counters())
    assert long_arcs == r["long_arcs"]
