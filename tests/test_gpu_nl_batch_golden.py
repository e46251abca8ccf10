"""The batched list descent on the device (tsp_dev_nl_3opt_batch) against the recorded trajectories of its CPU reference
(tests/golden/nl_batch_runs.json, recorded by tests/golden/make_golden_nl_batch.py, held to the reference by
tests/test_cpu_nl_batch_golden.py): a decision of more moves than k_nlb_apply has workgroups, whole and under caps that cut it; arcs
longer than a workgroup of nl_apply_move; a TSPLIB instance with non-integer costs to its end; a time-limited run, which ends
between two decisions.  One test per record: the recorded tour (by its hash), cost and counters."""
import pytest

import nl_batch_golden_cases as G
from helpers import golden
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from tsp_optimization_amd import engine as E
    assert E.device_count() >= 1, "no HIP device visible: the product path has no CPU fallback"
    return E


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def runs():
    return golden(G.FIXTURE)


def _instance(eng, ctx, rec, xy, wt, start):
    """the device's lists are the recorded ones, the start tour is the recorded one"""
    p = rec["params"]
    inst = eng.Instance(ctx, xy, wt, p["integer_cost"])
    inst.knn_build(p["K"])
    assert G.sha(inst.knn()) == rec["lists_sha"], "the lists differ from the reference's"
    assert G.sha(start) == rec["start_sha"]
    return inst


def _is(rec, rc, succ, obj, st, want_rc=0):
    assert rc == want_rc
    assert O.is_tour(succ)
    got = G.kept(st)
    for k, v in rec["counters"].items():
        assert got[k] == v, (k, got[k], v, "moves per decision: %s" % rec["decision_moves"])
    assert G.sha(succ) == rec["sha"], "tour differs from the reference; moves per decision: %s" % rec["decision_moves"]
    assert obj == rec["cost"]


@pytest.fixture(scope="module")
def a1(eng, ctx, runs):
    xy, wt, start = G.a1_instance(lists=False)
    inst = _instance(eng, ctx, runs["A1"], xy, wt, start)
    yield inst, xy, wt, start, runs["A1"]
    inst.close()


def _a1_run(a1, **kw):
    inst, xy, wt, start, rec = a1
    p = rec["params"]
    kw.setdefault("time_limit", 300.0)
    return inst.nl_3opt_batch(start, kinds=p["kinds"], max_arc=p["max_arc"], rounds=p["rounds"], **kw)


@pytest.mark.parametrize("cap", ["A", "A-1", "1025", "1024", "1"])
def test_a_decision_wider_than_the_apply_grid_under_a_cap(a1, cap):
    """cap = A: every workgroup of k_nlb_apply carries out one or two moves; below it the first `cap` in (delta, key) order"""
    rec = a1[4]
    A = rec["A"]
    assert A >= G.A1_MIN_MOVES
    cap = {"A": A, "A-1": A - 1}.get(cap) or int(cap)
    rc, s, o, st = _a1_run(a1, max_moves=cap)
    assert st["decisions"] == 1 and st["moves"] == cap
    _is(rec["caps"][str(cap)], rc, s, o, st)


def test_the_first_decisions_of_the_wide_descent(a1):
    rec = a1[4]["descent"]
    rc, s, o, st = _a1_run(a1, max_moves=rec["max_moves"])
    assert st["decisions"] == rec["decisions"] == len(rec["decision_moves"])
    _is(rec, rc, s, o, st)


def test_a_time_limited_run_ends_between_decisions(eng, a1):
    """Descent::run stops between whole decisions: the tour is the reference's after exactly stats.decisions of them"""
    inst, xy, wt, start, rec = a1
    rc, s, o, st = _a1_run(a1, time_limit=1e-6)
    assert rc == eng.TIME_LIMIT_EXCEEDED == 2
    assert O.is_tour(s) and o == O.succ_cost(xy, wt, s)
    assert st["decisions"] >= 1
    assert st["decisions"] <= len(rec["prefix"]), \
        "the device took %d decisions within the limit: record a longer prefix (A1_PREFIX)" % st["decisions"]
    _is(rec["prefix"][st["decisions"] - 1], rc, s, o, st, want_rc=2)


@pytest.fixture(scope="module")
def a2(eng, ctx, runs):
    xy, wt, start = G.a2_instance(lists=False)
    inst = _instance(eng, ctx, runs["A2"], xy, wt, start)
    yield inst, start, runs["A2"]
    inst.close()


@pytest.mark.parametrize("name", ["default", "plain"])
def test_arcs_longer_than_a_workgroup(a2, name):
    inst, start, rec = a2
    r = rec[name]
    assert r["long_arcs"] >= 1
    max_arc, rounds = (0, 0) if name == "default" else (r["max_arc"], r["rounds"])
    rc, s, o, st = inst.nl_3opt_batch(start, kinds=rec["params"]["kinds"], max_arc=max_arc, rounds=rounds, max_moves=r["max_moves"],
                                      time_limit=300.0)
    _is(r, rc, s, o, st)


def test_u724_with_non_integer_costs_to_the_end(eng, ctx, runs):
    rec = runs["A3"]
    xy, wt, start = G.a3_instance(lists=False)
    inst = _instance(eng, ctx, rec, xy, wt, start)
    rc, s, o, st = inst.nl_3opt_batch(start, kinds=rec["params"]["kinds"], time_limit=300.0)
    inst.close()
    _is(rec["descent"], rc, s, o, st)
