"""The windowed iterated local search on the device (tsp_dev_seg_ils, _seg_ils3, _seg_ils_groups, _seg_ils_lk) against the recorded
results of its CPU references at the shapes it works at (tests/golden/seg_runs.json, recorded by tests/golden/make_golden_seg.py, held
to the references by tests/test_cpu_seg_golden.py): windows of 1024 and 2048 whose active set, reversals, relabelings and chain hulls
outgrow the workgroup, 78 windows at once without groups, 1248 workgroups with groups, 640 iterations of a search that rejects nearly
every trial, and a time limit that cuts them.  One test per recorded state: a valid tour with the recorded hash, cost, start_cost
and every counter of the reference, and the same bits (deltas_executed too) from a second call.

Behind them, inline against the references: non-integer costs at windows whose cost tree takes more than one pass of the
workgroup (W - 1 = 517 and 1024, n - 1 of u724 and pr1002, ATT, lattices with their ties), with groups and chains, without
groups, and the kick alone, which is accepted by the tree's sum and nothing else: there a node far away makes the outcome
depend on the order of that sum.  There are no tolerances: the definition fixes every order."""
import numpy as np
import pytest

import seg_golden_cases as G
import seg_ils3_ref as S3
import seg_lk_ref as SL
from helpers import golden, random_tour
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LIMIT = 300.0      # a call that does not end is a failure, not a hang
STATES = [(name, it) for name, r in G.RUNS.items() for it in r["iterations"]]


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


@pytest.fixture(scope="module")
def insts(eng, ctx, runs):
    """name -> (the device's instance with its own lists, which are the recorded ones; the recorded start tour), built once"""
    made = {}

    def get(name):
        if name not in made:
            rec = runs["instances"][name]
            xy, wt, start = G.instance(name, lists=False)
            inst = eng.Instance(ctx, xy, wt, rec["integer_cost"])
            inst.knn_build(rec["K"])
            assert G.sha(inst.knn()) == rec["lists_sha"], "the lists differ from the reference's"
            assert G.sha(start) == rec["start_sha"]
            made[name] = (inst, start)
        return made[name]

    yield get
    for inst, _ in made.values():
        inst.close()


def _is(r, rec, rc, succ, obj, st, want_rc=0):
    assert rc == want_rc
    assert O.is_tour(succ)
    got = G.kept(r["entry"], st)
    print(r["entry"], "device:", got, obj, "recorded:", rec["counters"], rec["cost"])
    for k, v in rec["counters"].items():
        assert got[k] == v, (k, got[k], v)
    assert G.sha(succ) == rec["sha"], "tour differs from the reference"
    assert obj == rec["cost"] and st["start_cost"] == rec["start_cost"]


def _alive(r, st):
    """the call ran what its run is about, by the device's own counters"""
    G.consistent(r["entry"], G.kept(r["entry"], st), st["iterations"], r["trials"])
    assert st["deltas_executed"] > 0 or not r["kinds"] & 7
    for bit, k in ((1, "moves_2opt"), (2, "moves_oropt"), (4, "moves_3opt"), (8, "moves_lk")):
        assert st[k] > 0 if r["kinds"] & bit else not st.get(k, 0), (k, st)
    if r["kinds"] & 8:
        assert st["lk_flips"] > st["moves_lk"] and st["lk_steps"] > st["lk_flips"] and st["lk_depth"] == r["depth"]
    if r["case"] == "S1":
        assert st["windows"] == 1 and st["accepted"] >= 1 and (st["reversed"] > G.THREADS or not r["kinds"] & 1)
        assert st["active_nodes"] > G.THREADS * st["decisions"] // 4           # the mean alone is a quarter of the workgroup
    if r["case"] == "S2":
        assert st["windows"] == 1 and st["accepted"] == 1 and st["active_nodes"] > G.THREADS * st["decisions"]
    if r["case"] == "S3":
        assert st["windows"] == 78 and 2 * st["accepted"] > st["windows"] * st["iterations"]
    if r["case"] == "S4":
        assert st["commits"] < st["offers"] and st["groups"] == r["groups"]
        assert r["span"] or st["accepted"] < st["trials"]                      # span W - 1: trials are rejected and restored
        assert r["window"] != 64 or st["windows"] * st["groups"] == 1248 > G.RESIDENT
    if r["case"] == "S5":
        assert 10 * st["accepted"] < st["trials"] and st["iterations"] > G.BATCH_ENDS[7]


# ---- 1. the recorded states ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,iterations", STATES, ids=["%s-%d" % s for s in STATES])
def test_a_recorded_state(insts, runs, name, iterations):
    r = runs["runs"][name]
    assert {k: r[k] for k in G.RUNS[name]} == G.RUNS[name], "the fixture was recorded with other parameters"
    inst, start = insts(r["instance"])
    rc, s, o, st = G.dev_run(inst, r, start, iterations, LIMIT)
    _is(r, r["states"][str(iterations)], rc, s, o, st)
    if iterations == max(r["iterations"]):
        _alive(r, st)
    # no scheduling order of the workgroups leaks into the result
    rc2, s2, o2, st2 = G.dev_run(inst, r, start, iterations, LIMIT)
    assert rc2 == 0 and (s2 == s).all() and o2 == o
    assert all(st2[k] == st[k] for k in G.counters_of(r["entry"]) + ("start_cost", "deltas_executed"))


@pytest.mark.parametrize("name", ["S5-lk", "S5-groups"])
def test_a_time_limit_cuts_the_long_run_between_two_iterations(eng, insts, runs, name):
    """Descent::run looks at the clock between its batches: the tour is the reference's after exactly stats.iterations"""
    r = runs["runs"][name]
    inst, start = insts(r["instance"])
    full = max(r["iterations"])
    G.dev_run(inst, r, start, full, LIMIT)
    rc, s, o, st = G.dev_run(inst, r, start, full, LIMIT)          # the second call's time: the first may have loaded the kernel
    _is(r, r["states"][str(full)], rc, s, o, st)
    limit = 0.3 * st["seconds"]
    rc, s, o, st = G.dev_run(inst, r, start, 10 ** 9, limit)
    print("limit %.6f s: %d iterations" % (limit, st["iterations"]))
    assert rc == eng.TIME_LIMIT_EXCEEDED and 0 < st["iterations"] < full
    assert O.is_tour(s)
    rec = r["states"].get(str(st["iterations"]))
    if rec is not None:
        _is(r, rec, rc, s, o, st, want_rc=eng.TIME_LIMIT_EXCEEDED)
    else:
        rc2, s2, o2, st2 = G.dev_run(inst, r, start, st["iterations"], LIMIT)
        assert rc2 == 0 and (s2 == s).all() and o2 == o
        assert all(st2[k] == st[k] for k in G.counters_of(r["entry"]) + ("start_cost", "deltas_executed"))


# ---- 2. inline: non-integer costs at large windows ------------------------------------------------------------------------------------------

def _same(entry, dev, ref):
    (rc, s, o, st), (ref_succ, ref_cost, ref_st) = dev, ref
    assert rc == 0 and O.is_tour(s)
    got = G.kept(entry, st)
    print(entry, "device:", got, o, "reference:", G.kept(entry, ref_st), ref_cost)
    for k in G.counters_of(entry):
        assert got[k] == ref_st[k], (k, got[k], ref_st[k])
    assert (s == np.asarray(ref_succ)).all(), "tour differs from the reference"
    assert np.float64(o).tobytes() == np.float64(ref_cost).tobytes() and st["start_cost"] == ref_st["start_cost"]


@pytest.fixture(scope="module")
def inline(eng, ctx):
    """name -> (the device's instance under non-integer costs with its own lists, the oracle's matrix, the lists, the start)"""
    made = {}

    def get(name):
        if name not in made:
            K = G.INLINE[name][2]
            xy, wt, start = G.inline_instance(name)
            inst = eng.Instance(ctx, xy, wt, 0)
            inst.knn_build(K)
            made[name] = (inst, O.dist_matrix(xy, wt, 0), inst.knn(), start)
        return made[name]

    yield get
    for m in made.values():
        m[0].close()


@pytest.mark.parametrize("name", G.DESCENTS)
def test_non_integer_costs_at_a_window_deeper_than_one_pass_with_groups_and_chains(inline, name):
    _, _, K, W, Gr, T, its, seed = G.INLINE[name]
    inst, D, nbr, start = inline(name)
    assert W - 1 > 2 * G.THREADS and (D != np.floor(D)).any()
    ref = SL.run(D, start, nbr, 15, seed, 0, its, 16, Gr, W, 0, T)
    dev = inst.seg_ils_lk(start, its, 15, 16, Gr, W, 0, T, seed=seed, time_limit=LIMIT)
    _same("seg_ils_lk", dev, ref)
    st = dev[3]
    assert 0 < st["accepted"] and st["moves_lk"] > 0 and st["lk_flips"] > st["moves_lk"] and st["offers"] > 0


@pytest.mark.parametrize("name", G.DESCENTS)
def test_non_integer_costs_at_a_window_deeper_than_one_pass_without_groups(inline, name):
    """tsp_dev_seg_ils3: the workgroup that accepts writes order / pos itself"""
    _, _, K, W, Gr, T, its, seed = G.INLINE[name]
    inst, D, nbr, start = inline(name)
    ref = S3.run(D, start, nbr, 7, seed, 0, its, W, 0, T)
    dev = inst.seg_ils3(start, its, W, 0, T, seed=seed, kinds=7, time_limit=LIMIT)
    _same("seg_ils3", dev, ref)
    assert dev[3]["moves_3opt"] > 0 and dev[3]["trials"] == its * T * (D.shape[0] // W)


@pytest.mark.parametrize("name", G.KICKS)
def test_the_kick_alone_is_accepted_by_the_sum_of_the_tree(inline, name):
    """max_moves = 0: a trial is its kick, kept when the kicked window is cheaper by the tree's sum.  From a random tour about
    half of the kicks are; twenty seeds, three iterations of two trials each.  On the far instances (one node of the window at
    1e22: W - 1 = 517 and 1024) that sum in another order accepts other kicks, as tests/test_cpu_seg_golden.py makes sure:
    they pin the order of the tree, without groups and, every seed, with groups"""
    _, _, K, W, Gr, T, its, _ = G.INLINE[name]
    inst, D, nbr, _ = inline(name)
    n = D.shape[0]
    start = random_tour(n, np.random.default_rng(n))
    accepted = []
    for seed in range(20):
        ref = S3.run(D, start, nbr, 7, seed, 0, 3, W, 0, 2, max_moves=0)
        dev = inst.seg_ils3(start, 3, W, 0, 2, seed=seed, kinds=7, max_moves_per_trial=0, time_limit=LIMIT)
        _same("seg_ils3", dev, ref)
        assert dev[3]["decisions"] == dev[3]["moves"] == 0
        accepted.append(ref[2]["accepted"])
        if seed % 5 == 0 or name.startswith("far"):
            ref = SL.run(D, start, nbr, 15, seed, 0, 3, 16, 2, W, 0, 2, max_moves=0)
            _same("seg_ils_lk", inst.seg_ils_lk(start, 3, 15, 16, 2, W, 0, 2, seed=seed, max_moves=0, time_limit=LIMIT), ref)
    windows = n // W
    assert min(accepted) < 6 * windows and max(accepted) > 0 and 0 < sum(accepted) < 20 * 6 * windows, accepted
