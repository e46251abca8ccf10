"""CPU: tests/golden/seg_runs.json cannot drift from the references that recorded it (tests/seg_ils_ref.py, seg_ils3_ref.py,
seg_groups_ref.py, seg_lk_ref.py through tests/seg_golden_cases.py): the fixture's own numbers meet the conditions that make its
cases worth their name, every state's counters are consistent, the cheap records are recomputed here (the long run of kroA100 up to
252 iterations, one iteration of the 78 windows at once, the lists and the start tour of every instance), and the far instances
of tests/test_gpu_seg_golden.py tell the window cost's order of summation from another one."""
import numpy as np
import pytest

import seg_golden_cases as G
import seg_ils_ref as SR
import seg_lk_ref as SL
from helpers import golden, random_tour
from oracle import oracle as O


@pytest.fixture(scope="module")
def runs():
    return golden(G.FIXTURE)


def test_the_fixture_meets_the_conditions_of_its_cases(runs):
    assert sorted(runs["runs"]) == sorted(G.RUNS) and sorted(runs["instances"]) == sorted(G.INSTANCES)
    for name, r in runs["runs"].items():
        assert {k: r[k] for k in G.RUNS[name]} == G.RUNS[name], name
        assert sorted(int(k) for k in r["states"]) == sorted(r["iterations"]), name
    R = runs["runs"]
    big = G.THREADS
    # S1: one window of 1024 through four instantiations of k_seg_ils, and the chain kind alone
    s1 = {name: r for name, r in R.items() if r["case"] == "S1"}
    assert sorted((r["entry"], r["kinds"], r["groups"]) for r in s1.values() if r["trials"] == 1) == \
        [("seg_ils", 3, 1), ("seg_ils3", 7, 1), ("seg_ils_groups", 7, 2), ("seg_ils_lk", 8, 1), ("seg_ils_lk", 15, 1)]
    for name, r in s1.items():
        w, c = r["worth"], r["states"]["1"]["counters"]
        assert (r["window"], r["span"], r["max_moves"], r["instance"], r["trials"]) == (1024, 0, -1, "r1100", 1)
        assert w["max_active"] > big and c["windows"] == 1 and c["accepted"] >= 1, name
        assert w["max_rev2"] > big or not r["kinds"] & 1, name
        assert w["max_span3"] > big or not r["kinds"] & 4, name
        if r["kinds"] & 8:
            assert w["max_hull_lk"] > big and w["partial_chain_pass"] and r["depth"] == 16, name
    # S2: the largest window to the end
    r = R["S2-lk"]
    assert (r["window"], r["max_moves"], r["kinds"], r["depth"]) == (SR.MAX_WINDOW, -1, 15, 16)
    assert r["worth"]["max_active"] > 1024 and max(r["worth"][k] for k in ("max_rev2", "max_span3", "max_hull_lk")) > 1024
    # S3: many windows at once without groups
    for name in ("S3-ils", "S3-ils3"):
        r = R[name]
        assert r["groups"] == 1 and r["iterations"] == [1, 2, 3] and r["worth"]["straddles"]
        assert all(2 * a > 78 for a in r["worth"]["accepting_windows"]) and len(r["worth"]["accepting_windows"]) == 3
        assert all(s["counters"]["windows"] == 78 for s in r["states"].values())
    # S4: groups, and more workgroups than are resident
    # the restore branch at full length: hulls of more than 256 slots whose far part the group's next trial reads
    w = R["S4-lk-w1024-span0"]["worth"]
    assert R["S4-lk-w1024-span0"]["trials"] == 4 and w["long_restores_read_by_the_next_trial"] >= 2
    assert w["longest_restore_hull"] > big and w["restored_slots_read_by_the_next_trial"] >= 2
    for name in ("S4-groups", "S4-lk", "S4-lk-w1024", "S4-lk-w1024-span0", "S4-lk-w256"):
        r = R[name]
        c = r["states"][str(r["iterations"][0])]["counters"]
        assert c["commits"] < c["offers"] and r["worth"]["workgroups"] == c["windows"] * c["groups"]
        assert r["worth"]["most_commits_of_a_window"] >= 2 or r["window"] == 1024
        assert r["worth"]["commits_behind_the_first_window_and_group"] >= 1
    assert R["S4-groups"]["worth"]["workgroups"] == R["S4-lk"]["worth"]["workgroups"] == 1248 > G.RESIDENT
    assert (R["S4-lk-w1024"]["window"], R["S4-lk-w1024"]["groups"], R["S4-lk-w1024"]["trials"]) == (1024, 16, 4)
    # S5: past the second batch of 256 launches, and a search that has run dry
    for name in ("S5-lk", "S5-groups"):
        r = R[name]
        assert max(r["iterations"]) == 640 > G.BATCH_ENDS[7] and {6, 252, 253, 300, 509} <= set(r["iterations"])
        c = r["states"]["640"]["counters"]
        per = c["windows"] * c["groups"] * r["trials"]
        assert 10 * r["worth"]["accepted_behind_%d" % G.S5_DRY_FROM] < (640 - G.S5_DRY_FROM) * per
        acc = [r["states"][str(it)]["counters"]["accepted"] for it in sorted(r["iterations"])]
        assert acc == sorted(acc)                     # a longer call is the shorter one and more
    b, ends = 4, [1]
    while ends[-1] < 640:
        ends.append(ends[-1] + b)
        b = min(2 * b, 256)
    assert tuple(ends) == G.BATCH_ENDS


def test_every_state_is_consistent(runs):
    seen = 0
    for name, r in runs["runs"].items():
        starts = set()
        for it, s in r["states"].items():
            assert sorted(s) == ["cost", "counters", "sha", "start_cost"] and len(s["sha"]) == 64
            assert sorted(s["counters"]) == sorted(G.counters_of(r["entry"]))
            G.consistent(r["entry"], s["counters"], int(it), r["trials"])
            assert s["cost"] < s["start_cost"] and s["counters"]["accepted"] > 0
            starts.add(s["start_cost"])
            seen += 1
        assert len(starts) == 1
    assert seen == sum(len(r["iterations"]) for r in G.RUNS.values())


@pytest.mark.parametrize("name", list(G.INSTANCES))
def test_the_lists_and_the_start_of_an_instance(runs, name):
    rec = runs["instances"][name]
    xy, wt, D, nbr, start = G.instance(name)
    assert {k: rec[k] for k in G.INSTANCES[name]} == G.INSTANCES[name]
    assert G.sha(nbr) == rec["lists_sha"] and G.sha(start) == rec["start_sha"] and O.is_tour(start)
    for r in runs["runs"].values():
        if r["instance"] == name:
            assert all(s["start_cost"] == O.succ_cost(xy, wt, start, rec["integer_cost"]) for s in r["states"].values())


def _recompute(runs, name, iterations):
    r = runs["runs"][name]
    xy, wt, D, nbr, start = G.instance(r["instance"])
    for it in iterations:
        succ, cost, c = G.ref_run(r, D, start, nbr, it)
        assert G.state(xy, wt, runs["instances"][r["instance"]]["integer_cost"], r["entry"], succ, c) == r["states"][str(it)], (name, it)


def test_the_long_run_is_the_references_up_to_252_iterations(runs):
    _recompute(runs, "S5-lk", [6, G.S5_CPU])
    _recompute(runs, "S5-groups", [6, 29])


def test_one_iteration_of_78_windows_is_the_references(runs):
    _recompute(runs, "S3-ils", [1])


def test_the_probe_leaves_the_references_as_they_were():
    before = (SR.window_candidates, SR.apply_window_move, SR.kick, SR.trial, SL.trial)
    xy, wt, D, nbr, start = G.instance("kroA100")
    r = G.RUNS["S5-lk"]
    plain = G.ref_run(r, D, start, nbr, 3)
    log = []
    with G.probe() as seen:
        probed = G.ref_run(r, D, start, nbr, 3, log=log)
    assert (SR.window_candidates, SR.apply_window_move, SR.kick, SR.trial, SL.trial) == before
    assert (plain[0] == probed[0]).all() and plain[1:] == probed[1:]
    assert len(seen["accepts"]) == len(seen["kick"]) == plain[2]["trials"] and sum(seen["accepts"]) == plain[2]["accepted"]
    assert sum(seen["active"]) == plain[2]["active_nodes"] == sum(G.lk_log_sizes(log)[0])
    assert sum(seen["rev2"]) == plain[2]["reversed"] and len(seen["span3"]) == plain[2]["moves_3opt"]



def test_the_stale_slots_of_a_restore():
    seq = list(range(600))
    fin = seq[:10] + seq[10:500][::-1] + seq[500:]
    hull, stale = G.stale_slots(seq, fin)
    assert hull == 490 and stale == set(range(10 + G.THREADS, 500))
    assert G.stale_slots(seq, seq) == (0, set())
    assert G.stale_slots(seq, seq[:10] + seq[10:200][::-1] + seq[200:]) == (190, set())


@pytest.mark.parametrize("name", ["far600", "far1100"])
def test_a_far_node_tells_the_order_of_the_window_cost_from_another(monkeypatch, name):
    """the kick-alone calls that tests/test_gpu_seg_golden.py compares the device with change when the window cost is folded over
    neighbouring pairs: a kernel that summed in that order would not pass them"""
    W = G.INLINE[name][3]
    xy, wt, _ = G.inline_instance(name)
    D = O.dist_matrix(xy, wt, 0)
    nbr = G.NL.knn(D, G.INLINE[name][2])
    n = len(xy)
    start = random_tour(n, np.random.default_rng(n))
    seq = SR.walk(start, 0, W)
    assert G.window_cost_pairs(D, seq) == pytest.approx(SR.window_cost(D, seq), rel=1e-9)
    want = G.kick_runs(D, nbr, start, W)
    monkeypatch.setattr(SR, "window_cost", G.window_cost_pairs)
    other = G.kick_runs(D, nbr, start, W)
    differ = sum(1 for a, b in zip(want, other) if not (a[0] == b[0]).all() or a[2] != b[2])
    accepted = [a[2]["accepted"] for a in want]
    assert differ >= 5 and min(accepted) < 6 and max(accepted) > 0, (differ, accepted)
