"""CPU: tests/tabu_ref.replay (the reference of a run of tabu() iterations) and tests/golden/tabu_chains.json.

replay is pinned to the oracle's own tabu() loop (O.tabu, which draws from libc inside the loop) by feeding it libc's stream as
pairs; the committed file is regenerated in part; and what the generator asserts about its cases is checked on the file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O
from helpers import golden, load_instance, GOLDEN
import tabu_cases as TC
import tabu_ref as T

G = golden("tabu_chains.json")


def _initial(xy, wt):
    """What tabu() starts from: HEU_2opt_greedy_iter (tabusearch.c:200)"""
    _, s0, o0 = O.greedy_iter(xy, wt)
    _, s1, o1, _, _ = O.two_opt_first(xy, wt, s0, o0)
    return s1, o1


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("name", ["berlin52", "att48", "pr299"])
def test_replay_on_libcs_stream_is_the_oracles_tabu(name, policy):
    """150 iterations: the pairs are libc's draws after srandom(123), mapped as rand_choice does ((int)(raw / RAND_MAX * n)), the
    tenures those of the step and linear policies.  Same incumbent and cost as O.tabu; and after as many draws as the replay
    took pairs, libc's next value is the one that follows O.tabu's run -- the replay takes the reference's draws, in its order.
    (The random policy draws inside the loop; it is pinned at the host level by the committed runs.)"""
    libc = C.CDLL(None)
    libc.random.restype = C.c_long
    xy, wt = load_instance(name)
    n = len(xy)
    s1, o1 = _initial(xy, wt)
    O.srandom(123)
    es, eo, moves = O.tabu(xy, wt, s1, o1, 150, policy)
    next_oracle = libc.random()
    O.srandom(123)
    stream = np.array([[int(O.urand() * n), int(O.urand() * n)] for _ in range(1500)])
    r = T.replay(xy, wt, 1, s1, o1, None, 1, T.policy_tenures(n, policy, 150), stream)
    assert len(r.obj) == 150 and r.accepted and r.consumed < len(stream)
    assert r.inc_cost == eo and (r.inc == es).all() and moves > 0
    assert r.best[-1] == min(r.obj) and r.improved[0]
    O.srandom(123)
    for _ in range(2 * r.consumed):
        O.urand()
    assert libc.random() == next_oracle


def test_replay_does_not_depend_on_how_the_iterations_are_cut():
    """One run of 40 iterations against the same run resumed call by call from (tour, stamps, incumbent, stream position)"""
    xy, wt = load_instance("berlin52")
    n = len(xy)
    s1, o1 = _initial(xy, wt)
    tenures = [int(t) for t in np.random.default_rng(2).integers(0, 6, size=40)]
    stream = T.pair_stream(n, 9, 400)
    whole = T.replay(xy, wt, 1, s1, o1, None, 1, tenures, stream, snaps=(8,))
    tour, cost, stamps, best, inc, p, it = s1, o1, None, float("inf"), None, 0, 1
    obj, trials = [], []
    for K in (1, 7, 3, 29):
        part = T.replay(xy, wt, 1, tour, cost, stamps, it, tenures[it - 1:it - 1 + K], stream[p:], best0=best, inc0=inc)
        tour, cost, stamps, best, inc = part.tour, part.obj[-1], part.stamps, part.inc_cost, part.inc
        p += part.consumed; it += K
        obj += part.obj; trials += part.trials
        if it == 9:
            assert (tour == whole.snaps[8][0]).all() and (T.sparse(stamps)[0] == whole.snaps[8][1][0]).all()
    assert obj == whole.obj and trials == whole.trials and p == whole.consumed and max(trials) > 1
    assert (tour == whole.tour).all() and (stamps == whole.stamps).all() and (inc == whole.inc).all()
    # the stream runs out: the iteration in whose trials it does is the last, with the trials it could take
    short = T.replay(xy, wt, 1, s1, o1, None, 1, tenures, stream[:whole.consumed - 1])
    assert not short.accepted and len(short.obj) == 40 and short.trials[-1] == whole.trials[-1] - 1


def test_the_committed_att532_prefix_is_fresh():
    """The first 16 iterations of the att532 case, regenerated"""
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden_tabu as MG
    finally:
        sys.path.remove(GOLDEN)
    new, old = MG.make_case("att532", iterations=16, check=False), G["cases"]["att532"]
    for key in ("obj", "improved", "trials", "tenures"):
        assert new[key] == old[key][:16], key
    assert new["start"] == old["start"] and new["start_cost"] == old["start_cost"]
    assert new["pairs"] == old["pairs"][:len(new["pairs"])] and new["consumed"] == sum(old["trials"][:16])
    assert new["checkpoints"] == [c for c in old["checkpoints"] if c["iteration"] <= 16] and len(new["checkpoints"]) == 2


def test_the_committed_cases_meet_what_the_generator_asserts():
    assert set(G["cases"]) == set(TC.CASES)
    for case, rec in G["cases"].items():
        it = rec["iterations"]
        assert it == TC.CASES[case][2] and len(rec["obj"]) == len(rec["improved"]) == len(rec["trials"]) == len(rec["tenures"]) == it
        assert 20 * sum(1 for t in rec["trials"] if t > 1) >= it, case         # >= 5 % of the iterations take further trials
        assert any(rec["improved"][1:]), case                                   # the incumbent improves after iteration 1
        assert sum(rec["trials"]) == rec["consumed"] and len(rec["pairs"]) >= rec["consumed"] + 256
        assert any(a == b for a, b in rec["pairs"][:rec["consumed"]])
        assert [c["iteration"] for c in rec["checkpoints"]] == TC.checkpoints_of(it)
        assert rec["incumbent_cost"] == min(rec["obj"]) == rec["checkpoints"][-1]["best"]
        n = rec["n"]
        assert O.is_tour(np.array(rec["tour"])) and O.is_tour(np.array(rec["incumbent"])) and O.is_tour(np.array(rec["start"]))
        assert O.fnv1a(np.array(rec["tour"], dtype=np.int32)) == rec["checkpoints"][-1]["tour_hash"]
        lo, hi = T.tenure_bounds(n)
        if TC.CASES[case][3] == "drawn":
            assert {0, 1, 2} <= set(rec["tenures"]) and any(lo <= t <= hi for t in rec["tenures"])
        else:
            assert rec["tenures"] == T.policy_tenures(n, 1, it) and all(a != b for a, b in zip(rec["tenures"], rec["tenures"][1:]))
    # the metrics: integer coordinates (pr1002), ATT, fractional coordinates (d493), CEIL_2D
    assert (TC.instance_of("pr1002")[0] % 1 == 0).all() and (TC.instance_of("d493")[0] % 1 != 0).any()
    assert G["cases"]["att532"]["wtype"] == O.ATT and G["cases"]["ceil1500"]["wtype"] == O.CEIL_2D
    # the cluster sizes the cases get by default
    assert [TC.workgroups_natural(G["cases"][c]["n"]) for c in ("pr1002", "att532", "rand3000")] == [34, 12, 256]
    ng = (3000 + 63) // 64
    assert (ng * (ng + 1) // 2 + 3) // 4 >= 256
    assert [(r["instance"], r["policy"]) for r in G["host_runs"]] == TC.HOST_RUNS
    for r in G["host_runs"]:
        assert r["iterations"] == 300 and O.is_tour(np.array(r["incumbent"]))
        xy, wt = load_instance(r["instance"])
        assert O.succ_cost(xy, wt, np.array(r["incumbent"], dtype=np.int32)) == r["cost"]


def test_every_cut_into_calls_passes_checkpoints():
    """Each split's call boundaries contain at least three checkpoints and the last one, for every length of run; chains of the
    host's length (128) have a boundary only every 128 iterations: there every boundary is a checkpoint."""
    for it in (64, 128, 256):
        cps = TC.checkpoints_of(it)
        for split in TC.SPLITS:
            calls = TC.split_calls(split, it)
            ends = set(np.cumsum(calls).tolist())
            assert sum(calls) == it and it in ends and cps[-1] == it
            if split == "host":
                assert ends <= set(cps) and max(calls) == min(it, 128)
            else:
                assert len(ends & set(cps)) >= 3, (split, it)
            for K in calls:
                P = TC.pairs_of_call(split, K)
                assert K <= P <= 256 and (P == K) == (split == "exact")


def test_the_gpu_tests_parametrisation_covers_every_axis_with_every_case():
    import test_gpu_tabu_oracle as GT
    for case in TC.CASES:
        mine = [p for p in GT.PARAMS if p[0] == case]
        blocks = {None, 8, 64, 256} if case in ("pr1002", "att532", "d493") else {None}
        assert {p[1] for p in mine} >= {"ex", "queued", "single"} and {p[2] for p in mine} == set(TC.SPLITS)
        assert {p[3] for p in mine} == blocks and {p[4] for p in mine} == {-1.0, 600.0}
        assert {(p[3], p[4]) for p in mine if p[1] == "ex"} == {(b, tl) for b in blocks for tl in (-1.0, 600.0)}
    assert {p[0] for p in GT.PARAMS if p[1] == "grid"} == {"pr1002", "att532"}
    assert all(p[5] == 64 for p in GT.PARAMS if p[1] == "grid")
    assert os.path.getsize(os.path.join(GOLDEN, "tabu_chains.json")) < os.path.getsize(os.path.join(GOLDEN, "nl_descents.json"))   # the largest golden file before this one
