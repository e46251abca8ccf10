"""Records tests/golden/nl_batch_runs.json: trajectories of the batched list descent's CPU reference (tests/nl_batch_ref.py, the moves
carried out by nl3_opt_ref.apply_decision; never the device) at sizes beyond the inline references of tests/test_gpu_nl_batch.py.
The cases are those of tests/nl_batch_golden_cases.py.  Every state is kept as the SHA-256 of the tour's int32 little-endian bytes,
its cost (oracle.succ_cost), the counters of tsp_nl3_opt_stats that the reference keeps and the number of moves of every decision.

A1  rand_instance(8000), K = 6, scrambled greedy start, kinds 7, max_arc 8, two rounds.  The first decision accepts A = 1425 moves
    (583 2-opt, 808 Or-opt, 34 3-opt; one arc wraps past position n - 1), more than k_nlb_apply has workgroups.  Recorded: the
    state after that decision under max_moves = A, A - 1, 1025, 1024 and 1; the states after each of the first 16 decisions (the
    time-limited run of the GPU test ends at one of them); and the descent's first THREE decisions (1425 + 282 + 83 moves, through
    max_moves = 1790), not the descent to its end: behind its fifth decision the reference finds no candidate of an arc of 8
    positions or fewer almost anywhere and carries out one fall-back move per decision, 0.6 s each here; it was stopped at 7
    minutes, ~690 decisions in, with no end in sight.
A2  rand_instance(2600), K = 8, from a random tour: the defaults (max_arc = n / 2, two rounds) capped at the moves of the first 12
    decisions, and max_arc = 2 (every decision the fall-back, the plain descent) capped at 40 moves.  Both carry out moves whose
    arcs have more than 1024 positions.
A3  u724 with non-integer costs, K = 10, from the greedy tour with the defaults to the end.

Times of the reference on the recording machine (one core): A1 24 s (about 5 s for the first decision, 0.6 s for each of the later
ones, the rest for the oracle's matrix and lists it is checked against), A2 44 s, A3 2 s; the whole recording takes 70 s.

The recorder is deterministic: it reproduces the committed file byte for byte.  Run from the repository root, on the CPU:
    python tests/golden/make_golden_nl_batch.py"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def record_a1():
    import nl_batch_golden_cases as G
    import nl_opt_ref as NL
    from oracle import oracle as O
    xy, wt, D, nbr, s0 = G.a1_instance()
    n = len(xy)
    # the distances and the lists without the matrix are the oracle's matrix and the reference's lists
    full = O.dist_matrix(xy, wt, 1)
    rows = np.arange(n)
    assert all((D[rows[r0:r0 + 500, None], rows[None, :]] == full[r0:r0 + 500]).all() for r0 in range(0, n, 500))
    assert (nbr == NL.knn(full, G.A1["K"])).all()
    del full
    prefix, per, first = [], [], None
    for moves, pos, succ, c in G.decisions(D, s0, nbr, G.A1["kinds"], G.A1["max_arc"], G.A1["rounds"], G.A1_PREFIX):
        assert moves
        if first is None:
            first = (moves, pos)
        per.append(len(moves))
        prefix.append(G.state(xy, wt, 1, succ, c, per))
    moves, pos = first
    A = len(moves)
    by_kind = [sum(1 for m in moves if m[1] == k) for k in range(3)]
    wraps = G.wraps(moves, pos, n)
    assert A >= G.A1_MIN_MOVES and all(by_kind) and wraps >= 1, (A, by_kind, wraps)
    caps = {}
    for cap, (succ, c) in G.capped(s0, moves, set(G.a1_caps(A))).items():
        caps[str(cap)] = G.state(xy, wt, 1, succ, c, [cap])
    assert caps[str(A)] == prefix[0]
    three = dict(prefix[G.A1_THREE - 1], decisions=G.A1_THREE, max_moves=sum(per[:G.A1_THREE]))
    return {"params": dict(G.A1, wt="EUC_2D", integer_cost=1), "lists_sha": G.sha(nbr), "start_sha": G.sha(s0), "A": A,
            "first": {"by_kind": by_kind, "wraps": wraps}, "caps": caps, "prefix": prefix, "descent": three}


def record_a2():
    import nl_batch_golden_cases as G
    xy, wt, D, nbr, s0 = G.a2_instance()
    n = len(xy)
    out = {"params": dict(G.A2, wt="EUC_2D", integer_cost=1), "lists_sha": G.sha(nbr), "start_sha": G.sha(s0)}
    for name, max_arc, rounds, limit in (("default", n // 2, 2, G.A2_DECISIONS),
                                         ("plain", G.A2_PLAIN["max_arc"], G.A2_PLAIN["rounds"], G.A2_PLAIN["max_moves"])):
        per, long_arcs = [], 0
        for moves, pos, succ, c in G.decisions(D, s0, nbr, G.A2["kinds"], max_arc, rounds, limit):
            assert moves and (name == "default" or len(moves) == 1)
            per.append(len(moves))
            long_arcs += G.long_arcs(moves, pos, n, G.A2_LONG)
        assert long_arcs >= 1 and len(per) == limit
        out[name] = dict(G.state(xy, wt, 1, succ, c, per), max_arc=max_arc, rounds=rounds, max_moves=sum(per), long_arcs=long_arcs)
    assert out["plain"]["max_moves"] == G.A2_PLAIN["max_moves"]
    return out


def record_a3():
    import nl_batch_golden_cases as G
    xy, wt, D, nbr, s0 = G.a3_instance()
    per = []
    for moves, pos, succ, c in G.decisions(D, s0, nbr, G.A3["kinds"], len(xy) // 2, 2, 10 ** 9):
        per.append(len(moves))
    assert per[-1] == 0 and max(per) > 1
    return {"params": dict(G.A3, integer_cost=0), "lists_sha": G.sha(nbr), "start_sha": G.sha(s0),
            "descent": G.state(xy, wt, 0, succ, c, per)}


def main():
    import nl_batch_golden_cases as G
    out = {}
    for name, record in (("A1", record_a1), ("A2", record_a2), ("A3", record_a3)):
        t0 = time.time()
        out[name] = record()
        print("%s: %.0f s" % (name, time.time() - t0))
    with open(os.path.join(HERE, G.FIXTURE), "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
    print("A = %d, moves of A1's decisions: %s" % (out["A1"]["A"], out["A1"]["prefix"][-1]["decision_moves"]))


if __name__ == "__main__":
    main()
