#!/usr/bin/env python3
"""Trajectories of tabu() (src/tabusearch.c:188-320) too slow to compute inside a GPU test (an iteration of the oracle takes
0.2 s at pr1002, 1-2 s at n = 3000): about ten minutes of CPU for the whole file.

* cases: tests/tabu_ref.replay (the oracle's alg_2opt_tabu + the restated kick) from greedy(0) + alg_2opt, over a seeded
  stream of node pairs and one tenure per iteration -- per iteration the cost after the descent, whether the incumbent
  improved and the number of kick trials; at checkpoints the tour's hash, the non-zero stamps and the incumbent's hash; at the
  last one the tour and the incumbent themselves.  The start tour and the pairs are stored, so the GPU test computes nothing.
* host_runs: O.tabu after 300 iterations of the libc stream seeded with 123, from greedy_iter + alg_2opt: incumbent, cost,
  moves and the next value of random() after the run.

Provenance: every number written here comes from oracle/tsp_oracle.c and tests/tabu_ref.py; nothing is taken from the device.
tests/test_cpu_tabu_ref.py pins tabu_ref.replay to O.tabu and regenerates a prefix of this file."""
import ctypes as C
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import oracle as O  # noqa: E402
from helpers import load_instance  # noqa: E402
import tabu_ref as T  # noqa: E402
import tabu_cases as TC  # noqa: E402

LOOKAHEAD = 256 + 8      # pairs kept behind the last one the trajectory takes: a chain is handed up to 256 at a time


def make_case(case, iterations=None, check=True):
    """The record of one case; iterations: a prefix of the case's run (the freshness test)"""
    xy, wt, ic = TC.instance_of(case)
    n = len(xy)
    full = TC.CASES[case][2]
    iterations = full if iterations is None else iterations
    _, g, gobj = O.greedy(xy, wt, integer_cost=ic)
    _, s0, o0, _, _ = O.two_opt_first(xy, wt, g, gobj, integer_cost=ic)
    tenures = TC.tenures_of(case, n, full)[:iterations]
    stream = T.pair_stream(n, TC.CASES[case][4], 4 * full + LOOKAHEAD)
    cps = TC.checkpoints_of(iterations)
    r = T.replay(xy, wt, ic, s0, o0, None, 1, tenures, stream, snaps=cps)
    assert r.accepted and len(r.obj) == iterations and r.consumed + LOOKAHEAD <= len(stream)
    if check:
        many = sum(1 for t in r.trials if t > 1)
        assert 20 * many >= iterations, (case, many)                      # >= 5 % of the iterations take more than one trial
        assert any(r.improved[1:]), case                                  # the incumbent improves after iteration 1
    best_after = {k + 1: r.best[k] for k in range(iterations)}
    checkpoints = []
    for c in cps:
        tour, (idx, val), inc = r.snaps[c]
        checkpoints.append({"iteration": c, "tour_hash": O.fnv1a(tour), "stamps": [idx.tolist(), val.tolist()],
                            "best": best_after[c], "incumbent_hash": O.fnv1a(T.canonical_cycle(inc))})
    rec = {"n": n, "wtype": wt, "integer_cost": ic, "iterations": iterations, "tenures": [int(t) for t in tenures],
           "start": s0.tolist(), "start_cost": o0, "pairs": stream[:r.consumed + LOOKAHEAD].tolist(), "consumed": r.consumed,
           "obj": r.obj, "improved": [int(b) for b in r.improved], "trials": r.trials, "checkpoints": checkpoints,
           "tour": r.tour.tolist(), "incumbent": r.inc.tolist(), "incumbent_cost": r.inc_cost}
    print("%s: n %d, %d iterations, %d pairs, %d iterations with further trials, %d improvements, incumbent %.0f"
          % (case, n, iterations, r.consumed, sum(1 for t in r.trials if t > 1), sum(r.improved), r.inc_cost), flush=True)
    return rec


def make_host_run(name, policy):
    libc = C.CDLL(None)
    libc.random.restype = C.c_long
    xy, wt = load_instance(name)
    _, s0, o0 = O.greedy_iter(xy, wt)
    _, s1, o1, _, _ = O.two_opt_first(xy, wt, s0, o0)
    O.srandom(123)
    es, eo, moves = O.tabu(xy, wt, s1, o1, TC.HOST_ITERATIONS, policy)
    nxt = int(libc.random())
    print("host run %s policy %d: incumbent %.0f, %d moves" % (name, policy, eo, moves), flush=True)
    return {"instance": name, "policy": policy, "iterations": TC.HOST_ITERATIONS, "seed": 123, "incumbent": es.tolist(), "cost": eo,
            "moves": int(moves), "next_random": nxt}


def main():
    out = {"_source": "oracle/tsp_oracle.c + tests/tabu_ref.py via tests/golden/make_golden_tabu.py (oracle-derived; nothing from the device)"}
    with ProcessPoolExecutor(max_workers=min(9, os.cpu_count() or 1)) as ex:   # (a process each: libc's random() is per process)
        cases = {c: ex.submit(make_case, c) for c in TC.CASES}
        hosts = [ex.submit(make_host_run, nm, pol) for nm, pol in TC.HOST_RUNS]
        out["cases"] = {c: f.result() for c, f in cases.items()}
        out["host_runs"] = [f.result() for f in hosts]
    with open(os.path.join(HERE, "tabu_chains.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote tabu_chains.json")


if __name__ == "__main__":
    main()
