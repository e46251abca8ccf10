"""Records tests/golden/ils_runs.json: chains of tests/ils_ref.py (the stream, the kick and the accept rule on top of
nl3_opt_ref.descent) for the host-library test of tests/test_gpu_ils.py and for tests/test_cpu_ils.py, which runs the reference
again: start, parameters, final tour, cost, counters.  pr299 from the greedy tour over K = 5 nearest lists, chains 0 .. 2 of
seed 123 (what HEU_ils_greedy runs with tsp_host_set_ils(10, 50, 3)); att48 from a random tour, window 30.
Run from the repository root: python tests/golden/make_golden_ils.py"""
import json
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# name, K (nearest lists), start, seed, chain, iterations, span, kinds
RUNS = [("pr299", 5, "greedy", 123, b, 10, 50, 7) for b in range(3)] + [("att48", 5, "random", 7, 0, 40, 30, 7)]


def start_tour(name, start):
    from helpers import load_instance, random_tour
    from oracle import oracle as O
    xy, wt = load_instance(name)
    if start == "greedy":
        return O.greedy(xy, wt)[1]
    return random_tour(len(xy), np.random.default_rng(7))


def run(r):
    import ils_ref as IR
    import nl_opt_ref as NL
    from helpers import load_instance
    from oracle import oracle as O
    name, K, start, seed, b, iterations, span, kinds = r
    xy, wt = load_instance(name)
    D = O.dist_matrix(xy, wt, 1)
    succ, cost, st = IR.chain(D, start_tour(name, start), NL.knn(D, K), kinds, seed, b, iterations, span)
    return {"name": name, "K": K, "start": start, "seed": seed, "chain": b, "iterations": iterations, "span": span, "kinds": kinds,
            "succ": [int(v) for v in succ], "cost": cost, "stats": st}


def main():
    with mp.Pool(min(4, os.cpu_count() or 1)) as pool:
        out = pool.map(run, RUNS, chunksize=1)
    with open(os.path.join(HERE, "ils_runs.json"), "w") as f:
        json.dump({"runs": out}, f, separators=(",", ":"), sort_keys=True)
    for r in out:
        print(r["name"], r["chain"], r["cost"], r["stats"]["accepted"], r["stats"]["last_improved"])


if __name__ == "__main__":
    main()
