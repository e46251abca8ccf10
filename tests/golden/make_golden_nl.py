"""Records tests/golden/nl_descents.json: the descents of tests/nl_opt_ref.py (full delta matrices masked with the lists) that
tests/test_gpu_nl_opt.py compares the device with -- every kinds mask x K x {greedy start, random tour} on four instances.
Every descent runs to its end.  They take the CPU about a second per twenty decisions at n = 800, which is why they are recorded
and not recomputed next to the GPU; tests/test_cpu_nl_opt.py recomputes cases of every instance.  Run from the repository root: python tests/golden/make_golden_nl.py"""
import json
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

NAMES = ("pr299", "att532", "rat783", "rand800")
KS = (1, 3, 8, 16)
RANDOM_CAP = -1   # moves of the descents from random tours: -1 = to their end, like those from the greedy tour


def case_key(name, kinds, K, start):
    return "%s|%d|%d|%s" % (name, kinds, K, start)


def start_tour(name, kinds, K, start):
    from helpers import load_instance, random_tour
    from oracle import oracle as O
    xy, wt = load_instance(name)
    if start == "greedy":
        return O.greedy(xy, wt)[1]
    return random_tour(len(xy), np.random.default_rng(K * 8 + kinds))


def run(case):
    import nl_opt_ref as NL
    from helpers import load_instance
    from oracle import oracle as O
    name, kinds, K, start = case
    xy, wt = load_instance(name)
    D = O.dist_matrix(xy, wt, 1)
    succ, c = NL.descent(D, start_tour(*case), NL.knn(D, K), kinds, max_moves=RANDOM_CAP)
    return case_key(*case), {"succ": [int(v) for v in succ], "counters": c, "cost": O.succ_cost(xy, wt, succ)}


def main():
    cases = [(nm, kinds, K, st) for nm in NAMES for kinds in (1, 2, 3) for K in KS for st in ("greedy", "random")]
    with mp.Pool(min(32, os.cpu_count() or 1)) as pool:
        out = dict(pool.map(run, cases, chunksize=1))
    with open(os.path.join(HERE, "nl_descents.json"), "w") as f:
        json.dump({"random_cap": RANDOM_CAP, "cases": out}, f, separators=(",", ":"), sort_keys=True)
    print(len(out), "cases")


if __name__ == "__main__":
    main()
