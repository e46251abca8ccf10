"""Records tests/golden/nl3_descents.json: descents of tests/nl3_opt_ref.py (2-opt and Or-opt from the masked delta matrices of
nl_opt_ref, the 3-opt kind from the walk over the list entries, which tests/test_cpu_nl3_opt.py holds against the brute force
over all triples) that tests/test_gpu_nl3_opt.py compares the device with: pr299 over its K = 5 alpha lists (zero penalties)
and its K = 10 nearest-neighbour lists, kinds 4 and 7, from the greedy tour and from a random tour, each to its end.  The lists
are recorded with them.  Run from the repository root: python tests/golden/make_golden_nl3.py"""
import json
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

NAME = "pr299"
LISTS = (("alpha", 5), ("knn", 10))
KINDS = (4, 7)


def case_key(lists, K, kinds, start):
    return "%s|%d|%d|%s" % (lists, K, kinds, start)


def start_tour(kinds, K, start):
    from helpers import load_instance, random_tour
    from oracle import oracle as O
    xy, wt = load_instance(NAME)
    if start == "greedy":
        return O.greedy(xy, wt)[1]
    return random_tour(len(xy), np.random.default_rng(K * 8 + kinds))


def build_lists(D, lists, K):
    import alpha_ref as AR
    import nl_opt_ref as NL
    if lists == "knn":
        return NL.knn(D, K)
    A, Wt, _ = AR.alpha_rows(D, None)
    return AR.lists(A, Wt, np.arange(len(D)), K)[0]


def run(case):
    import nl3_opt_ref as N3
    from helpers import load_instance
    from oracle import oracle as O
    lists, K, kinds, start = case
    xy, wt = load_instance(NAME)
    D = O.dist_matrix(xy, wt, 1)
    succ, c = N3.descent(D, start_tour(kinds, K, start), build_lists(D, lists, K), kinds)
    return case_key(*case), {"succ": [int(v) for v in succ], "counters": c, "cost": O.succ_cost(xy, wt, succ)}


def main():
    from helpers import load_instance
    from oracle import oracle as O
    xy, wt = load_instance(NAME)
    D = O.dist_matrix(xy, wt, 1)
    cases = [(ls, K, kinds, st) for ls, K in LISTS for kinds in KINDS for st in ("greedy", "random")]
    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        out = dict(pool.map(run, cases, chunksize=1))
    nbrs = {"%s|%d" % (ls, K): build_lists(D, ls, K).tolist() for ls, K in LISTS}
    with open(os.path.join(HERE, "nl3_descents.json"), "w") as f:
        json.dump({"lists": nbrs, "cases": out}, f, separators=(",", ":"), sort_keys=True)
    print(len(out), "cases")


if __name__ == "__main__":
    main()
