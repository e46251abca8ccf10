"""Records tests/golden/dlb_runs.json: chains of tests/dlb_ref.py (ils_ref's stream, kick and accept rule over descents with
don't-look bits) for tests/test_gpu_dlb.py, which reads only the JSON, and for tests/test_cpu_dlb.py, which runs the reference
again: parameters, final tour, cost, counters.  pr299 from the greedy tour over K = 5 nearest lists, all three kinds, chain 0 of
seed 123, 10 iterations within 50 nodes, modes TSP_DLB_ON and TSP_DLB_CLOSE.
Run from the repository root: python tests/golden/make_golden_dlb.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# name, K (nearest lists), seed, iterations, span, mode
RUNS = [("pr299", 5, 123, 10, 50, 1), ("pr299", 5, 123, 10, 50, 2)]


def run(r):
    import dlb_ref as DR
    import nl_opt_ref as NL
    from helpers import load_instance
    from oracle import oracle as O
    name, K, seed, iterations, span, mode = r
    xy, wt = load_instance(name)
    D = O.dist_matrix(xy, wt, 1)
    succ, cost, st = DR.chain(D, O.greedy(xy, wt)[1], NL.knn(D, K), 7, seed, 0, iterations, span, mode=mode)
    return {"name": name, "K": K, "seed": seed, "iterations": iterations, "span": span, "mode": mode,
            "succ": [int(v) for v in succ], "cost": cost, "stats": st}


def main():
    out = [run(r) for r in RUNS]
    with open(os.path.join(HERE, "dlb_runs.json"), "w") as f:
        json.dump({"runs": out}, f, separators=(",", ":"), sort_keys=True)
    for r in out:
        print(r["name"], r["mode"], r["cost"], r["stats"]["accepted"], r["stats"]["decisions"], r["stats"]["active_nodes"])


if __name__ == "__main__":
    main()
