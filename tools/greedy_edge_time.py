"""Greedy-edge construction: build time, rounds and rows scanned per node on rand10000 ... rand200000, and what
the start is worth: tour cost, and the moves and device time of nl_3opt (KNN-10 lists) to a local optimum, from the greedy-edge
tour against HEU_greedy's nearest-neighbour tour from node 0.  Writes profiles/greedy_edge_time.txt (or the file given with
--out)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import rand_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greedy_edge_time.txt"))
    ap.add_argument("--sizes", default="10000,20011,50000,100003,200000")
    ap.add_argument("--descent-max-n", type=int, default=200000, help="no descents above this size")
    ap.add_argument("--time-limit", type=float, default=120.0, help="per descent, seconds")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = E.Context(0)
    for n in [int(x) for x in a.sizes.split(",")]:
        name = "rand%d" % n
        inst = E.Instance(ctx, rand_instance(n), E.EUC_2D, 1)
        inst.greedy_edge()   # warm: code objects, scratch
        best = None
        for _ in range(3):
            ge_succ, ge_cost, st = inst.greedy_edge(want_stats=True)
            if best is None or st["device_ms"] < best["device_ms"]:
                best = st
        inst.construct(E.GREEDY, np.array([0], dtype=np.int32))   # warm
        t0 = time.perf_counter()
        succ, obj, _ = inst.construct(E.GREEDY, np.array([0], dtype=np.int32))
        nn_s = time.perf_counter() - t0
        nn_succ, nn_cost = succ[0], float(obj[0])
        say("greedy_edge %-10s %9.3f ms device (%.4f s wall)  %3d rounds  %.2f n rows scanned  %.3e distances/s  at most %d edges in a "
            "round  cost %.0f = %.4f x HEU_greedy's %.0f (%.4f s wall)"
            % (name, best["device_ms"], best["seconds"], best["rounds"], best["rows_scanned"] / n,
               best["dists_executed"] / best["device_ms"] * 1e3, best["max_edges_in_round"], ge_cost, ge_cost / nn_cost, nn_cost, nn_s))
        if n > a.descent_max_n:
            inst.close()
            continue
        knn_ms = inst.knn_build(10)
        inst.nl_3opt(nn_succ, max_moves=4)   # warm
        for what, start, cost0 in (("HEU_greedy", nn_succ, nn_cost), ("greedy_edge", ge_succ, ge_cost)):
            rc, _, cost, d = inst.nl_3opt(start, time_limit=a.time_limit)
            say("nl_3opt     %-10s from %-11s %10.1f ms device  %7d moves  cost %.0f -> %.0f  (KNN-10 %.3f ms)%s"
                % (name, what, d["device_ms"], d["moves"], cost0, cost, knn_ms, "  TIME LIMIT" if rc else ""))
        inst.close()
    ctx.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
