"""Candidate-list 3-opt: tsp_dev_nl_3opt with all three kinds (kinds 7) against the 2-opt + Or-opt descent
(kinds 3, which follows tsp_dev_nl_opt move for move) from the same greedy tour, over K = 5 alpha lists (zero penalties) and
K = 10 nearest-neighbour lists.  Writes profiles/nl3_time.txt (or the file given with --out).  --limit S: time limit of a descent."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import rand_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nl3_time.txt"))
    ap.add_argument("--sizes", default="10000,20011,50000,100003")
    ap.add_argument("--limit", type=float, default=300.0)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = E.Context(0)
    for n in [int(x) for x in a.sizes.split(",")]:
        xy = rand_instance(n)
        inst = E.Instance(ctx, xy, E.EUC_2D, 1)
        succ, obj, _ = inst.construct(E.GREEDY, np.array([0], dtype=np.int32))
        for lists, K in (("alpha", 5), ("knn", 10)):
            if lists == "alpha":
                _, ast = inst.alpha_build(K, want_stats=True)
                build_ms = ast["device_ms"]
            else:
                build_ms = inst.knn_build(K)
            cost = {}
            for kinds in (3, 7):
                rc, s, o, st = inst.nl_3opt(succ[0], kinds=kinds, time_limit=a.limit)
                cost[kinds] = o
                say("n=%-7d %-5s K=%-2d kinds=%d rc=%d %10.1f ms device  %7d moves (%d 2-opt, %d Or-opt, %d 3-opt by type %s)  "
                    "%.1f us/decision  %.3e deltas  cost %.0f -> %.0f  [lists %.1f ms]"
                    % (n, lists, K, kinds, rc, st["device_ms"], st["moves"], st["moves_2opt"], st["moves_oropt"], st["moves_3opt"],
                       st["moves_by_type"], 1e3 * st["device_ms"] / max(1, st["decisions"]), st["deltas_executed"], obj[0], o,
                       build_ms))
            say("n=%-7d %-5s K=%-2d cost(kinds 7) / cost(kinds 3) = %.4f" % (n, lists, K, cost[7] / cost[3]))
        inst.close()
    ctx.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
