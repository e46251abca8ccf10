"""Neighbour-list descent: the KNN build and tsp_dev_nl_opt against the exhaustive 2-opt + Or-opt route.
Writes profiles/nl_time.txt (or the file given with --out).  --parent-limit S: time limit of the exhaustive route's runs."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import rand_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402

OR_SCAN_RATE = 2.5e12   # k_or_scan's delta expressions per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nl_time.txt"))
    ap.add_argument("--sizes", default="10000,20011,50000,100003,200000")
    ap.add_argument("--parent-sizes", default="10000,20011,50000,100003,200000")
    ap.add_argument("--parent-limit", type=float, default=300.0)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = E.Context(0)
    parent = {int(x) for x in a.parent_sizes.split(",") if x}
    for n in [int(x) for x in a.sizes.split(",")]:
        xy = rand_instance(n)
        inst = E.Instance(ctx, xy, E.EUC_2D, 1)
        succ, obj, _ = inst.construct(E.GREEDY, np.array([0], dtype=np.int32))
        for K in (16, 10):
            inst.knn_build(K)                       # warm
            ms = min(inst.knn_build(K) for _ in range(3))
            rate = n * (n - 1.0) / (ms * 1e-3)
            say("knn_build  n=%-7d K=%-2d %9.3f ms  %.3e distances/s  (%.2f x k_or_scan's %.1e deltas/s)"
                % (n, K, ms, rate, rate / OR_SCAN_RATE, OR_SCAN_RATE))
        knn_ms = ms
        rc, s, o, st = inst.nl_opt(succ[0], time_limit=600.0)
        say("nl_opt     n=%-7d K=10 rc=%d %10.1f ms device  %7d moves (%d 2-opt, %d Or-opt)  %.1f us/decision  cost %.0f -> %.0f"
            "  [knn + descent %.1f ms]"
            % (n, rc, st["device_ms"], st["moves"], st["moves_2opt"], st["moves_oropt"], 1e3 * st["device_ms"] / max(1, st["decisions"]),
               obj[0], o, knn_ms + st["device_ms"]))
        if n in parent:
            rc2, s2, o2, st2, sto = inst.two_opt_or_opt(succ[0], obj[0], mode=E.FIRST, time_limit=a.parent_limit)
            say("two_opt_or_opt n=%-7d rc=%d %10.1f + %.1f ms device  %.2f s wall  cost %.0f  (lists / exhaustive cost = %.4f)"
                % (n, rc2, st2["device_ms"], sto["device_ms"], sto["seconds"], o2, o / o2))
        inst.close()
    ctx.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
