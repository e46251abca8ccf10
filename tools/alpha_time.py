"""Alpha-nearness candidate lists: build time and pair rate beside k_knn_scan's from the same run, and the
neighbour-list descent from the greedy tour on KNN-10, alpha-5 and alpha-8 lists (pi = 0 and pi_best after 50 and 300 ascent
iterations, the ascent's time listed separately).  Writes profiles/alpha_time.txt (or the file given with --out)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import load_instance, rand_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alpha_time.txt"))
    ap.add_argument("--sizes", default="1002,10000,20011,100003")
    ap.add_argument("--ascents", default="0,50,300")
    ap.add_argument("--time-limit", type=float, default=120.0, help="per descent, seconds")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = E.Context(0)
    for n in [int(x) for x in a.sizes.split(",")]:
        xy, wt = load_instance("pr1002") if n == 1002 else (rand_instance(n), E.EUC_2D)
        name = "pr1002" if n == 1002 else "rand%d" % n
        inst = E.Instance(ctx, xy, wt, 1)
        succ, obj, _ = inst.construct(E.GREEDY, np.array([0], dtype=np.int32))
        start, ub = succ[0], float(obj[0])
        inst.alpha_build(5)   # warm: code objects, scratch
        tree_ms = min(inst.one_tree(want_stats=True)[3]["device_ms"] for _ in range(3))
        best = None
        for _ in range(3):
            st = inst.alpha_build(5, want_stats=True)[1]
            if best is None or st["device_ms"] < best["device_ms"]:
                best = st
        knn_ms = min(inst.knn_build(16) for _ in range(3))
        alpha_ms = best["device_ms"] - tree_ms
        say("alpha_build %-10s %9.3f ms device (%.3f ms of it the 1-tree, %d rounds), scan + merge %.3e pairs/s; k_knn_scan + merge "
            "%.3f ms = %.3e pairs/s (%.2f x)"
            % (name, best["device_ms"], tree_ms, best["rounds"], n * (n - 1.0) / max(alpha_ms, 1e-6) * 1e3, knn_ms,
               n * (n - 1.0) / knn_ms * 1e3, knn_ms / max(alpha_ms, 1e-6)))
        inst.knn_build(10)
        inst.nl_opt(start, max_moves=4)   # warm
        rc, _, cost, st = inst.nl_opt(start, time_limit=a.time_limit)
        say("nl_opt      %-10s KNN-10            %10.1f ms device  %7d moves  cost %.0f (greedy %.0f)%s"
            % (name, st["device_ms"], st["moves"], cost, ub, "  TIME LIMIT" if rc else ""))
        for iters in [int(x) for x in a.ascents.split(",")]:
            pi, asc_ms, bound = None, 0.0, float("nan")
            if iters:
                bound, pi, hs = inst.held_karp(ub, max_iters=iters)
                asc_ms = hs["device_ms"]
            for K in (5, 8):
                ast = inst.alpha_build(K, pi, want_stats=True)[1]
                rc, _, cost, st = inst.nl_opt(start, time_limit=a.time_limit)
                say("nl_opt      %-10s alpha-%d pi@%-3d     %10.1f ms device  %7d moves  cost %.0f  (lists %.3f ms, ascent %.1f ms, bound %.1f)%s"
                    % (name, K, iters, st["device_ms"], st["moves"], cost, ast["device_ms"], asc_ms, bound, "  TIME LIMIT" if rc else ""))
        inst.close()
    ctx.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
