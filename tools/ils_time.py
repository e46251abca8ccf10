"""Iterated local search: tsp_dev_ils from the greedy tour on pr1002 and rand10000, B = 1 and 64 chains, span 0
and 50, over K = 5 alpha lists (zero penalties) and K = 10 nearest-neighbour lists, each run ended by --limit seconds: iterations
per second and us per decision (five launches), beside the us per decision of tsp_dev_nl_3opt from the same tour over the same
lists (four launches: the descent without k_ils_step), and the best chain's cost over the tsp_dev_held_karp bound.  Writes
profiles/ils_time.txt (or the file given with --out).  --instances: names of tests/golden/instances or rand<n>."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import load_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ils_time.txt"))
    ap.add_argument("--instances", default="pr1002,rand10000")
    ap.add_argument("--chains", default="1,64")
    ap.add_argument("--spans", default="0,50")
    ap.add_argument("--limit", type=float, default=4.0)
    ap.add_argument("--hk-iters", type=int, default=100)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = E.Context(0)
    for name in a.instances.split(","):
        xy, wt = load_instance(name)
        n = len(xy)
        inst = E.Instance(ctx, xy, wt, 1)
        succ, obj, _ = inst.construct(E.GREEDY, np.array([0], dtype=np.int32))
        bound, _, lb = inst.held_karp(obj[0], max_iters=a.hk_iters, time_limit=60.0)
        say("%s n=%d greedy %.0f  Held-Karp bound %.1f (%d iterations, %.0f ms device)"
            % (name, n, obj[0], bound, lb["iterations"], lb["device_ms"]))
        for lists, K in (("alpha", 5), ("knn", 10)):
            if lists == "alpha":
                inst.alpha_build(K)
            else:
                inst.knn_build(K)
            for B in [int(x) for x in a.chains.split(",")]:
                starts = np.stack([succ[0]] * B)
                rc, s, o, st = inst.nl_3opt(starts, time_limit=60.0)
                dec = sum(q["decisions"] for q in st)
                say("%s %-5s K=%-2d B=%-2d nl_3opt        rc=%d %9.1f ms device %8d decisions (longest chain %d) %7.1f us/decision of the "
                    "longest chain  cost %.0f (%.4f x bound)"
                    % (name, lists, K, B, rc, st[0]["device_ms"], dec, max(q["decisions"] for q in st),
                       1e3 * st[0]["device_ms"] / max(1, max(q["decisions"] for q in st)), o.min(), o.min() / bound))
                for span in [int(x) for x in a.spans.split(",")]:
                    rc, s, o, st = inst.ils(starts, 10 ** 9, seed=1, span=span, time_limit=a.limit)
                    its = sum(q["iterations"] for q in st)
                    longest = max(q["decisions"] for q in st)
                    say("%s %-5s K=%-2d B=%-2d ils span=%-3d  rc=%d %9.1f ms device %8d decisions (longest chain %d) %7.1f us/decision of the "
                        "longest chain  %8d iterations  %9.1f iterations/s  accepted %d  cost %.0f -> %.0f (%.4f x bound)"
                        % (name, lists, K, B, span, rc, st[0]["device_ms"], sum(q["decisions"] for q in st), longest,
                           1e3 * st[0]["device_ms"] / max(1, longest), its, its / max(1e-9, st[0]["seconds"]),
                           sum(q["accepted"] for q in st), min(q["start_cost"] for q in st), o.min(), o.min() / bound))
        inst.close()
    ctx.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
