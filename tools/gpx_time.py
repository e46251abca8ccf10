"""Partition crossover: what one tsp_dev_gpx call costs, and whether C windowed chains merged by a tournament beat
one chain at equal device time.  rand10000 and rand100003 from the tsp_dev_nl_3opt_batch local optimum (all three kinds) of the
greedy-edge tour, the 10 nearest neighbours, tsp_dev_seg_ils_lk at its defaults (kinds 15, default depth, window and groups) with
S = 50, T = 4, seed 1: the protocol of tools/seg_lk_time.py.

1. One call.  Parents: two chains (streams 0 and 1 of seed 1) of --warm-iters iterations from the start.  Device ms of one gpx call
   with P = 1 and with P = 4 (the same pair four times), the minimum of three after a warm-up call, with the component rounds and
   the counters.  --calls-only stops here: run that under `rocprofv3 --kernel-trace --stats` for the share of the kernels in the
   call's device time (the rest is launch gaps and the host's polls).
2. The claim.  For every budget T of --budgets and C of --chains: C chains in one device call (B = C) under a time limit of T
   seconds, then the tournament; against one chain under the same limit.  Same seed, one run each.  Per merge: components /
   exchangeable / taken.  Gaps are to the best certified bound of profiles/hk_sparse_time.txt.

Writes profiles/gpx_time.txt (or --out)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import rand_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402

K_NN, SPAN, TRIALS = 10, 50, 4
BOUNDS = {10000: 71209485.0, 100003: 221498593.1}   # profiles/hk_sparse_time.txt: the best certified bound of each size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpx_time.txt"))
    ap.add_argument("--sizes", default="10000,100003")
    ap.add_argument("--budgets", default="1,10")
    ap.add_argument("--chains", default="2,4,8")
    ap.add_argument("--warm-iters", type=int, default=50)
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = E.Context(0)
    for n in [int(x) for x in a.sizes.split(",") if x]:
        xy = rand_instance(n)
        inst = E.Instance(ctx, xy, E.EUC_2D, 1)
        inst.knn_build(K_NN)
        succ, obj = inst.greedy_edge()
        gap = lambda c: "" if n not in BOUNDS else "  %.3f %% above the bound" % (100.0 * (c / BOUNDS[n] - 1.0))   # noqa: E731
        rc, start, c0, st = inst.nl_3opt_batch(succ, obj, kinds=7)
        say("n=%-7d start: greedy_edge %.0f -> nl_3opt_batch (kinds 7) %.0f%s" % (n, obj, c0, gap(c0)))
        chains = lambda C, I, **kw: inst.seg_ils_lk(np.stack([start] * C), I, 15, 0, 0, 0, SPAN, TRIALS, seed=1, **kw)   # noqa: E731

        rc, par, po, _ = chains(2, a.warm_iters)
        inst.gpx(par[0], par[1])                                     # warm-up: module load, scratch
        for P in (1, 4):
            A, B = np.stack([par[0]] * P), np.stack([par[1]] * P)
            runs = [inst.gpx(A, B, want_stats=True)[2][0] for _ in range(3)]
            s = min(runs, key=lambda r: r["device_ms"])
            say("n=%-7d gpx P=%d: %.3f ms device (min of 3: %s), %.3f ms wall, %d component rounds; parents %.0f %.0f -> child %.0f; "
                "%d common edges, %d components, %d exchangeable, %d taken, %d stretches"
                % (n, P, s["device_ms"], " ".join("%.3f" % r["device_ms"] for r in runs), 1e3 * s["seconds"], s["rounds"], s["cost_a"],
                   s["cost_b"], s["cost_child"], s["common_edges"], s["components"], s["exchangeable"], s["taken"], s["stretches"]))
        if a.calls_only:
            inst.close()
            continue

        for budget in [float(x) for x in a.budgets.split(",") if x]:
            rc, s1, o1, t1 = chains(1, 10 ** 9, time_limit=budget)
            o1 = float(o1[0])
            say("n=%-7d %4.0f s C=1: %7d iterations, %.0f ms device, cost %.0f%s"
                % (n, budget, t1[0]["iterations"], t1[0]["device_ms"], o1, gap(o1)))
            for C in [int(x) for x in a.chains.split(",") if x]:
                rc, sC, oC, tC = chains(C, 10 ** 9, time_limit=budget)
                child, cost, rounds = inst.gpx_tournament(sC)
                merge_ms = sum(r[0]["device_ms"] for r in rounds)
                per = " | ".join(" ".join("%d/%d/%d" % (m["components"], m["exchangeable"], m["taken"]) for m in r) for r in rounds)
                say("n=%-7d %4.0f s C=%d: %7d iterations, %.0f ms device + %.2f ms merging; chains %.0f .. %.0f, child %.0f%s; "
                    "child / best chain = %.6f, child / one chain = %.6f; components/exchangeable/taken per merge: %s"
                    % (n, budget, C, tC[0]["iterations"], tC[0]["device_ms"], merge_ms, oC.min(), oC.max(), cost, gap(cost),
                       cost / oC.min(), cost / o1, per))
        inst.close()
    ctx.close()
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
