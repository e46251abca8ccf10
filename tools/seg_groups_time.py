"""Windowed iterated local search with groups: tsp_dev_seg_ils_groups against tsp_dev_seg_ils3 from the same
start, the tsp_dev_nl_3opt_batch local optimum (all three kinds) of the greedy-edge tour, on rand10000 and rand100003; the 10
nearest neighbours, S = 50, T = 4, B = 1, seed 1 (the protocol of tools/seg_ils3_time.py).

1. The old entry points: tsp_dev_seg_ils3 (kinds 7) and tsp_dev_seg_ils (kinds 3) at W = 1024 at the last size under the rate
   protocol (a warm-up call, then --repeats calls of --iters launches from the same start): median and min .. max of the device ms
   per launch.  Run from a checkout of the parent commit with --old-only it gives the parent's figures; the parent's min .. max is
   the margin.
2. Rate: for W in 1024, 2048 and G = 1, 2, 4, 8, .. up to the default G (and the default itself) the same protocol for
   tsp_dev_seg_ils_groups: ms per iteration (both launches), trials per second, offers and commits of the last call.
3. Cost at equal time: a time limit of 1 s and of 10 s (--budgets), W in 1024, 2048: tsp_dev_seg_ils3 and tsp_dev_seg_ils_groups
   with the default G, with the gap to the best certified bound of profiles/hk_sparse_time.txt.  One run each.

Writes profiles/seg_groups_time.txt (or --out).  --old-only: parts 1 and 3 of the old entry points alone, which is all a checkout
of the parent commit can run: this file, copied into that checkout's tools/, uses that checkout's package and libraries; its lines
go behind the others with --append."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import rand_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402

K_NN, SPAN, TRIALS = 10, 50, 4
WINDOWS = (1024, 2048)
BOUNDS = {10000: 71209485.0, 100003: 221498593.1}   # profiles/hk_sparse_time.txt: the best certified bound of each size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_groups_time.txt"))
    ap.add_argument("--sizes", default="10000,100003")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--budgets", default="1,10")
    ap.add_argument("--old-only", action="store_true")
    ap.add_argument("--no-rate", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rate(call, W):
        """the rate protocol -> (median, min, max ms per iteration, stats of the last call)"""
        call(2, W)                                                            # warm-up: module load, scratch
        ms, st = [], None
        for _ in range(a.repeats):
            rc, s, o, st = call(a.iters, W)
            ms.append(st["device_ms"] / a.iters)
        return statistics.median(ms), min(ms), max(ms), st

    if a.label:
        say("# " + a.label)
    budgets = [float(x) for x in a.budgets.split(",") if x]
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = E.Context(0)
    for idx, n in enumerate(sizes):
        xy = rand_instance(n)
        inst = E.Instance(ctx, xy, E.EUC_2D, 1)
        inst.knn_build(K_NN)
        succ, obj = inst.greedy_edge()
        gap = lambda c: "" if n not in BOUNDS else "  %.3f %% above the bound" % (100.0 * (c / BOUNDS[n] - 1.0))   # noqa: E731
        rc, start, c0, st = inst.nl_3opt_batch(succ, obj, kinds=7)
        say("n=%-7d start: greedy_edge %.0f -> nl_3opt_batch (kinds 7) %.0f, %d moves, %.1f ms device%s"
            % (n, obj, c0, st["moves"], st["device_ms"], gap(c0)))
        old2 = lambda I, W, **kw: inst.seg_ils(start, I, W, SPAN, TRIALS, seed=1, kinds=3, **kw)           # noqa: E731
        old3 = lambda I, W, **kw: inst.seg_ils3(start, I, W, SPAN, TRIALS, seed=1, kinds=7, **kw)          # noqa: E731
        if idx == len(sizes) - 1 and not a.no_rate:
            for name, call in (("seg_ils3 kinds=7", old3), ("seg_ils  kinds=3", old2)):
                med, lo, hi, st = rate(call, 1024)
                say("n=%-7d %s W=1024 T=%d M=%-4d %8.4f ms/launch (min %.4f max %.4f, %d runs of %d launches)"
                    % (n, name, TRIALS, st["windows"], med, lo, hi, a.repeats, a.iters))
        if not a.old_only and not a.no_rate:
            for W in WINDOWS:
                top = max(1, min(E.SEG_ILS_MAX_GROUPS, 1024 // (n // W)))
                gs = sorted({g for g in (1, 2, 4, 8, 16, 32, 64) if g <= top} | {top})
                for G in gs:
                    call = lambda I, W, G=G, **kw: inst.seg_ils_groups(start, I, G, W, SPAN, TRIALS, seed=1, kinds=7, **kw)   # noqa: E731
                    med, lo, hi, st = rate(call, W)
                    say("n=%-7d seg_ils_groups kinds=7 W=%-4d T=%d M=%-4d G=%-2d%s workgroups %-5d %8.3f ms/iteration (min %.3f max %.3f)  "
                        "%9.0f trials/s  accepted %d, offers %d, commits %d of %d trials"
                        % (n, W, TRIALS, st["windows"], G, "*" if G == top else " ", st["windows"] * G, med, lo, hi,
                           1e3 * st["windows"] * G * TRIALS / med, st["accepted"], st["offers"], st["commits"], st["trials"]))
        for budget in budgets:
            for W in WINDOWS:
                rc, s, oo, so = old3(10 ** 9, W, time_limit=budget)
                say("n=%-7d %4.0f s W=%-4d T=%d seg_ils3       kinds=7: %8d iterations %10d trials (%d accepted)  %10.1f ms device  "
                    "cost %.0f%s" % (n, budget, W, TRIALS, so["iterations"], so["trials"], so["accepted"], so["device_ms"], oo, gap(oo)))
                if a.old_only:
                    continue
                rc, s, on, sn = inst.seg_ils_groups(start, 10 ** 9, 0, W, SPAN, TRIALS, seed=1, kinds=7, time_limit=budget)
                say("n=%-7d %4.0f s W=%-4d T=%d seg_ils_groups kinds=7: %8d iterations %10d trials (%d accepted)  %10.1f ms device  "
                    "cost %.0f%s  G=%d  offers %d, commits %d  cost / cost(seg_ils3) = %.5f"
                    % (n, budget, W, TRIALS, sn["iterations"], sn["trials"], sn["accepted"], sn["device_ms"], on, gap(on), sn["groups"],
                       sn["offers"], sn["commits"], on / oo))
        inst.close()
    ctx.close()
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
