"""Windowed iterated local search with Lin-Kernighan chains: tsp_dev_seg_ils_lk with kinds 15 against
tsp_dev_seg_ils_groups with kinds 7 from the same start, the tsp_dev_nl_3opt_batch local optimum (all three kinds) of the
greedy-edge tour, on rand10000 and rand100003; the 10 nearest neighbours, S = 50, T = 4, B = 1, seed 1 (the protocol of
tools/seg_groups_time.py).

1. The old entry points: tsp_dev_seg_ils (kinds 3), tsp_dev_seg_ils3 (kinds 7) and tsp_dev_seg_ils_groups (kinds 7, default G) at
   W = 1024 at the last size under the rate protocol (a warm-up call, then --repeats calls of --iters launches from the same start):
   median and min .. max of the device ms per launch (per iteration for the groups, which are two launches).  Run from a checkout
   of the parent commit with --old-only it gives the parent's figures; the parent's min .. max is the margin.
2. Cost of the kind: at the last size, W in 1024, 2048, default G and G = 1, the same protocol for kinds 7 (tsp_dev_seg_ils_groups)
   and for kinds 15 at every depth of --depths: ms per iteration, microseconds and decisions per trial, and the chain counters of
   the last call.
3. Cost at equal time: a time limit of 1 s and of 10 s (--budgets), every size, W in 1024, 2048, default G: kinds 7 and kinds 15 at
   every depth, with the gap to the best certified bound of profiles/hk_sparse_time.txt; G = 1 the same at the budgets of
   --budgets1 and the windows of --windows1.  One run each.

Writes profiles/seg_lk_time.txt (or --out).  --old-only: part 1 alone, which is all a checkout of the parent commit can run: this
file, copied into that checkout's tools/, uses that checkout's package and libraries; its lines go behind the others with
--append."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_lk_time.txt"))
    ap.add_argument("--sizes", default="10000,100003")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--depths", default="3,5,8,12,16")
    ap.add_argument("--budgets", default="1,10")
    ap.add_argument("--budgets1", default="1,10")
    ap.add_argument("--windows1", default="1024,2048")
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
    floats = lambda s: [float(x) for x in s.split(",") if x]   # noqa: E731
    ints = lambda s: [int(x) for x in s.split(",") if x]       # noqa: E731
    depths, sizes = ints(a.depths), ints(a.sizes)
    ctx = E.Context(0)
    for idx, n in enumerate(sizes):
        last = idx == len(sizes) - 1
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
        grp = lambda I, W, G=0, **kw: inst.seg_ils_groups(start, I, G, W, SPAN, TRIALS, seed=1, kinds=7, **kw)   # noqa: E731
        if last and not a.no_rate:
            for name, call in (("seg_ils        kinds=3", old2), ("seg_ils3       kinds=7", old3), ("seg_ils_groups kinds=7", grp)):
                med, lo, hi, st = rate(call, 1024)
                say("n=%-7d %s W=1024 T=%d M=%-4d %8.4f ms/iteration (min %.4f max %.4f, %d runs of %d iterations)"
                    % (n, name, TRIALS, st["windows"], med, lo, hi, a.repeats, a.iters))
        if a.old_only:
            inst.close()
            continue
        lk = lambda I, W, D, G=0, **kw: inst.seg_ils_lk(start, I, 15, D, G, W, SPAN, TRIALS, seed=1, **kw)   # noqa: E731
        if last and not a.no_rate:
            for W in WINDOWS:
                for G in (0, 1):
                    med7, lo, hi, st = rate(lambda I, W: grp(I, W, G), W)
                    per = st["trials"] / a.iters
                    say("n=%-7d rate W=%-4d G=%-2d kinds=7       %8.3f ms/iteration (min %.3f max %.3f)  %7.3f us/trial  %6.2f decisions/trial"
                        % (n, W, st["groups"], med7, lo, hi, 1e3 * med7 / per, st["decisions"] / st["trials"]))
                    for D in depths:
                        med, lo, hi, st = rate(lambda I, W: lk(I, W, D, G), W)
                        say("n=%-7d rate W=%-4d G=%-2d kinds=15 D=%-2d %8.3f ms/iteration (min %.3f max %.3f)  %7.3f us/trial  %6.2f decisions/trial"
                            "  x%.2f of kinds 7  lk_chains %d lk_steps %d moves_lk %d lk_flips %d of %d moves"
                            % (n, W, st["groups"], D, med, lo, hi, 1e3 * med / per, st["decisions"] / st["trials"], med / med7,
                               st["lk_chains"], st["lk_steps"], st["moves_lk"], st["lk_flips"], st["moves"]))
        plans = [(0, floats(a.budgets), WINDOWS), (1, floats(a.budgets1), ints(a.windows1))]
        for G, budgets, windows in plans:
            for budget in budgets:
                for W in windows:
                    rc, s, o7, s7 = grp(10 ** 9, W, G, time_limit=budget)
                    say("n=%-7d %4.0f s W=%-4d G=%-2d kinds=7      : %7d iterations %10d trials (%d accepted)  cost %.0f%s"
                        % (n, budget, W, s7["groups"], s7["iterations"], s7["trials"], s7["accepted"], o7, gap(o7)))
                    for D in depths:
                        rc, s, o, sl = lk(10 ** 9, W, D, G, time_limit=budget)
                        say("n=%-7d %4.0f s W=%-4d G=%-2d kinds=15 D=%-2d: %7d iterations %10d trials (%d accepted)  cost %.0f%s  "
                            "moves_lk %d lk_flips %d of %d moves  cost / cost(kinds 7) = %.5f"
                            % (n, budget, W, sl["groups"], D, sl["iterations"], sl["trials"], sl["accepted"], o, gap(o),
                               sl["moves_lk"], sl["lk_flips"], sl["moves"], o / o7))
        inst.close()
    ctx.close()
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
