"""Windowed iterated local search with the 3-opt kind: tsp_dev_seg_ils3 over all three kinds against
tsp_dev_seg_ils over 2-opt + Or-opt from the same start, the tsp_dev_nl_3opt_batch local optimum (all three kinds) of the
greedy-edge tour, on rand10000 and rand100003; S = 50, B = 1, seed 1.  Lists: the 10 nearest neighbours and, at the first size, the
5 alpha-nearest under the penalties of tsp_dev_held_karp.

1. The old entry point: tsp_dev_seg_ils at W = 1024, T = 4 at the last size under seg_ils_time.py's rate protocol (a warm-up call,
   then --repeats calls of --iters launches from the same start): median and min .. max of the device ms per launch.  Run from a
   checkout of the parent commit with --old-only it gives the parent's figures; the parent's min .. max is the margin.
2. A trial with the third kind: for W in 128, 1024, 2048 and T in 1, 4, 16 the same protocol for seg_ils3 (kinds 7) and seg_ils
   (kinds 3): ms per launch, microseconds per trial of a workgroup (ms per launch / T), decisions per trial, accepted trials.
3. Cost at equal time: a time limit of 1 s and of 10 s (--budgets), T = 4, W in 512, 1024, 2048, both entry points, both kinds of
   lists; with --bound the gap to tsp_dev_held_karp's bound at the first size.  One run each.

Writes profiles/seg_ils3_time.txt (or --out).  --old-only: parts 1 and 3 of tsp_dev_seg_ils alone, which is all a checkout of the
parent commit can run: this file, copied into that checkout's tools/, uses that checkout's package and libraries (the binding of
this commit does not load a library without tsp_dev_seg_ils3); its lines go behind the others with --append."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import rand_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402

K_NN, K_ALPHA, SPAN = 10, 5, 50
RATE_WINDOWS, RATE_TRIALS = (128, 1024, 2048), (1, 4, 16)
COST_WINDOWS, COST_TRIALS = (512, 1024, 2048), 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_ils3_time.txt"))
    ap.add_argument("--sizes", default="10000,100003")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--budgets", default="1,10")
    ap.add_argument("--bound", action="store_true")
    ap.add_argument("--old-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rate(call, W, T):
        """the rate protocol -> (median, min, max ms per launch, stats of the last call)"""
        call(2, W, T)                                                         # warm-up: module load, scratch
        ms, st = [], None
        for _ in range(a.repeats):
            rc, s, o, st = call(a.iters, W, T)
            ms.append(st["device_ms"] / a.iters)
        return statistics.median(ms), min(ms), max(ms), st

    if a.label:
        say("# " + a.label)
    budgets = [float(x) for x in a.budgets.split(",")]
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = E.Context(0)
    for idx, n in enumerate(sizes):
        xy = rand_instance(n)
        inst = E.Instance(ctx, xy, E.EUC_2D, 1)
        inst.knn_build(K_NN)
        succ, obj = inst.greedy_edge()
        bound = pi = None
        gap = lambda c: "" if bound is None or not a.bound else "  %.3f %% above the bound" % (100.0 * (c / bound - 1.0))   # noqa: E731
        for lists in ("knn%d" % K_NN,) + (("alpha%d" % K_ALPHA,) if idx == 0 else ()):
            if lists.startswith("alpha"):
                inst.alpha_build(K_ALPHA, pi=pi)
            rc, start, c0, st = inst.nl_3opt_batch(succ, obj, kinds=7)
            if idx == 0 and pi is None:                                       # the bound, and the penalties of the alpha lists
                bound, pi, hst = inst.held_karp(c0, time_limit=30.0)          # valid also when the limit ends the ascent
                say("n=%-7d held_karp bound %.1f (%d iterations, %.0f ms device)" % (n, bound, hst["iterations"], hst["device_ms"]))
            say("n=%-7d %-7s start: greedy_edge %.0f -> nl_3opt_batch (kinds 7) %.0f, %d moves, %.1f ms device%s"
                % (n, lists, obj, c0, st["moves"], st["device_ms"], gap(c0)))
            old = lambda I, W, T, **kw: inst.seg_ils(start, I, W, SPAN, T, seed=1, kinds=3, **kw)           # noqa: E731
            new = lambda I, W, T, **kw: inst.seg_ils3(start, I, W, SPAN, T, seed=1, kinds=7, **kw)          # noqa: E731
            if lists.startswith("knn"):
                if idx == len(sizes) - 1:
                    med, lo, hi, st = rate(old, 1024, 4)
                    say("n=%-7d %-7s seg_ils  kinds=3 W=1024 T=4  M=%-4d %8.4f ms/launch (min %.4f max %.4f, %d runs of %d launches)"
                        % (n, lists, st["windows"], med, lo, hi, a.repeats, a.iters))
                for W in RATE_WINDOWS if not a.old_only else ():
                    for T in RATE_TRIALS:
                        for name, call in (("seg_ils3 kinds=7", new), ("seg_ils  kinds=3", old)):
                            med, lo, hi, st = rate(call, W, T)
                            say("n=%-7d %-7s %s W=%-4d T=%-2d M=%-4d %8.3f ms/launch (min %.3f max %.3f)  %7.1f us/trial  "
                                "%5.2f decisions/trial  %5.2f moves/trial (%d 3-opt)  accepted %d of %d"
                                % (n, lists, name, W, T, st["windows"], med, lo, hi, 1e3 * med / T,
                                   st["decisions"] / max(1, st["trials"]), st["moves"] / max(1, st["trials"]),
                                   st.get("moves_3opt", 0), st["accepted"], st["trials"]))
            for budget in budgets:
                for W in COST_WINDOWS:
                    rc, s, oo, so = old(10 ** 9, W, COST_TRIALS, time_limit=budget)
                    say("n=%-7d %-7s %4.0f s W=%-4d T=%d seg_ils  kinds=3: %8d iterations %10d trials (%d accepted) %5.2f decisions/trial  "
                        "%10.1f ms device  cost %.0f%s"
                        % (n, lists, budget, W, COST_TRIALS, so["iterations"], so["trials"], so["accepted"],
                           so["decisions"] / max(1, so["trials"]), so["device_ms"], oo, gap(oo)))
                    if a.old_only:
                        continue
                    rc, s, on, sn = new(10 ** 9, W, COST_TRIALS, time_limit=budget)
                    say("n=%-7d %-7s %4.0f s W=%-4d T=%d seg_ils3 kinds=7: %8d iterations %10d trials (%d accepted) %5.2f decisions/trial  "
                        "%10.1f ms device  cost %.0f  cost / cost(seg_ils) = %.5f%s  moves %d = %d + %d + %d, types %s"
                        % (n, lists, budget, W, COST_TRIALS, sn["iterations"], sn["trials"], sn["accepted"],
                           sn["decisions"] / max(1, sn["trials"]), sn["device_ms"], on, on / oo, gap(on), sn["moves"],
                           sn["moves_2opt"], sn["moves_oropt"], sn["moves_3opt"], sn["moves_by_type"]))
        inst.close()
    ctx.close()
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
