"""Windowed iterated local search: tsp_dev_seg_ils against tsp_dev_ils_dlb (TSP_DLB_ON, 2-opt + Or-opt, span
50, one chain) from the same start, the tsp_dev_nl_3opt_batch local optimum (2-opt + Or-opt) of the greedy-edge tour over K = 10
nearest-neighbour lists, on rand10000 and rand100003.

1. Rate: for W in 128 .. 2048 and T in 1, 4, 16 (S = 50, B = 1) a warm-up call, then --repeats calls of --iters iterations from
   the same start (the same work each time): median and min .. max of the device ms (HIP events, stats.device_ms) per launch and
   the trials per second of the median.
2. Baseline: tsp_dev_ils_dlb under a time limit, as iterations per second of device time.
3. Cost at equal time: both under a time limit of 1 s and of 10 s (--budgets); with --bound the gap to tsp_dev_held_karp's
   bound at the first size.

Writes profiles/seg_ils_time.txt (or --out).  --baseline-only: parts 2 and 3 of tsp_dev_ils_dlb alone, which is all a checkout
of an older commit can run: this file, copied into that checkout's tools/, uses that checkout's package and libraries (the
binding of this commit does not load a library without tsp_dev_seg_ils); its lines go behind the others with --append."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import rand_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402

K, SPAN, KINDS = 10, 50, E.NL_2OPT | E.NL_OROPT
WINDOWS = (128, 256, 512, 1024, 2048)
TRIALS = (1, 4, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_ils_time.txt"))
    ap.add_argument("--sizes", default="10000,100003")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--budgets", default="1,10")
    ap.add_argument("--bound", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.label:
        say("# " + a.label)
    budgets = [float(x) for x in a.budgets.split(",")]
    ctx = E.Context(0)
    for idx, n in enumerate(int(x) for x in a.sizes.split(",")):
        xy = rand_instance(n)
        inst = E.Instance(ctx, xy, E.EUC_2D, 1)
        inst.knn_build(K)
        succ, obj = inst.greedy_edge()
        rc, start, c0, st = inst.nl_3opt_batch(succ, obj, kinds=KINDS)
        say("n=%-7d start: greedy_edge %.0f -> nl_3opt_batch (2-opt + Or-opt) %.0f, %d moves, %.1f ms device"
            % (n, obj, c0, st["moves"], st["device_ms"]))
        bound = None
        if a.bound and idx == 0:
            bound, _, hst = inst.held_karp(c0, time_limit=30.0)   # valid also when the limit ends the ascent
            say("n=%-7d held_karp bound %.1f (%d iterations, %.0f ms device): the start is %.3f %% above it"
                % (n, bound, hst["iterations"], hst["device_ms"], 100.0 * (c0 / bound - 1.0)))
        gap = lambda c: "" if bound is None else "  %.3f %% above the bound" % (100.0 * (c / bound - 1.0))   # noqa: E731
        if not a.baseline_only:
            for W in WINDOWS:
                for T in TRIALS:
                    inst.seg_ils(start, 2, W, SPAN, T, seed=1)                # warm-up: module load, scratch
                    ms, last = [], None
                    for _ in range(a.repeats):
                        rc, s, o, st = inst.seg_ils(start, a.iters, W, SPAN, T, seed=1)
                        ms.append(st["device_ms"] / a.iters)
                        last = (o, st)
                    med = statistics.median(ms)
                    o, st = last
                    say("n=%-7d seg_ils W=%-4d T=%-2d M=%-4d %8.3f ms/launch (min %.3f max %.3f, %d runs of %d launches)  "
                        "%10.0f trials/s  %5.1f decisions/trial  accepted %d of %d  cost %.0f"
                        % (n, W, T, st["windows"], med, min(ms), max(ms), a.repeats, a.iters,
                           1e3 * st["windows"] * T / med, st["decisions"] / max(1, st["trials"]), st["accepted"], st["trials"], o))
        inst.ils(start, 2, seed=1, span=SPAN, kinds=KINDS, dlb=E.DLB_ON)      # warm-up
        for budget in budgets:
            rc, s, o, st = inst.ils(start, 10 ** 9, seed=1, span=SPAN, kinds=KINDS, time_limit=budget, dlb=E.DLB_ON)
            say("n=%-7d ils_dlb  %4.0f s: %8d iterations (%d accepted) %10.1f ms device  %9.1f iterations/s  cost %.0f (start %.0f)%s"
                % (n, budget, st["iterations"], st["accepted"], st["device_ms"], 1e3 * st["iterations"] / st["device_ms"], o, c0,
                   gap(o)))
            if a.baseline_only:
                continue
            for W in WINDOWS:
                rc, s, ow, sw = inst.seg_ils(start, 10 ** 9, W, SPAN, 4, seed=1, time_limit=budget)
                say("n=%-7d seg_ils  %4.0f s: W=%-4d T=4 %8d iterations %10d trials (%d accepted) %10.1f ms device  %10.0f trials/s  "
                    "cost %.0f  cost / cost(ils_dlb) = %.5f%s"
                    % (n, budget, W, sw["iterations"], sw["trials"], sw["accepted"], sw["device_ms"],
                       1e3 * sw["trials"] / sw["device_ms"], ow, ow / o, gap(ow)))
        inst.close()
    ctx.close()
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
