"""Held-Karp ascent over the candidate graph: the certified bound and the device time of
tsp_dev_held_karp_sparse beside the dense 300-iteration ascent, from the nl_3opt_batch tour's cost as ub.  Writes
profiles/hk_sparse_time.txt (or the file given with --out).  Every figure is the minimum and the median of --reps timed calls
behind one warm-up call; the bounds are the same bits in every repetition."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import load_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402

# the tours whose gaps README.md and DESIGN.md 4.21 quote against the 300-iteration bound (profiles/seg_ils3_time.txt)
QUOTED = {"rand10000": [("nl_3opt_batch start, KNN-10", 73682070.0), ("seg_ils3 10 s W=2048, KNN-10", 72480004.0),
                        ("seg_ils3 10 s W=2048, alpha-5", 72375440.0)]}


def timed(call, reps):
    call()   # warm: code objects, scratch, lists
    out = [call() for _ in range(reps)]
    ms = [o[2]["device_ms"] for o in out]
    assert len({o[0] for o in out}) == 1, "two runs returned different bounds"
    return out[0], min(ms), statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hk_sparse_time.txt"))
    ap.add_argument("--instances", default="pr1002,rand10000,rand100003")
    ap.add_argument("--iters", default="300,1000,3000,10000")
    ap.add_argument("--lists", default="10,16")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(a.out, "w") as f:   # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    ctx = E.Context(0)
    for name in a.instances.split(","):
        xy, wt = load_instance(name)
        n = len(xy)
        inst = E.Instance(ctx, xy, wt, 1)
        inst.knn_build(10)
        succ, obj = inst.greedy_edge()
        _, _, ub, _ = inst.nl_3opt_batch(succ, obj, kinds=7)
        say("%-10s ub = %.0f (greedy_edge -> nl_3opt_batch, kinds 7, KNN-10)" % (name, ub))
        reps = a.reps if n <= 20000 else max(1, a.reps - 1)
        (dbound, _, dst), dmin, dmed = timed(lambda: inst.held_karp(ub), reps)
        say("%-10s dense   300 iterations: bound %.1f  %.1f ms device (median %.1f, %d runs)  %.1f us/tree  %.1f rounds/tree  lambda %.3g"
            % (name, dbound, dmin, dmed, reps, 1e3 * dmin / dst["trees"], dst["rounds"] / dst["trees"], dst["lambda_final"]))
        best_bound = dbound
        in_time = None   # the best certified bound among the runs that took no longer than the dense ascent
        per_tree = {}
        for K in [int(k) for k in a.lists.split(",")]:
            K = min(K, n - 1)
            for iters in [int(i) for i in a.iters.split(",")]:
                def call():
                    inst.knn_build(K)
                    return inst.held_karp_sparse(ub, iters, 1)
                (bound, _, st), smin, smed = timed(call, reps)
                sp_ms = st["sparse_device_ms"]
                us = 1e3 * sp_ms / max(1, st["sparse_trees"])
                per_tree[K] = us
                say("%-10s sparse  KNN-%-2d %5d + 1: certified %.1f  sparse_best %.1f (%.4f %% above it)  %.1f ms device (median %.1f)  "
                    "%.1f us/sparse tree  %.2f + %.2f rounds/tree  %d components  lambda %.3g  gap (ub - bound)/bound = %.4f"
                    % (name, K, iters, bound, st["sparse_best"], 100.0 * (st["sparse_best"] - bound) / bound, smin, smed, us,
                       st["sparse_rounds"] / max(1, st["sparse_trees"]), st["completion_rounds"] / max(1, st["sparse_trees"]),
                       st["components"], st["lambda_sparse_final"], (ub - bound) / bound))
                best_bound = max(best_bound, bound)
                if smin <= dmin and (in_time is None or bound > in_time[0]):
                    in_time = (bound, K, iters, smin)
        # as many sparse iterations over KNN-10 as the dense ascent's device time holds beside the one dense tree
        K = min(10, n - 1)
        dense_tree_ms = dmin / dst["trees"]
        fit = int(max(1.0, (dmin - 2.0 * dense_tree_ms) / (1e-3 * per_tree[K])))
        inst.knn_build(K)
        bound, _, st = inst.held_karp_sparse(ub, fit, 1)
        say("%-10s equal time: KNN-%d %d + 1 in %.1f ms device (dense 300: %.1f ms): certified %.1f against the dense ascent's %.1f"
            % (name, K, fit, st["device_ms"], dmin, bound, dbound))
        if st["device_ms"] <= dmin:
            best_bound = max(best_bound, bound)
            if in_time is None or bound > in_time[0]:
                in_time = (bound, K, fit, st["device_ms"])
        if in_time:
            say("%-10s best certified bound within the dense ascent's %.1f ms: %.1f (KNN-%d, %d + 1, %.1f ms); dense 300: %.1f"
                % (name, dmin, in_time[0], in_time[1], in_time[2], in_time[3], dbound))
        else:
            say("%-10s no sparse run fitted into the dense ascent's %.1f ms" % (name, dmin))
        say("%-10s best certified bound of this file: %.1f; ub stands %.3f %% above it (%.3f %% above the dense 300-iteration bound)"
            % (name, best_bound, 100.0 * (ub - best_bound) / best_bound, 100.0 * (ub - dbound) / dbound))
        for what, cost in QUOTED.get(name, []):
            say("%-10s quoted tour %-32s cost %.0f: %.3f %% above the best certified bound (%.3f %% above the dense 300-iteration bound)"
                % (name, what, cost, 100.0 * (cost - best_bound) / best_bound, 100.0 * (cost - dbound) / dbound))
        inst.close()
    ctx.close()


if __name__ == "__main__":
    main()
