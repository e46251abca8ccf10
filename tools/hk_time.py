"""Held-Karp lower bound: time per 1-tree, Boruvka rounds, the scan's distance rate beside k_knn_scan's and
k_or_scan's, the 300-iteration ascent and the gap it leaves to the 2-opt + Or-opt tour.  Writes profiles/hk_time.txt (or the
file given with --out).  --cpu-sizes: sizes at which the reference ascent's time per tree is taken on this machine's CPU.
--ascent-only N: just the default ascent at rand<N> (the run a kernel trace is taken of)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import held_karp_ref as HK  # noqa: E402
from helpers import load_instance, rand_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402

OR_SCAN_RATE = 2.5e12   # k_or_scan's delta expressions per second


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hk_time.txt"))
    ap.add_argument("--sizes", default="1002,10000,20011,100003")
    ap.add_argument("--cpu-sizes", default="1002,10000")
    ap.add_argument("--iters", type=int, default=E.HK_DEFAULT_ITERS)
    ap.add_argument("--ascent-only", type=int, default=0)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = E.Context(0)
    if a.ascent_only:
        n = a.ascent_only
        inst = E.Instance(ctx, rand_instance(n), E.EUC_2D, 1)
        succ, obj, _ = inst.construct(E.GREEDY, np.array([0], dtype=np.int32))
        _, _, ub, _, _ = inst.two_opt_or_opt(succ[0], obj[0])
        bound, _, st = inst.held_karp(ub, max_iters=a.iters)
        print("ascent n=%d: bound %.1f, %d iterations, %.1f ms device" % (n, bound, st["iterations"], st["device_ms"]))
        inst.close()
        ctx.close()
        return
    cpu = {int(x) for x in a.cpu_sizes.split(",") if x}
    for n in [int(x) for x in a.sizes.split(",")]:
        xy, wt = load_instance("pr1002") if n == 1002 else (rand_instance(n), E.EUC_2D)
        name = "pr1002" if n == 1002 else "rand%d" % n
        inst = E.Instance(ctx, xy, wt, 1)
        inst.one_tree()   # warm: code objects, scratch
        best = None
        for _ in range(5):
            st = inst.one_tree(want_stats=True)[3]
            if best is None or st["device_ms"] < best["device_ms"]:
                best = st
        knn_ms = min(inst.knn_build(16) for _ in range(3))
        rate = best["dists_executed"] / (best["device_ms"] * 1e-3)
        knn_rate = n * (n - 1.0) / (knn_ms * 1e-3)
        say("one_tree   %-10s %10.1f us  %2d rounds (all %d queued)  %.3e weights/s over the whole tree  (%.2f x k_knn_scan's %.3e distances/s, "
            "%.2f x k_or_scan's %.1e deltas/s)"
            % (name, 1e3 * best["device_ms"], best["rounds"], max(1, int(np.ceil(np.log2(n - 1)))), rate, rate / knn_rate, knn_rate,
               rate / OR_SCAN_RATE, OR_SCAN_RATE))
        succ, obj, _ = inst.construct(E.GREEDY, np.array([0], dtype=np.int32))
        _, _, ub, _, _ = inst.two_opt_or_opt(succ[0], obj[0])
        w0 = inst.one_tree()[2]
        inst.held_karp(ub, max_iters=3)   # warm
        bound, _, st = inst.held_karp(ub, max_iters=a.iters)
        say("held_karp  %-10s %10.1f ms device  %.2f s wall  %d iterations  %d trees  %.1f rounds/tree  %.1f us/tree  %.3e weights/s  "
            "ub %.0f  W(0) %.0f  bound %.1f  gap (ub - bound)/bound = %.4f  lambda %.3g%s"
            % (name, st["device_ms"], st["seconds"], st["iterations"], st["trees"], st["rounds"] / max(1, st["trees"]),
               1e3 * st["device_ms"] / max(1, st["trees"]), st["dists_executed"] / (st["device_ms"] * 1e-3), ub, w0, bound,
               (ub - bound) / bound, st["lambda_final"], "  (tour found)" if st["tour_found"] else ""))
        inst.close()
        if n in cpu:
            R = HK.Matrix(__import__("oracle.oracle", fromlist=["x"]).dist_matrix(xy, wt, 1)) if n <= 2000 else HK.Euc2DRows(xy)
            t0 = time.perf_counter()
            HK.one_tree(R)
            say("reference  %-10s %10.1f ms per tree (numpy Prim of tests/held_karp_ref.py, one thread of: %s)"
                % (name, 1e3 * (time.perf_counter() - t0), cpu_model()))
    ctx.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
