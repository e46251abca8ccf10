"""Don't-look bits: tsp_dev_ils_dlb with modes 0, 1 and 2, everything else equal -- instance, K = 10 nearest
lists, the greedy tour, seed, iterations, span.  Per row one warm-up call, then --repeats calls of `iterations` iterations and as
many of none (the first descent alone); the iterations' own time is the difference of the two medians.  Reported per mode: device
ms of both (median, min .. max), iterations/s of the iterations alone, decisions, deltas_executed and active_nodes per iteration
(the first descent's taken off), closing scans and the final cost of the best chain.  Mode 0 of the same build is the baseline.
Writes profiles/dlb_time.txt (or the file given with --out).  --rows: instance:chains:iterations, instance a name of
tests/golden/instances or rand<n>."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import load_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dlb_time.txt"))
    ap.add_argument("--rows", default="rand10000:1:300,rand10000:64:300,rand100003:1:100")
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--span", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def spread(v):
        return "%9.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v))

    ctx = E.Context(0)
    say("tsp_dev_ils_dlb, K = %d nearest lists, greedy start, seed %d, span %d, %d repeats behind one warm-up; ms are device ms, "
        "median (min .. max)" % (a.K, a.seed, a.span, a.repeats))
    built = {}
    for row in a.rows.split(","):
        name, B, iters = row.split(":")
        B, iters = int(B), int(iters)
        if name not in built:
            xy, wt = load_instance(name)
            inst = E.Instance(ctx, xy, wt, 1)
            succ, obj, _ = inst.construct(E.GREEDY, np.array([0], dtype=np.int32))
            inst.knn_build(a.K)
            built[name] = (inst, succ[0], obj[0])
        inst, start, obj0 = built[name]
        starts = np.stack([start] * B)
        base = None
        for mode in (E.DLB_OFF, E.DLB_ON, E.DLB_CLOSE):
            def call(I):
                if mode == E.DLB_OFF:
                    return inst.ils(starts, I, seed=a.seed, span=a.span, time_limit=a.limit)
                return inst.ils(starts, I, seed=a.seed, span=a.span, time_limit=a.limit, dlb=mode)
            call(0)
            first, whole = [], []
            for _ in range(a.repeats):
                rc0, _, _, st0 = call(0)
                rc, s, o, st = call(iters)
                first.append(st0[0]["device_ms"])
                whole.append(st[0]["device_ms"])
            own = statistics.median(whole) - statistics.median(first)
            per = lambda k: (sum(q[k] for q in st) - sum(q[k] for q in st0)) / (B * iters)   # noqa: E731
            act = per("active_nodes") if mode != E.DLB_OFF else float(inst.n) * per("decisions")
            base = own if mode == E.DLB_OFF else base
            say("%-10s B=%-2d I=%-4d mode %d rc=%d/%d  first descent %s ms  with iterations %s ms  iterations alone %9.1f ms = %9.1f "
                "iterations/s (all chains; %.2f x mode 0)  per iteration: %6.1f decisions %12.0f deltas %9.1f active nodes  closing "
                "scans %d  accepted %d  cost %.0f -> %.0f"
                % (name, B, iters, mode, rc0, rc, spread(first), spread(whole), own, 1e3 * B * iters / max(own, 1e-9),
                   base / max(own, 1e-9), per("decisions"), per("deltas_executed"), act,
                   sum(q.get("closing_scans", 0) for q in st), sum(q["accepted"] for q in st), obj0, o.min()))
    for inst, _, _ in built.values():
        inst.close()
    ctx.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
