"""Batched list descent: tsp_dev_nl_3opt_batch over a few (max_arc, rounds) settings against the plain rule
(tsp_dev_nl_3opt) from the same greedy-edge tour, all three kinds over K = 10 nearest-neighbour lists, on rand10000 .. rand200000.
Per run: decisions, moves, device ms and the final cost; per batched run the ratio of the plain rule's device time to its own
(above 1: the batched rule is faster).  Writes profiles/nl_batch_time.txt (or the file given with --out).

--plain-only: the plain rule alone, for a build of another commit (TSP_LIB_DIR names its libraries): its lines go behind the
others with --append, and the ratios against them are taken by hand.  --limit S: time limit of a descent."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import rand_instance  # noqa: E402
from tsp_optimization_amd import engine as E  # noqa: E402

K = 10
# (max_arc, rounds); max_arc 0 = n / 2
SETTINGS = ((0, 1), (0, 2), (0, 4), (1000, 2), (1000, 4), (100, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nl_batch_time.txt"))
    ap.add_argument("--sizes", default="10000,20011,50000,100003,200000")
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def row(n, rule, rc, st, o, plain_ms):
        ratio = "" if plain_ms is None else "  plain / this = %.2f" % (plain_ms / st["device_ms"])
        say("n=%-7d %-22s rc=%d %7d decisions %7d moves (%d 2-opt, %d Or-opt, %d 3-opt) %10.1f ms device  %.1f us/decision  "
            "cost %.0f%s" % (n, rule, rc, st["decisions"], st["moves"], st["moves_2opt"], st["moves_oropt"], st["moves_3opt"],
                             st["device_ms"], 1e3 * st["device_ms"] / max(1, st["decisions"]), o, ratio))

    if a.label:
        say("# " + a.label)
    ctx = E.Context(0)
    for n in [int(x) for x in a.sizes.split(",")]:
        xy = rand_instance(n)
        inst = E.Instance(ctx, xy, E.EUC_2D, 1)
        knn_ms = inst.knn_build(K)
        succ, obj = inst.greedy_edge()
        say("n=%-7d greedy_edge cost %.0f, KNN-%d lists %.1f ms" % (n, obj, K, knn_ms))
        inst.nl_3opt(succ, max_moves=8)                                   # warm-up: module load, scratch
        rc, s, o, st = inst.nl_3opt(succ, time_limit=a.limit)
        row(n, "plain", rc, st, o, None)
        plain_ms = st["device_ms"] if rc == 0 else None
        if not a.plain_only:
            inst.nl_3opt_batch(succ, max_moves=8)
            for max_arc, rounds in SETTINGS:
                rc, s, ob, st = inst.nl_3opt_batch(succ, max_arc=max_arc, rounds=rounds, time_limit=a.limit)
                row(n, "max_arc=%s rounds=%d" % ("n/2" if max_arc <= 0 else max_arc, rounds), rc, st, ob, plain_ms)
                say("n=%-7d %-22s cost / cost(plain) = %.4f" % (n, "", ob / o))
        inst.close()
    ctx.close()
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
