"""CPU search for an ascent in which tsp_dev_held_karp would have to repeat an iteration: a tree that needs
more Boruvka rounds than the batch it is in was queued with (one more than the last tree before the batch took).  Seeded
instances, n <= 100, clusters of very different diameters, large lambda0; the reference ascent (tests/held_karp_ref.py) gives
the trees, tests/hk_trace_cases.short_queues the host's batches.  Prints every instance with a rise of two or more rounds
between consecutive trees or with a repeated iteration, and the totals.

    python tools/hk_round_jumps.py [instances = 300] [iterations = 25]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import held_karp_ref as HK   # noqa: E402
import hk_trace_cases as T   # noqa: E402
from oracle import oracle as O   # noqa: E402


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    jumps = repeats = 0
    top = 0
    for seed in range(count):
        xy, lambda0, patience = T.clustered(seed)
        D = O.dist_matrix(xy, O.EUC_2D, 1)
        ub = 1.3 * HK.one_tree(D)[2]
        steps = HK.ascent_trace(D, ub, iters, lambda0, patience)
        rounds = [HK.boruvka_rounds(D, s.pi) for s in steps]
        jump = max([b - a for a, b in zip(rounds, rounds[1:])], default=0)
        hits = sorted({k for m in range(1, iters + 1) for k, _ in T.short_queues(rounds, m)})
        top = max(top, jump)
        if jump >= 2 or hits:
            jumps += jump >= 2
            repeats += bool(hits)
            print("seed %d: n %d, lambda0 %g, patience %d, rounds %s, repeated iterations %s" % (seed, len(xy), lambda0, patience, rounds, hits))
    print("%d instances x %d iterations: %d with a rise of >= 2 rounds (largest rise %d), %d with a repeated iteration"
          % (count, iters, jumps, top, repeats))


if __name__ == "__main__":
    main()
