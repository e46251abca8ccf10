"""The cases on which the Held-Karp ascent is compared step by step (test_cpu_held_karp.py: the reference's own spread and that
the comparison can fail; test_gpu_held_karp.py: the device against the reference).  One list, so both see the same numbers.

ub is a constant written here, the same for both cost settings (it only scales the steps): 1.07 x the published optimum
where the instance has one under its own metric (berlin52 7542, eil51 426, pr76 108159, kroA100 21282, att48 10628, burma14
3323, ulysses22 7013), and 1.3 x the reference's W(0) with integer costs for berlin52's coordinates under CEIL_2D (6201) and
under MAN_2D / MAX_2D (1730; both are |dx|, the reference's `dy = |y2 - y2|`).  1.3 x W(0) was not taken for burma14: it lies
below that instance's optimum, W settles on it after 13 iterations, every later step is 0 and two of the seven mutations of
test_cpu_held_karp.py change nothing.

Tried and left out: kroA100 from a seeded start (W crosses zero in iteration 6, and `best`, measured relative to itself, moves
by 2.9e-14 under the summation order -- cancellation, not a tie; the trees are the same) -- the starts kept are two whose
first W is not that close to zero."""
import os

import numpy as np

import held_karp_ref as HK
from helpers import INSTANCES
from oracle import oracle as O

K = 40   # iterations compared per case
UB = {("berlin52", None): 8069.94, ("eil51", None): 455.82, ("pr76", None): 115730.13, ("kroA100", None): 22771.74,
      ("berlin52", O.CEIL_2D): 8061.3, ("berlin52", O.MAN_2D): 2249.0, ("berlin52", O.MAX_2D): 2249.0, ("att48", None): 11371.96,
      ("burma14", None): 3555.61, ("ulysses22", None): 7503.91}


def clustered(seed):
    """-> (xy, lambda0, patience): 30 to 100 integer points in 2 to 8 clusters whose diameters go from a few units to a third
    of the field, and a large lambda0 -- the family tools/hk_round_jumps.py searches for trees whose number of Boruvka rounds
    jumps (the penalties of a long step pull the tree into a star of one round; the next one is back at three or four)"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(30, 101))
    k = int(rng.integers(2, 9))
    centres = rng.uniform(0, 1e5, size=(k, 2))
    diam = 10.0 ** rng.uniform(0, 4.5, size=k)
    which = rng.integers(0, k, size=n)
    xy = np.rint(centres[which] + rng.uniform(-0.5, 0.5, size=(n, 2)) * diam[which, None])
    return xy, float(rng.choice([2.0, 8.0, 32.0])), int(rng.choice([1, 3, 0]))


class Case:
    def __init__(self, name, wt_as=None, integer_cost=1, patience=3, lambda0=2.0, start_seed=None, ub=None):
        self.name, self.wt_as, self.integer_cost, self.patience, self.lambda0 = name, wt_as, integer_cost, patience, lambda0
        self.start_seed = start_seed   # None: pi = 0; else uniform in +- 0.5 x the mean distance from this seed
        self.ub = UB[name, wt_as] if ub is None else ub
        self.id = "%s%s-int%d-pat%d%s%s" % (name, "" if wt_as is None else "-as%d" % wt_as, integer_cost, patience,
                                           "" if lambda0 == 2.0 else "-lam%g" % lambda0,
                                           "" if start_seed is None else "-start%d" % start_seed)

    def load(self):
        """-> (xy, metric)"""
        if self.name.startswith("clustered"):
            return clustered(int(self.name[9:]))[0], O.EUC_2D
        xy, wt = O.parse_tsplib(os.path.join(INSTANCES, self.name + ".tsp"))
        return xy, (wt if self.wt_as is None else self.wt_as)

    def matrix(self):
        """The oracle's distances (for GEO the device tests take the device's own matrix instead: its tolerance tier)"""
        xy, wt = self.load()
        return O.dist_matrix(xy, wt, self.integer_cost)

    def start(self, D):
        if self.start_seed is None:
            return None
        n = len(D)
        return np.random.default_rng(self.start_seed).uniform(-0.5, 0.5, n) * D[np.triu_indices(n, 1)].mean()

    def trace(self, D, iters=K, sum_order=None):
        return HK.ascent_trace(D, self.ub, iters, self.lambda0, self.patience, self.start(D), sum_order)


# every metric x both cost settings with patience 3 (the stall logic acts many times within K iterations) ...
CASES = [Case(name, wt_as, ic) for name, wt_as in (("berlin52", None), ("berlin52", O.CEIL_2D), ("berlin52", O.MAN_2D),
                                                   ("berlin52", O.MAX_2D), ("att48", None), ("eil51", None), ("pr76", None),
                                                   ("kroA100", None), ("burma14", None), ("ulysses22", None))
         for ic in (1, 0)]
# ... the default patience (0 -> max(10, n / 20)), another lambda0, a start that is not zero
CASES += [Case("berlin52", patience=0), Case("eil51", integer_cost=0, patience=0), Case("pr76", patience=0),
          Case("kroA100", integer_cost=0, patience=0), Case("att48", patience=0), Case("ulysses22", patience=0),
          Case("eil51", lambda0=1.25), Case("berlin52", start_seed=7), Case("eil51", integer_cost=0, start_seed=7)]
# ... and two of the clustered family in which the host has to repeat an iteration (REPEATS below): lambda0 = 32, the default
# patience, ub = 1.3 x W(0).  Their steps are so long that W never passes W(0) again within K iterations: best and pi_best stay
# at the start; lambda (32 -> 4), the counts and the rounds (1 to 4 per tree) are what these two compare.
CASES += [Case("clustered5", patience=0, lambda0=32.0, ub=229845.2), Case("clustered31", patience=0, lambda0=32.0, ub=286062.4)]
IDS = [c.id for c in CASES]

# berlin52 from ub = 8100, patience 3, lambda0 2: the reference's ascent ends on the optimal tour.
# integer_cost -> (best, the (iterations, lambda at the end) that summation order allows).  With integer costs the run is NOT
# stable under the summation order: W differs in its last bits from iteration 2 on, the tree of iteration 6 has a near-tie that
# those bits decide, and of 10 seeded orders 7 end after 49 iterations (as fsum does) and 3 after 60; both on the optimal tour.
TOUR_UB = 8100.0
TOUR_ENDS = {1: (7542.0, [(49, 2.0 ** -6), (60, 2.0 ** -8)]), 0: (7544.365901904089, [(62, 2.0 ** -8)])}

# the cases in which a call with max_iters <= K repeats an iteration (short_queues below; test_cpu_held_karp.py checks the list):
# clustered5 iterations 4 (first of its batch of four) and 12 (fifth of eight: three queued trees behind it become no-ops),
# clustered31 iterations 5 and 16
REPEATS = {"clustered5-int1-pat0-lam32", "clustered31-int1-pat0-lam32"}

TOL = 1e-12   # what test_gpu_held_karp.check_tree allows W for summation order


def deviation(step, best, pi_best):
    """(|best - step.best| relative to step.best, max|pi_best - step.pi_best| relative to max(1, max|step.pi_best|))"""
    return (abs(best - step.best) / abs(step.best),
            float(np.abs(np.asarray(pi_best) - step.pi_best).max()) / max(1.0, float(np.abs(step.pi_best).max())))


def short_queues(rounds, max_iters):
    """tsp_dev_held_karp queues the trees of a batch (1, 2, 4 ... 64 iterations) with one round more than the last tree before
    the batch took (the first with all ceil(log2(n - 1))); a tree that needs more stops the batch and is repeated with all.
    rounds[k - 1] = the rounds tree k needs -> [(iteration from 1, rounds it was queued with)] for the iterations that a call
    with max_iters repeats.  (The scans of those rounds are in the call's dists_executed and in none of its other counts.)"""
    full = 32
    R, batch, it, hits = full, 1, 0, []
    last = min(max_iters, len(rounds))
    while it < last:
        short = False
        for _ in range(min(batch, last - it)):
            if rounds[it] > R:
                short = True
                hits.append((it + 1, R))
                break
            it += 1
        R = full if short else rounds[it - 1] + 1
        batch = min(2 * batch, 64)
    return hits
