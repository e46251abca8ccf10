"""The cases of tests/golden/tabu_chains.json and the ways the GPU test cuts their iterations into calls: shared by the generator
(tests/golden/make_golden_tabu.py), tests/test_cpu_tabu_ref.py and tests/test_gpu_tabu_oracle.py."""
import numpy as np

from oracle import oracle as O
from helpers import load_instance, rand_instance
import tabu_ref as T

# checkpoints after these iterations (those a case reaches): tour hash, non-zero stamps, incumbent.  32 is there so that a run
# of 64 iterations cut into eights still passes three of them.
CHECKPOINTS = (1, 8, 32, 64, 128, 256)

# name -> (instance, integer_cost, iterations, tenures: "linear" or "drawn", seed of the pair stream)
#   pr1002    integer coordinates: the *_ICOORD metric and the float replica; 34 workgroups by default
#   att532    ATT; 12 workgroups; tenures drawn per iteration from {0, 1, 2} and [lo, hi] (tenure 0: every stamp of an earlier
#             iteration has expired, the kick's own two are what is left)
#   d493      fractional coordinates: the general EUC_2D metric and the double replica
#   rand3000  ng = 47 groups of 64 -> 1128 group pairs, (1128 + 3) / 4 = 282 >= 256: the smallest size class whose cluster is 256
#             workgroups with group pairs for every one of them
#   ceil1500  CEIL_2D, the third sqrt metric, on seeded integer coordinates in [0, 500 000)
CASES = {
    "pr1002": ("pr1002", 1, 256, "linear", 1002),
    "att532": ("att532", 1, 256, "drawn", 532),
    "d493": ("d493", 1, 128, "linear", 493),
    "rand3000": ("rand3000", 1, 128, "linear", 3000),
    "ceil1500": (("rand", 1500, 77, 500_000, O.CEIL_2D), 1, 64, "linear", 1500),
}
HOST_RUNS = [("pr1002", 0), ("pr1002", 1), ("pr1002", 2), ("att532", 0)]
HOST_ITERATIONS = 300

# The calls a run's iterations are cut into, as lengths over 256 iterations (a shorter case takes the prefix that fits).
#   "steps"  [1, 7, 56, 64, 128]
#   "eights" all 8s
#   "host"   chains of 128, the length tsp_host_tabu asks for, with its P = K + K / 3 + 4 pairs (a run of 64 iterations: one chain)
#   "exact"  P == K: the pairs run out inside a chain wherever a trial is rejected
SPLITS = {
    "steps": [1, 7, 56, 64, 128],
    "eights": [8] * 32,
    "host": [128, 128],
    "exact": [8, 24, 32, 64, 128],
}


def split_calls(split, iterations):
    out, done = [], 0
    for k in ([iterations] if split == "host" and iterations < 128 else SPLITS[split]):
        if done + k > iterations:
            break
        out.append(k)
        done += k
    assert done == iterations, (split, iterations)
    return out


def pairs_of_call(split, K):
    """How many pairs of the stream a chain of K iterations is handed (tsp_host.c: K + K / 3 + 4, at most 256)"""
    return K if split == "exact" else min(K + K // 3 + 4, 256)


def checkpoints_of(iterations):
    return [c for c in CHECKPOINTS if c <= iterations]


def instance_of(case):
    """-> (xy, wtype, integer_cost)"""
    spec, ic = CASES[case][0], CASES[case][1]
    if isinstance(spec, tuple):
        _, n, seed, hi, wt = spec
        return rand_instance(n, seed=seed, hi=hi), wt, ic
    xy, wt = load_instance(spec)
    return xy, wt, ic


def tenures_of(case, n, iterations):
    kind = CASES[case][3]
    if kind == "linear":
        return T.policy_tenures(n, 1, iterations)
    lo, hi = T.tenure_bounds(n)
    rng = np.random.default_rng(CASES[case][4] + 1)
    pool = [0, 1, 2] + list(range(lo, hi + 1))
    # half of the draws from {0, 1, 2}: among the 46 values of [lo, hi] they would come up once in sixteen iterations
    return [int(rng.choice([0, 1, 2])) if rng.random() < 0.5 else int(rng.choice(pool)) for _ in range(iterations)]


def workgroups_natural(n):
    """tsp_cluster_size's default for the sorted scan of one tour: a quarter of the group pairs, at most 256"""
    ng = (n + 63) // 64
    return min(256, (ng * (ng + 1) // 2 + 3) // 4)
