"""The cases on which the two-phase ascent (tsp_dev_held_karp_sparse) is compared step by step: the cases of hk_trace_cases.py,
each with candidate lists.  One list for test_cpu_hk_sparse.py (the reference's own spread under the summation order) and
test_gpu_hk_sparse.py (the device against the reference).

Lists: the K nearest nodes by (d, id) on the case's own matrix (hk_sparse_ref.knn_lists), K = 5; K = 3 for the clustered family,
whose candidate graphs then fall into several components, so that every tree has a completion."""
import hk_sparse_ref as S
import hk_trace_cases as T

K_ITERS = 40     # sparse iterations compared per case
DENSE_AFTER = 5  # dense iterations behind them in the stability check

# Removed by name, with the reason (test_cpu_hk_sparse.py::test_every_case_is_stable_under_the_summation_order fails on them):
UNSTABLE = {
    "pr76-int1-pat3": "a near-tie between two candidate edges: some of the 10 summation orders build another tree within 40 iterations",
    "pr76-int0-pat3": "the same near-tie with real costs",
    "berlin52-int1-pat3-start7": "the trees and lambda agree, but W_C passes close to zero from this start and `best`, measured "
                                 "relative to itself, moves by 2.4e-13 (cancellation, as kroA100's seeded start in hk_trace_cases.py)",
}


def list_k(case):
    return 3 if case.name.startswith("clustered") else 5


CASES = [c for c in T.CASES if c.id not in UNSTABLE]
IDS = [c.id for c in CASES]


def lists(case, D):
    return S.knn_lists(D, list_k(case))


def trace(case, D, nbr, sparse_iters=K_ITERS, dense_iters=DENSE_AFTER, sum_order=None, rounds=False):
    return S.ascent_trace_sparse(D, nbr, case.ub, sparse_iters, dense_iters, case.lambda0, case.patience, case.start(D), sum_order,
                                 rounds)
