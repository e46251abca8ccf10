"""GPU: minimum 1-trees and the Held-Karp ascent on the device (tsp_dev_one_tree, tsp_dev_held_karp, tsp_host_lower_bound)
against the CPU reference of the definitions (tests/held_karp_ref.py).  Trees are decision-exact: edges and degrees equal the
reference's; values agree to summation order."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import held_karp_ref as HK
import hk_trace_cases as T
from helpers import INSTANCES, Instance, HostInstance, rand_instance
from oracle import oracle as O

pytestmark = pytest.mark.gpu
OPTIMA = {"berlin52": 7542, "eil51": 426, "pr76": 108159, "kroA100": 21282, "pr299": 48191}


@pytest.fixture(scope="module")
def eng():
    from tsp_optimization_amd import engine as E
    assert E.device_count() >= 1
    return E


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.Context(0)
    yield c
    c.close()


def tie_grid(n=30, seed=5):
    return np.random.default_rng(seed).integers(0, 4, size=(n, 2)).astype(np.float64)


def load(name):
    if name == "grid30":
        return tie_grid(), O.EUC_2D
    return O.parse_tsplib(os.path.join(INSTANCES, name + ".tsp"))


def check_tree(inst, D, pi, what):
    edges, deg, value, st = inst.one_tree(pi, want_stats=True)
    re_, rd, rv, _ = HK.one_tree(D, pi)
    print("%s: W %.6f (reference %.6f, relative difference %.2e), %d rounds" % (what, value, rv, abs(value - rv) / abs(rv), st["rounds"]))
    assert (edges == re_).all(), what
    assert (deg == rd).all() and deg.sum() == 2 * inst.n, what
    assert abs(value - rv) <= 1e-12 * abs(rv), (what, value, rv)
    assert st["trees"] == 1 and st["rounds"] >= 1 and st["dists_executed"] >= st["rounds"] * (inst.n - 1) * (inst.n - 1)
    return value


# the six metrics x both integer_cost settings; MAX_2D and MAN_2D (which no fixture names) on berlin52's coordinates
TREE_CASES = [("burma14", None), ("ulysses22", None), ("att48", None), ("berlin52", None), ("berlin52", O.MAX_2D),
              ("berlin52", O.MAN_2D), ("pr1002", None), ("dsj1000", None), ("grid30", None)]


@pytest.mark.parametrize("integer_cost", [1, 0])
@pytest.mark.parametrize("name,wt_as", TREE_CASES)
def test_one_tree_is_decision_exact(eng, ctx, name, wt_as, integer_cost):
    xy, wt = load(name)
    wt = wt if wt_as is None else wt_as
    inst = eng.Instance(ctx, xy, wt, integer_cost)
    # GEO is the tolerance tier (cos / acos differ in the last ulp between libraries): its trees are compared on the device's own distances
    D = inst.dist_matrix()[0] if wt == O.GEO else O.dist_matrix(xy, wt, integer_cost)
    n = len(xy)
    scale = D[np.triu_indices(n, 1)].mean()
    rng = np.random.default_rng(1000 + n)
    for k, pi in enumerate((None, rng.uniform(-0.5, 0.5, n) * scale, rng.uniform(-1.0, 1.0, n) * scale)):
        check_tree(inst, D, pi, "%s wt %d int %d pi#%d" % (name, wt, integer_cost, k))
    inst.close()


def test_metric_coverage_of_the_tree_cases():
    seen = {(load(n)[1] if w is None else w) for n, w in TREE_CASES}
    assert seen == {O.EUC_2D, O.MAX_2D, O.MAN_2D, O.CEIL_2D, O.GEO, O.ATT}


@pytest.mark.parametrize("n", [10000, 20011])
def test_one_tree_at_scale(eng, ctx, n):
    xy = rand_instance(n)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    R = HK.Euc2DRows(xy)
    rng = np.random.default_rng(n)
    for k, pi in enumerate((None, rng.uniform(-0.5, 0.5, n) * 5.2e5)):   # 5.2e5: the mean distance of two uniform points in [0, 1e6)^2
        check_tree(inst, R, pi, "rand%d pi#%d" % (n, k))
    inst.close()


def local_optimum(eng, inst):
    succ, obj, status = inst.construct(eng.GREEDY, np.array([0], dtype=np.int32))
    assert status[0] == 0
    rc, s, o, _, _ = inst.two_opt_or_opt(succ[0], obj[0])
    assert rc == 0
    return o


@pytest.fixture(scope="module")
def ascents(eng, ctx):
    """name -> (D, ub, W(0), device bound, pi_best, stats) for the default 300-iteration ascent"""
    out = {}
    for name in ("berlin52", "eil51", "pr76", "kroA100", "pr299", "pr1002"):
        xy, wt = load(name)
        inst = eng.Instance(ctx, xy, wt, 1)
        D = O.dist_matrix(xy, wt, 1)
        ub = local_optimum(eng, inst)
        w0 = inst.one_tree()[2]
        bound, pi_best, st = inst.held_karp(ub)
        inst.close()
        print("%s: ub %.0f, W(0) %.1f, bound %.3f after %d iterations / %d rounds, gap %.4f, %.1f ms on the device"
              % (name, ub, w0, bound, st["iterations"], st["rounds"], (ub - bound) / bound, st["device_ms"]))
        out[name] = (D, ub, w0, bound, pi_best, st)
    return out


@pytest.mark.parametrize("name", ["berlin52", "eil51", "pr76", "kroA100", "pr299", "pr1002"])
def test_the_ascent_returns_a_true_lagrangian_value(ascents, name):
    D, ub, w0, bound, pi_best, st = ascents[name]
    rv = HK.one_tree(D, pi_best)[2]
    print("%s: bound %.6f, reference W(pi_best) %.6f" % (name, bound, rv))
    assert abs(rv - bound) <= 1e-9 * abs(bound)
    assert bound <= ub
    assert bound >= w0
    assert st["status"] == 0 and 1 <= st["iterations"] <= 300 and st["trees"] >= st["iterations"]
    if name in OPTIMA:
        assert bound <= OPTIMA[name] * (1 + 1e-9)
    if name == "berlin52":
        assert math.ceil(bound - 1e-6) == 7542


@pytest.mark.parametrize("name", ["berlin52", "eil51", "pr76", "kroA100", "pr299"])
def test_ascent_quality_against_the_reference_ascent(ascents, name):
    """Same ub, 300 iterations, defaults.  Trajectories need not match bit for bit (summation order; a near-tie can flip a
    tree), the bounds must agree to 1e-3: a CPU prototype of this schedule moved by at most 2.2e-5 relative when ub went from
    1.05 x to 1.15 x the optimum on these five instances."""
    D, ub, _, bound, _, st = ascents[name]
    ref, _, info = HK.ascent(D, ub, 300)
    print("%s: device %.4f (%d iterations), reference %.4f (%d iterations), relative difference %.2e, %.4f of the optimum"
          % (name, bound, st["iterations"], ref, info["iterations"], abs(bound - ref) / ref, bound / OPTIMA[name]))
    assert abs(bound - ref) <= 1e-3 * ref


@pytest.mark.parametrize("case", T.CASES, ids=T.IDS)
def test_ascent_trajectory_equals_the_reference(eng, ctx, case):
    """The schedule step by step: calls with max_iters = 1 .. K (each a prefix of the next: the ascent is deterministic; they
    cross the host's batches of 1, 2, 4, 8, 16 and `done` inside a batch) against entry k of the reference's trace.  lambda,
    the counts, the Boruvka rounds and the weights scanned (which alone show an iteration that the host had to repeat) are
    equal; best and pi_best agree to the 1e-12 that check_tree gives W for summation order, which is all that separates the
    two by design -- test_cpu_held_karp.py holds every case to the same trees and to 1e-14 under ten other orders, and shows
    that seven one-line changes of the schedule leave this band.  Measured on an MI355X: 8.0e-16 and 1.6e-15 at worst."""
    xy, wt = case.load()
    inst = eng.Instance(ctx, xy, wt, case.integer_cost)
    D = inst.dist_matrix()[0] if wt == O.GEO else case.matrix()   # GEO: the device's own distances, as the tree test
    ref = case.trace(D)
    start = case.start(D)
    per_tree = [HK.boruvka_rounds(D, s.pi) for s in ref]
    rounds = np.cumsum(per_tree)
    worst_b = worst_p = 0.0
    wrong = []
    scan = repeats = 0
    for k in range(1, T.K + 1):
        r = ref[min(k, len(ref)) - 1]   # (a reference that has stopped on a tour stays at its last entry)
        bound, pi_best, st = inst.held_karp(case.ub, max_iters=k, lambda0=case.lambda0, patience=case.patience, pi=start)
        db, dp = T.deviation(r, bound, pi_best)
        worst_b, worst_p = max(worst_b, db), max(worst_p, dp)
        if k == 1:   # weights per round; the first tree is queued with every round it can need
            scan = st["dists_executed"] // per_tree[0]
        # an iteration that the host repeats (T.short_queues) shows in nothing but the scans of its first, short, attempt
        again = T.short_queues(per_tree, k)
        repeats = max(repeats, len(again))
        got = (st["status"], st["lambda_final"], st["iterations"], st["trees"], st["tour_found"], st["rounds"], st["dists_executed"])
        want = (0, r.lam, r.k, r.k, int(r.g2 == 0.0), int(rounds[r.k - 1]), (int(rounds[r.k - 1]) + sum(q for _, q in again)) * scan)
        if got != want or not db <= T.TOL or not dp <= T.TOL:
            wrong.append((k, got, want, db, dp))
    inst.close()
    print("%s: %d calls, %d reference iterations (%s), lambda %g -> %g, %d rounds, %d iterations repeated; worst deviation of the "
          "bound %.2e, of pi_best %.2e" % (case.id, T.K, len(ref), "ends on a tour" if ref[-1].g2 == 0.0 else "no tour",
                                           case.lambda0, ref[-1].lam, rounds[-1], repeats, worst_b, worst_p))
    assert not wrong, wrong[:3]
    assert (repeats > 0) == (case.id in T.REPEATS)


@pytest.mark.parametrize("integer_cost", [1, 0])
def test_ascent_ends_on_the_tour(eng, ctx, integer_cost):
    """berlin52 from ub = 8100, patience 3, lambda0 2: the ascent stops on the optimal tour (|g|^2 = 0) before max_iters.
    Non-integer costs: 62 iterations, 7544.3659..., lambda 2^-8.  Integer costs: the reference takes 49 iterations to 7542
    with lambda 2^-6, but that run is not stable under the summation order (hk_trace_cases.TOUR_ENDS,
    test_cpu_held_karp.test_berlin52_ends_on_the_tour): a near-tie in iteration 6 sends 3 of 10 orders to the same tour after
    60 iterations with lambda 2^-8, so either end is the definition's."""
    xy, wt = load("berlin52")
    inst = eng.Instance(ctx, xy, wt, integer_cost)
    best, ends = T.TOUR_ENDS[integer_cost]
    bound, pi_best, st = inst.held_karp(T.TOUR_UB, max_iters=120, lambda0=2.0, patience=3)
    deg = inst.one_tree(pi_best)[1]
    inst.close()
    print("berlin52 int %d: %d iterations, bound %.9f, lambda %g, %d rounds" % (integer_cost, st["iterations"], bound,
                                                                               st["lambda_final"], st["rounds"]))
    assert st["status"] == 0 and st["tour_found"] == 1 and st["trees"] == st["iterations"]
    assert (st["iterations"], st["lambda_final"]) in ends
    assert abs(bound - best) <= 1e-12 * best
    assert (deg == 2).all()


def test_determinism_and_small_cases(eng, ctx):
    xy, wt = load("pr299")
    inst = eng.Instance(ctx, xy, wt, 1)
    ub = 1.1 * OPTIMA["pr299"]
    b1, p1, s1 = inst.held_karp(ub, max_iters=120)
    b2, p2, s2 = inst.held_karp(ub, max_iters=120)
    assert np.float64(b1).tobytes() == np.float64(b2).tobytes() and p1.tobytes() == p2.tobytes()
    assert s1["iterations"] == s2["iterations"] == 120 and s1["rounds"] == s2["rounds"]
    # one iteration = the tree of the start
    assert inst.held_karp(ub, max_iters=1)[0] == inst.one_tree()[2]
    start = np.random.default_rng(3).uniform(-300.0, 300.0, inst.n)
    b3, p3, _ = inst.held_karp(ub, max_iters=1, pi=start)
    assert b3 == inst.one_tree(start)[2] and (p3 == start).all()
    # ... and a start is where the ascent goes on from: 60 iterations from the result of 60 are no worse than it
    b60, p60, _ = inst.held_karp(ub, max_iters=60)
    assert inst.held_karp(ub, max_iters=60, pi=p60)[0] >= b60
    inst.close()
    for n in (3, 4):
        xy = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 7.0], [0.0, 7.0]])[:n]
        inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
        D = O.dist_matrix(xy, O.EUC_2D, 1)
        check_tree(inst, D, None, "n = %d" % n)
        check_tree(inst, D, np.array([1.5, -2.0, 0.25, 3.0])[:n], "n = %d with penalties" % n)
        tour = float(sum(D[k, (k + 1) % n] for k in range(n)))
        bound, _, st = inst.held_karp(tour)
        assert bound == tour and st["tour_found"] == 1   # every 1-tree of 3 nodes is the tour; the rectangle's is one too
        inst.close()


def test_bad_arguments(eng, ctx):
    with pytest.raises(eng.TspDeviceError, match="-3"):
        eng.Instance(ctx, np.array([[0.0, 0.0], [1.0, 1.0]]), O.EUC_2D, 1)   # n = 2: no handle to ask with
    L = eng.lib()
    bound = C.c_double(0)
    assert L.tsp_dev_held_karp(None, 100.0, 10, 2.0, 0, -1.0, None, C.byref(bound), None) == eng.E_ARG
    assert L.tsp_dev_one_tree(None, None, None, None, None, None) == eng.E_ARG
    xy, wt = load("berlin52")
    inst = eng.Instance(ctx, xy, wt, 1)
    for ub in (0.0, -5.0, float("nan"), float("inf")):
        with pytest.raises(eng.TspDeviceError, match="-3.*tsp_dev_held_karp"):
            inst.held_karp(ub)
        assert b"tsp_dev_held_karp" in L.tsp_dev_last_error()
    with pytest.raises(eng.TspDeviceError, match="-3"):
        inst.held_karp(8000.0, max_iters=0)
    with pytest.raises(eng.TspDeviceError, match="-3"):
        inst.one_tree(np.full(inst.n, np.nan))
    with pytest.raises(eng.TspDeviceError, match="-3"):
        inst.one_tree(np.zeros(inst.n - 1))
    assert inst.held_karp(8000.0, max_iters=5)[0] <= 7542   # the handle still works
    inst.close()


def test_time_limit_returns_a_valid_bound(eng, ctx):
    xy = rand_instance(10000)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    ub = 0.7124 * math.sqrt(10000 * 1e12) * 1.25   # above any local optimum of 10 000 uniform points (0.7124 sqrt(n A) is the limit constant of the optimum)
    bound, pi_best, st = inst.held_karp(ub, time_limit=1e-3)
    print("rand10000, 1 ms: %d iterations, bound %.1f, %.2f ms" % (st["iterations"], bound, st["device_ms"]))
    assert st["status"] == eng.TIME_LIMIT_EXCEEDED
    assert math.isfinite(bound) and bound <= ub and 1 <= st["iterations"] < 300
    assert np.isfinite(pi_best).all()
    inst.close()


def test_host_library_equals_the_device_api(eng, ctx):
    from tsp_optimization_amd.build import lib_path
    L = C.CDLL(lib_path("libtsp_host.so"))
    L.tsp_host_lower_bound.restype = C.c_double
    L.tsp_host_lower_bound.argtypes = [C.POINTER(Instance), C.c_double, C.c_int, C.c_double]
    L.tsp_host_last_lb_stats.argtypes = [C.POINTER(eng.LbStats)]
    h = HostInstance("pr1002")
    ub = 290000.0
    got = L.tsp_host_lower_bound(C.byref(h.c), ub, 80, -1.0)
    hs = eng.LbStats()
    L.tsp_host_last_lb_stats(C.byref(hs))
    L.tsp_host_shutdown()
    inst = eng.Instance(ctx, h.xy, h.wt, 1)
    bound, _, st = inst.held_karp(ub, max_iters=80)
    inst.close()
    assert np.float64(got).tobytes() == np.float64(bound).tobytes()
    assert (hs.iterations, hs.rounds, hs.tour_found) == (st["iterations"], st["rounds"], st["tour_found"]) and hs.iterations == 80
    assert got <= 259045   # pr1002's optimum
