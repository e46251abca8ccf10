"""Or-opt on the device (tsp_dev_or_opt, tsp_dev_two_opt_or_opt) against the CPU reference of the definition in
include/tsp_hip.h (tests/or_opt_ref.py): tours bit for bit and every counter for the integer-valued metrics and --fcost,
the incremental path against a full sweep per decision, batches, move caps, a GRID-sized instance, GEO at the tolerance
tier, and the error paths."""
import ctypes as C
import os

import numpy as np
import pytest

import or_opt_ref as R
from helpers import golden, load_instance, rand_instance, random_tour
from oracle import oracle as O

pytestmark = pytest.mark.gpu

COUNTERS = ("sweeps", "evals", "moves", "moves_by_len", "moves_reversed")


@pytest.fixture(scope="module")
def eng():
    from tsp_optimization_amd import engine as E
    assert E.device_count() >= 1, "no HIP device visible: the product path has no CPU fallback"
    return E


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.Context(0)
    yield c
    c.close()


def _oropt(inst, succ, *a, **kw):
    kw.setdefault("time_limit", 120.0)     # a descent that does not end is a failure, not a hang
    return inst.or_opt(succ, *a, **kw)


def _composite(inst, succ, *a, **kw):
    kw.setdefault("time_limit", 120.0)
    return inst.two_opt_or_opt(succ, *a, **kw)


def _cost_ok(xy, wt, succ, obj, ic):
    ref = O.succ_cost(xy, wt, succ, ic)
    return obj == ref if ic else abs(obj - ref) <= 1e-9 * abs(ref)


def _same(dev_succ, dev_obj, dev_st, ref_succ, ref_c, xy, wt, ic):
    assert O.is_tour(dev_succ)
    assert (dev_succ == ref_succ).all(), "tour differs from the reference"
    assert _cost_ok(xy, wt, dev_succ, dev_obj, ic), dev_obj
    for k in COUNTERS:
        assert dev_st[k] == ref_c[k], (k, dev_st[k], ref_c[k])


@pytest.mark.parametrize("ic", [1, 0])
@pytest.mark.parametrize("name", ["berlin52", "pr299", "d657", "att532", "dsj1000", "pr1002"])
def test_descent_from_two_opt_optimum_of_greedy(eng, ctx, name, ic):
    xy, wt = load_instance(name)
    _, es, eo = O.greedy(xy, wt, 0, ic)
    _, s2, o2, _, _ = O.two_opt_first(xy, wt, es, eo, ic)
    inst = eng.Instance(ctx, xy, wt, ic)
    rc, s, o, st = _oropt(inst, s2, o2)
    inst.close()
    ref, c = R.or_opt_descent(xy, wt, s2, ic)
    assert rc == 0 and c["moves"] > 0
    _same(s, o, st, ref, c, xy, wt, ic)
    assert st["sweeps"] == st["moves"] + 1 and st["deltas_executed"] > 0 and st["rounds"] == 0


@pytest.mark.parametrize("n,seed,cap", [(200, 1, -1), (200, 2, -1), (500, 1, -1), (500, 2, -1), (1000, 1, 150), (1000, 2, 150)])
def test_descent_from_random_tours(eng, ctx, n, seed, cap):
    xy = rand_instance(n, seed=1000 + n + seed)
    succ = random_tour(n, np.random.default_rng(seed))
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    rc, s, o, st = _oropt(inst, succ, max_moves=cap)
    inst.close()
    ref, c = R.or_opt_descent(xy, O.EUC_2D, succ, 1, max_moves=cap)
    assert rc == 0 and c["moves"] >= 100
    _same(s, o, st, ref, c, xy, O.EUC_2D, 1)


@pytest.mark.parametrize("side", [10, 14, 20])
def test_tie_rule_on_lattices(eng, ctx, side):
    g = np.array([(x, y) for x in range(side) for y in range(side)], dtype=np.float64) * 100
    succ = random_tour(len(g), np.random.default_rng(side))
    inst = eng.Instance(ctx, g, O.EUC_2D, 1)
    rc, s, o, st = _oropt(inst, succ)
    inst.close()
    ref, c = R.or_opt_descent(g, O.EUC_2D, succ, 1)
    assert rc == 0
    _same(s, o, st, ref, c, g, O.EUC_2D, 1)


def _full_and_incremental(eng, ctx, xy, wt, succ, ic=1, max_moves=-1):
    out = []
    for full in ("1", None):
        if full:
            os.environ["TSP_OROPT_FULL"] = full
        try:
            inst = eng.Instance(ctx, xy, wt, ic)
            out.append(_oropt(inst, succ, max_moves=max_moves))
            inst.close()
        finally:
            os.environ.pop("TSP_OROPT_FULL", None)
    (r1, s1, o1, st1), (r2, s2, o2, st2) = out
    assert r1 == r2 == 0 and (s1 == s2).all() and o1 == o2
    for k in COUNTERS + ("rounds",):
        assert st1[k] == st2[k], k
    assert st2["deltas_executed"] < st1["deltas_executed"]
    return s2, o2, st2


@pytest.mark.parametrize("name", ["pr1002", "rand5000"])
def test_incremental_equals_full_sweeps(eng, ctx, name):
    xy, wt = load_instance(name)
    succ = random_tour(len(xy), np.random.default_rng(5))
    _, _, st = _full_and_incremental(eng, ctx, xy, wt, succ, max_moves=3000)
    assert st["moves"] > 500


def test_incremental_work_rand10000(eng, ctx):
    """greedy -> alg_2opt -> Or-opt on rand10000: the incremental path executes at most 5 % of the logical evaluations."""
    xy, wt = load_instance("rand10000")
    inst = eng.Instance(ctx, xy, wt, 1)
    succ, obj, _ = inst.construct(eng.GREEDY, np.array([0], dtype=np.int32))
    rc, s2, o2, _ = inst.two_opt(succ[0], obj[0], mode=eng.FIRST)
    inst.close()
    s, o, st = _full_and_incremental(eng, ctx, xy, wt, s2)
    assert st["moves"] > 0 and o < o2 and o == O.succ_cost(xy, wt, s, 1)
    assert st["deltas_executed"] / st["evals"] <= 0.05, st


def test_batch_equals_single_calls(eng, ctx):
    n = 300
    xy = rand_instance(n, seed=77)
    rng = np.random.default_rng(8)
    tours = np.stack([random_tour(n, rng) for _ in range(8)])
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    rc, sb, ob, stb = _oropt(inst, tours)
    assert rc == 0
    for b in range(8):
        r1, s1, o1, st1 = _oropt(inst, tours[b])
        assert r1 == 0 and (s1 == sb[b]).all() and o1 == ob[b]
        for k in COUNTERS + ("deltas_executed",):
            assert st1[k] == stb[b][k], (b, k)
    inst.close()


def test_max_moves_prefix(eng, ctx):
    xy, wt = load_instance("rand4000")
    succ = random_tour(len(xy), np.random.default_rng(30))
    inst = eng.Instance(ctx, xy, wt, 1)
    rc, s, o, st = _oropt(inst, succ, max_moves=30)
    inst.close()
    ref, c = R.or_opt_descent(xy, wt, succ, 1, max_moves=30)
    assert rc == 0 and st["moves"] == 30 and st["sweeps"] == 30
    _same(s, o, st, ref, c, xy, wt, 1)


def test_grid_sized_instance(eng, ctx):
    """n = 20 011 (beyond every LDS engine), from the committed first-improvement 2-opt optimum of greedy."""
    g = golden("oracle_vectors_grid.json")["rand20011_first"]
    xy = np.random.default_rng(20011).integers(0, 700_000, size=(20011, 2)).astype(np.float64)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    succ, obj, _ = inst.construct(eng.GREEDY, np.array([g["start"]], dtype=np.int32))
    rc, s2, o2, _ = inst.two_opt(succ[0], obj[0], mode=eng.FIRST)
    inst.close()
    assert rc == 0 and o2 == g["final"]["cost"] and O.fnv1a(s2) == g["final"]["hash"]
    s, o, st = _full_and_incremental(eng, ctx, xy, O.EUC_2D, s2)
    assert O.is_tour(s) and o == O.succ_cost(xy, O.EUC_2D, s, 1) and o < o2 and st["moves"] > 0
    assert R.is_or_opt_optimal(xy, O.EUC_2D, s, 1)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["pr299", "att532", "pr1002"])
def test_two_opt_or_opt_composite(eng, ctx, name, mode):
    xy, wt = load_instance(name)
    _, es, eo = O.greedy(xy, wt, 0, 1)
    inst = eng.Instance(ctx, xy, wt, 1)
    rc, s, o, st2, sto = _composite(inst, es, eo, mode=mode)
    inst.close()
    ref, ro, rounds = R.two_opt_or_opt(xy, wt, es, eo, mode=mode)
    assert rc == 0 and (s == ref).all() and o == ro and sto["rounds"] == rounds >= 1
    assert st2["moves"] > 0
    _, _, _, bst, _, _ = O.two_opt_best(xy, wt, s, o, 1)
    assert bst["moves"] == 0
    assert R.decide(O.dist_matrix(xy, wt, 1), s) is None


@pytest.mark.parametrize("name", ["gr431", "ali535"])
def test_geo_tolerance_tier(eng, ctx, name):
    xy, wt = load_instance(name)
    assert wt == O.GEO
    inst = eng.Instance(ctx, xy, wt, 1)
    succ, obj, _ = inst.construct(eng.GREEDY, np.array([0], dtype=np.int32))
    rc, s, o, st = _oropt(inst, succ[0], obj[0])
    assert rc == 0 and O.is_tour(s) and st["moves"] > 0
    rc0, s0, o0, st0 = _oropt(inst, s, max_moves=0)      # the device's recomputation of the final tour's cost
    inst.close()
    assert rc0 == 0 and (s0 == s).all() and o0 == o and st0["sweeps"] == 0
    assert R.is_or_opt_optimal(xy, wt, s, 1, rel_tol=1e-9, cost=o)


def test_error_paths(eng, ctx):
    xy = rand_instance(50, seed=3)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    bad = np.arange(50, dtype=np.int32)            # every node its own successor
    n = 50
    o = np.zeros(1)
    st = eng.OrOptStats()
    L = eng.lib()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))              # noqa: E731
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))           # noqa: E731
    assert L.tsp_dev_or_opt(inst._h, 1, ip(bad), 1, n, dp(o), -1, -1.0, C.byref(st)) == -4
    good = random_tour(n, np.random.default_rng(1))
    assert L.tsp_dev_two_opt_or_opt(inst._h, 7, 1, ip(good), 1, n, dp(o), -1.0, None, None) == -3
    assert L.tsp_dev_two_opt_or_opt(inst._h, 0, 1, ip(bad), 1, n, dp(o), -1.0, None, None) == -4
    assert L.tsp_dev_or_opt(inst._h, 0, ip(good), 1, n, dp(o), -1, -1.0, None) == -3
    assert L.tsp_dev_or_opt(inst._h, 2, ip(np.concatenate([good, good])), 1, n - 1, dp(np.zeros(2)), -1, -1.0, None) == -3
    inst.close()
    # n < 5: nothing to do
    xy4 = np.array([[0, 0], [10, 3], [4, 9], [7, 7]], dtype=np.float64)
    inst = eng.Instance(ctx, xy4, O.EUC_2D, 1)
    s4 = np.array([2, 3, 1, 0], dtype=np.int32)
    rc, s, o4, st4 = _oropt(inst, s4)
    inst.close()
    assert rc == 0 and (s == s4).all() and o4 == O.succ_cost(xy4, O.EUC_2D, s4, 1)
    assert st4["sweeps"] == st4["moves"] == st4["evals"] == 0
    # a time limit of 1 ms: status 2, a valid tour and its cost
    xy, wt = load_instance("rand10000")
    succ = random_tour(len(xy), np.random.default_rng(9))
    inst = eng.Instance(ctx, xy, wt, 1)
    rc, s, o, st = _oropt(inst, succ, time_limit=0.001)
    rc2, s2, o2, _, _ = _composite(inst, succ, 0.0, time_limit=0.001)
    inst.close()
    assert rc == 2 and O.is_tour(s) and o == O.succ_cost(xy, wt, s, 1)
    assert rc2 == 2 and O.is_tour(s2) and o2 == O.succ_cost(xy, wt, s2, 1)
