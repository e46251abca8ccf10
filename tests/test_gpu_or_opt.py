"""Or-opt on the device (tsp_dev_or_opt, tsp_dev_two_opt_or_opt) against the CPU reference of the definition in
include/tsp_hip.h (tests/or_opt_ref.py): tours bit for bit and every counter for the integer-valued metrics and --fcost,
the incremental path against a full sweep per decision, batches, move caps, a GRID-sized instance, GEO at the tolerance
tier, and the error paths.  Then every (WT, INT) instance of the kernels, the sizes where their index arithmetic changes
(one wave, 62-row groups, column chunks, shifts longer than a workgroup), GEO bit for bit on the device's own matrix,
coincident-node ties, batches of the composite and the strided C ABI."""
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
    if st2["moves"] > 0:   # (no move: both paths ran the one full decision)
        assert st2["deltas_executed"] < st1["deltas_executed"]
    else:
        assert st2["deltas_executed"] == st1["deltas_executed"]
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


# ---- every (WT, INT) instance of TSP_DISPATCH_METRIC, size edges, long shifts, GEO exact, ties, batches, strides ---------

def _ref(xy, wt, succ, ic, max_moves=-1, D=None):
    return R.or_opt_descent(xy, wt, succ, ic, max_moves=max_moves, D=D)


def _cost_ok_D(D, succ, obj, ic):
    ref = float(D[np.arange(len(succ)), succ].sum())
    return obj == ref if ic else abs(obj - ref) <= 1e-9 * abs(ref)


def _both_vs_ref(eng, ctx, xy, wt, succ, ic, max_moves=-1, D=None):
    """Full sweeps and the incremental path: identical to each other and to the reference (D: the device's own matrix)."""
    s, o, st = _full_and_incremental(eng, ctx, xy, wt, succ, ic, max_moves=max_moves)
    ref, c = _ref(xy, wt, succ, ic, max_moves, D)
    if D is None:
        _same(s, o, st, ref, c, xy, wt, ic)
    else:
        assert (s == ref).all(), "tour differs from the reference"
        assert _cost_ok_D(D, s, o, ic), o
        for k in COUNTERS:
            assert st[k] == c[k], (k, st[k], c[k])
    return st


def _geo(name, n=None):
    xy, wt = load_instance(name)
    assert wt == O.GEO
    return (xy if n is None else xy[:n]), wt


def _device_matrix(eng, ctx, xy, wt, ic):
    inst = eng.Instance(ctx, xy, wt, ic)
    D, _ = inst.dist_matrix()
    inst.close()
    return D


# api.hip picks the instance: all coordinates integers and the bounding-box diagonal below TSP_ICOORD_MAX_DIST (2^21 - 1)
# -> EUC_2D_ICOORD / ATT_ICOORD (integer costs only) and CEIL_2D_ICOORD (either cost mode); anything else -> the general
# instance of the metric with INT = the cost mode.  So:
#   "i1k"   integers in [0, 1000): span about 1 400 -> the *_ICOORD instances;
#   "i3m"   integers in [0, 3e6):  span about 4.2e6 > 2^21 -> the general instances with integer coordinates (INT = 1);
#   "float" uniform floats: not integers -> the general instances (either cost mode);
#   MAN_2D / MAX_2D have no ICOORD form: integer coordinates take the general instance in both cost modes, and keep
#   --fcost free of rounding-noise cycles (their distances stay exact integers);
#   GEO: the first 257 nodes of gr431, compared through the device's own matrix (cos / acos differ from glibc's in the ulp).
DISPATCH = [
    ("EUC_2D_ICOORD", O.EUC_2D, 1, "i1k"), ("EUC_2D", O.EUC_2D, 1, "i3m"), ("EUC_2D", O.EUC_2D, 0, "float"),
    ("CEIL_2D_ICOORD", O.CEIL_2D, 1, "i1k"), ("CEIL_2D", O.CEIL_2D, 1, "float"), ("CEIL_2D", O.CEIL_2D, 0, "i3m"),
    ("ATT_ICOORD", O.ATT, 1, "i1k"), ("ATT", O.ATT, 1, "i3m"), ("ATT", O.ATT, 0, "float"),
    ("MAN_2D", O.MAN_2D, 1, "i3m"), ("MAN_2D", O.MAN_2D, 0, "i1k"),
    ("MAX_2D", O.MAX_2D, 1, "float"), ("MAX_2D", O.MAX_2D, 0, "i1k"),
    ("GEO", O.GEO, 1, "geo"), ("GEO", O.GEO, 0, "geo"),
]


def _coords(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "i1k":
        return rng.integers(0, 1000, size=(n, 2)).astype(np.float64)
    if kind == "i3m":
        return rng.integers(0, 3_000_000, size=(n, 2)).astype(np.float64)
    if kind == "float":
        return rng.uniform(-5000, 5000, size=(n, 2))
    return _geo("gr431", n)[0]


@pytest.mark.parametrize("start", ["random", "greedy"])
@pytest.mark.parametrize("label,wt,ic,kind", DISPATCH, ids=["%s-int%d" % (d[0], d[2]) for d in DISPATCH])
def test_every_dispatch_instance(eng, ctx, label, wt, ic, kind, start):
    n = 257
    xy = _coords(kind, n, 257 + wt)
    if kind == "i1k" or kind == "i3m":
        span = np.hypot(*(xy.max(0) - xy.min(0)))
        assert (span < 2097151.0) == (kind == "i1k")
    succ = random_tour(n, np.random.default_rng(wt + 10 * ic)) if start == "random" else O.greedy(xy, wt, 0, ic)[1]
    D = _device_matrix(eng, ctx, xy, wt, ic) if wt == O.GEO else None
    st = _both_vs_ref(eng, ctx, xy, wt, succ, ic, D=D)
    # MAN_2D sees x only (dy = |y2 - y2|): greedy on a line is already Or-opt-optimal, one full decision finds no move
    assert st["moves"] > 0 or (wt == O.MAN_2D and start == "greedy")


@pytest.mark.parametrize("n", [5, 6, 7, 8, 61, 62, 63, 64, 65, 124, 125, 126, 127, 512, 513, 1024, 1025])
def test_size_edges(eng, ctx, n):
    """One wave covers every row (n < 62, lanes wrap modulo n), the 62-row groups and their halo, and the column chunks of
    scratch_alloc (CH = 512 up to n = 8192: Cc = 1 / 2 at 512 / 513, 2 / 3 at 1024 / 1025).  The whole descent up to
    n = 127; 120 decisions beyond, where the CPU reference costs seconds per decision."""
    xy = np.random.default_rng(n).integers(0, 1000, size=(n, 2)).astype(np.float64)
    succ = random_tour(n, np.random.default_rng(n + 1))
    cap = -1 if n < 500 else 120
    st = _both_vs_ref(eng, ctx, xy, O.EUC_2D, succ, 1, max_moves=cap)
    assert st["moves"] > 0 or n == 5
    if cap > 0:
        assert st["moves"] == cap


def _trajectory(D, succ, moves):
    """The reference's first `moves` decisions -> [(m1, m2)] as k_or_pick_apply splits each move."""
    n, out = len(succ), []
    for _ in range(moves):
        d = R.decide(D, succ)
        if d is None:
            break
        f, L, a, o = R.decode(d[1], n)
        out.append(R.shift_lengths(succ, f, L, a))
        succ = R.apply_move(succ, f, L, a, o)
    return out


def test_long_shifts_in_pick_apply(eng, ctx):
    """n = 2600 from a random tour: the prefix holds moves whose shorter arc exceeds kPickThreads = 1024 in both branches
    of k_or_pick_apply (s .. a back by L in ascending chunks, b .. p on by L in descending chunks)."""
    n, cap = 2600, 8
    xy = rand_instance(n, seed=n)
    succ = random_tour(n, np.random.default_rng(5))
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    tr = _trajectory(D, succ, cap)
    assert len(tr) == cap
    assert any(m1 <= m2 and m1 > 1024 for m1, m2 in tr), tr
    assert any(m1 > m2 and m2 > 1024 for m1, m2 in tr), tr
    _both_vs_ref(eng, ctx, xy, O.EUC_2D, succ, 1, max_moves=cap, D=D)


@pytest.mark.parametrize("n,seed", [(8192, 8192), (8193, 2)])
def test_chunk_width_edges_8192(eng, ctx, n, seed):
    """CH = max(512, ceil(n / 16)): 16 chunks of 512 at n = 8192; at 8193, CH = 513 (the only chunks wider than 512).  The
    first decisions against the blocked reference (no n x n matrix); the tours are chosen so that these include shifts
    longer than kPickThreads in both branches of k_or_pick_apply."""
    moves = 4
    xy = rand_instance(n, seed=n)
    succ = random_tour(n, np.random.default_rng(seed))
    ref, c, shifts = R.or_opt_prefix_blocked(xy, O.EUC_2D, succ, moves, 1)
    assert c["moves"] == moves
    assert any(m1 <= m2 and m1 > 1024 for m1, m2 in shifts), shifts
    assert any(m1 > m2 and m2 > 1024 for m1, m2 in shifts), shifts
    s, o, st = _full_and_incremental(eng, ctx, xy, O.EUC_2D, succ, 1, max_moves=moves)
    _same(s, o, st, ref, c, xy, O.EUC_2D, 1)


@pytest.mark.parametrize("ic", [1, 0])
@pytest.mark.parametrize("name", ["burma14", "ulysses22", "gr431", "ali535"])
def test_geo_exact_on_device_matrix(eng, ctx, name, ic):
    """GEO bit for bit: the reference's descent on the device's own distance matrix.  With --fcost the descents are capped:
    ali535 holds 29 duplicate nodes, and from greedy the definition's own descent cycles on a delta of -1.8e-15 after
    99 moves; the device must follow that cycle move for move."""
    xy, wt = _geo(name)
    cap = -1 if ic else 300
    D = _device_matrix(eng, ctx, xy, wt, ic)
    assert (D == D.T).all(), "device GEO distance depends on the argument order"
    assert np.abs(D - O.dist_matrix(xy, wt, ic)).max() <= 1.0
    _, es, _ = O.greedy(xy, wt, 0, ic)
    for succ in (es, random_tour(len(xy), np.random.default_rng(len(xy)))):
        st = _both_vs_ref(eng, ctx, xy, wt, succ, ic, max_moves=cap, D=D)
        assert st["moves"] > 0


@pytest.mark.parametrize("wt", [O.MAN_2D, O.MAX_2D])
def test_man_max_coincident_ties(eng, ctx, wt):
    """dy = |y2 - y2| makes every node with the same x coincide: 300 nodes on 40 x values, so the node-id key decides
    most decisions, while the incremental path's row cache keeps bests among equal deltas."""
    rng = np.random.default_rng(600 + wt)
    xy = np.stack([rng.integers(0, 40, 300), rng.integers(0, 1_000_000, 300)], axis=1).astype(np.float64)
    succ = random_tour(300, rng)
    st = _both_vs_ref(eng, ctx, xy, wt, succ, 1)
    assert st["moves"] > 100


@pytest.mark.parametrize("mode", [0, 1])
def test_composite_batch_equals_single_calls(eng, ctx, mode):
    n, B = 200, 4
    xy = rand_instance(n, seed=4200 + mode)
    rng = np.random.default_rng(mode)
    tours = np.stack([random_tour(n, rng) for _ in range(B)])
    costs = np.array([O.succ_cost(xy, O.EUC_2D, t, 1) for t in tours])
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    rc, sb, ob, s2b, sob = _composite(inst, tours, costs, mode=mode)
    assert rc == 0
    for b in range(B):
        r1, s1, o1, s21, so1 = _composite(inst, tours[b], costs[b], mode=mode)
        assert r1 == 0 and (s1 == sb[b]).all() and o1 == ob[b]
        for k in COUNTERS + ("rounds", "deltas_executed"):
            assert so1[k] == sob[b][k], (b, k)
        for k in ("sweeps", "evals", "moves"):
            assert s21[k] == s2b[b][k], (b, k)
        ref, ro, rounds = R.two_opt_or_opt(xy, O.EUC_2D, tours[b], costs[b], mode=mode)
        assert (sb[b] == ref).all() and ob[b] == ro and sob[b]["rounds"] == rounds
    inst.close()


def test_composite_time_limit_in_batch(eng, ctx):
    """The budget runs out in tour 0 of three: tours 1 and 2 come back as they went in, with their costs and zeroed stats."""
    xy, wt = load_instance("rand10000")
    n = len(xy)
    rng = np.random.default_rng(33)
    tours = np.stack([random_tour(n, rng) for _ in range(3)])
    inst = eng.Instance(ctx, xy, wt, 1)
    rc, s, o, s2, so = _composite(inst, tours, np.zeros(3), time_limit=0.001)
    inst.close()
    assert rc == 2
    for b in range(3):
        assert O.is_tour(s[b]) and o[b] == O.succ_cost(xy, wt, s[b], 1)
    for b in (1, 2):
        assert (s[b] == tours[b]).all()
        assert all(v == 0 for v in s2[b].values()), s2[b]
        assert so[b]["moves_by_len"] == [0, 0, 0] and all(v == 0 for k, v in so[b].items() if k != "moves_by_len"), so[b]


def _strided(tours, stride, pad, fill):
    B, n = tours.shape
    ts = stride * n + pad
    buf = np.full(B * ts, fill, dtype=np.int32)
    for b in range(B):
        buf[b * ts: b * ts + stride * n: stride] = tours[b]
    return buf, ts


def test_strided_c_abi(eng, ctx):
    """tsp_dev_or_opt and tsp_dev_two_opt_or_opt with B = 3, succ_stride = 2, tour_stride = 2n + 3: the same results as the
    contiguous calls, the interleaved words and the padding untouched."""
    n, B = 150, 3
    xy = rand_instance(n, seed=150)
    rng = np.random.default_rng(150)
    tours = np.stack([random_tour(n, rng) for _ in range(B)])
    costs = np.array([O.succ_cost(xy, O.EUC_2D, t, 1) for t in tours])
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    L = eng.lib()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))              # noqa: E731
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))           # noqa: E731
    fill = -7
    rc, sc, oc, stc = _oropt(inst, tours)
    assert rc == 0
    buf, ts = _strided(tours, 2, 3, fill)
    o = costs.copy()
    st = (eng.OrOptStats * B)()
    assert L.tsp_dev_or_opt(inst._h, B, ip(buf), 2, ts, dp(o), -1, 120.0, st) == 0
    keep = np.ones(len(buf), dtype=bool)
    for b in range(B):
        keep[b * ts: b * ts + 2 * n: 2] = False
        assert (buf[b * ts: b * ts + 2 * n: 2] == sc[b]).all() and o[b] == oc[b]
        d = st[b].as_dict()
        for k in COUNTERS + ("deltas_executed",):
            assert d[k] == stc[b][k], (b, k)
    assert (buf[keep] == fill).all()
    rc, sc2, oc2, _, soc2 = _composite(inst, tours, costs)
    assert rc == 0
    buf, ts = _strided(tours, 2, 3, fill)
    o = costs.copy()
    so = (eng.OrOptStats * B)()
    assert L.tsp_dev_two_opt_or_opt(inst._h, eng.FIRST, B, ip(buf), 2, ts, dp(o), 120.0, None, so) == 0
    inst.close()
    for b in range(B):
        assert (buf[b * ts: b * ts + 2 * n: 2] == sc2[b]).all() and o[b] == oc2[b]
        assert so[b].rounds == soc2[b]["rounds"] and so[b].moves == soc2[b]["moves"]
    assert (buf[keep] == fill).all()
