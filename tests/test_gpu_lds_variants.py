"""The LDS engine's kernel bodies k_lds_two_opt<WT, INT, MODE, CACHE, F32> for the three integer-coordinate metrics, held to the
oracle's trajectory: the fp32 first tier of the new-edge bound (F32) and the edge-length cache (CACHE) on and off, both rules.  The
fp32 tier is a pruning bound: were it wrong by a unit, an improving pair would be skipped and the descent would take another valid
trajectory, which only equality with the oracle notices.  So every comparison here is exact -- tour, cost, sweeps, evaluations,
moves and reversal length against oracle.two_opt_first / two_opt_best -- and every case first asserts through
Instance.lds_variant that the body it names is the one the library selects.  The switches are set before the Instance is created
(they are read once per handle)."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from helpers import rand_instance, random_tour

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = {"EUC_2D": O.EUC_2D, "ATT": O.ATT, "CEIL_2D": O.CEIL_2D}
FIRST, BEST = 0, 1
RULE = {FIRST: "FIRST", BEST: "BEST"}
COUNTERS = ("sweeps", "evals", "moves", "reversed")
SIZES = [5, 6, 7, 8, 33, 257, 513, 514, 515, 516, 1023, 1024, 1025]
# TSP_ICOORD_MAX_DIST = 2 097 151: the largest integer c with c sqrt(2) below it (2 c^2 < 2 097 151^2 < 2 (c + 1)^2)
SPAN_C = 1482909
assert 2 * SPAN_C ** 2 < 2097151 ** 2 < 2 * (SPAN_C + 1) ** 2


@pytest.fixture(scope="module")
def eng():
    from tsp_optimization_amd import engine as E
    assert E.device_count() >= 1, "no HIP device visible: the product path has no CPU fallback"
    assert (E.FIRST, E.BEST) == (FIRST, BEST)
    return E


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.Context(0)
    yield c
    c.close()


# ---- the reference: computed once per (instance, start, rule), shared by every case that runs it, never changed -----------------------

_REF = {}


def oracle_descent(xy, wt, succ, rule):
    """-> (tour, cost, (sweeps, evals, moves, reversed)) of the oracle's descent from `succ`"""
    key = hashlib.sha1(xy.tobytes() + np.asarray(succ, dtype=np.int32).tobytes() + bytes([wt, rule])).digest()
    if key not in _REF:
        if rule == FIRST:
            _, s, o, st, _ = O.two_opt_first(xy, wt, succ, O.succ_cost(xy, wt, succ))
        else:
            _, s, o, st, _, _ = O.two_opt_best(xy, wt, succ)
        s.setflags(write=False)
        _REF[key] = (s, o, tuple(st[k] for k in COUNTERS))
    return _REF[key]


def variant_line(metric, rule, cache, f32, icoord=True):
    return "k_lds_two_opt<%s%s, %s, cache=%d, f32=%d> " % (metric, "_ICOORD" if icoord else "", RULE[rule], cache, f32)


def check(eng, inst, xy, metric, succs, rule, cache, f32, icoord=True):
    """the body named is the one selected; then the LDS engine's descent from each start equals the oracle's, counters included.
    -> the device's (tours, costs, counters) for comparisons between runs"""
    wt = METRICS[metric]
    line = inst.lds_variant(rule)
    print(line)
    assert line.startswith(variant_line(metric, rule, cache, f32, icoord)), line
    succs = np.atleast_2d(np.asarray(succs, dtype=np.int32))
    obj = np.array([O.succ_cost(xy, wt, s) for s in succs])
    rc, got, cost, st = inst.two_opt(succs, obj, mode=rule, engine=eng.ENGINE_LDS)
    assert rc == 0
    counters = []
    for k, start in enumerate(succs):
        es, eo, ec = oracle_descent(xy, wt, start, rule)
        gc = tuple(st[k][c] for c in COUNTERS)
        assert cost[k] == eo and gc == ec and (got[k] == es).all(), (line, k, cost[k], eo, gc, ec)
        counters.append(gc)
    return got, cost, counters


def points(n, hi=100_000, seed=None):
    return np.random.default_rng(n if seed is None else seed).integers(0, hi, size=(n, 2)).astype(np.float64)


def greedy_tour(xy, metric):
    return O.greedy(xy, METRICS[metric])[1]


def reversals(succ, count, seed):
    """`succ` with `count` seeded random segments of its node sequence reversed: a few long edges in an otherwise good tour"""
    rng = np.random.default_rng(seed)
    perm = O.succ_to_perm(succ)
    n = len(perm)
    for _ in range(count):
        a, b = sorted(int(x) for x in rng.integers(0, n, 2))
        perm[a:b + 1] = perm[a:b + 1][::-1].copy()
    return O.perm_to_succ(perm)


def set_switches(monkeypatch, f32=None, cache=None, **more):
    for k in ("TSP_LDS_F32_MIN_N", "TSP_LDS_EDGE_CACHE", "TSP_LDS_MIN_ROWS", "TSP_LDS_PROBE", "TSP_NO_PRUNE", "TSP_NO_FILTER", "TSP_NO_ICOORD",
              "TSP_ENGINE"):
        monkeypatch.delenv(k, raising=False)
    if f32 is not None:
        monkeypatch.setenv("TSP_LDS_F32_MIN_N", "0" if f32 else str(1 << 30))
    if cache is not None:
        monkeypatch.setenv("TSP_LDS_EDGE_CACHE", str(cache))
    for k, v in more.items():
        monkeypatch.setenv(k, str(v))


def both_rules(eng, ctx, xy, metric, cache, f32, first_start, best_start, icoord=True):
    inst = eng.Instance(ctx, xy, METRICS[metric], 1)
    try:
        a = check(eng, inst, xy, metric, first_start, FIRST, cache, f32, icoord)
        b = check(eng, inst, xy, metric, best_start, BEST, cache, f32, icoord)
    finally:
        inst.close()
    return a, b


# ---- (a) the whole matrix at small n ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cache", [1, 0])
@pytest.mark.parametrize("metric", list(METRICS))
def test_fp32_tier_on_every_body_at_small_sizes(eng, ctx, monkeypatch, metric, cache, n):
    """every residue of n mod 4 (the padding), row blocks of 1 to 32 rows with tails that are no multiple of the trip's four rows,
    one, two and more column batches, the vote on / off boundary at n - jbase > 1 024.  FIRST from a random tour at every size;
    BEST from a random tour up to 300 nodes and from the greedy tour above (the oracle's BEST is O(n^3) from a random tour)."""
    set_switches(monkeypatch, f32=1, cache=cache)
    xy = points(n)
    rnd = random_tour(n, np.random.default_rng(n + 1))
    both_rules(eng, ctx, xy, metric, cache, 1, rnd, rnd if n <= 300 else greedy_tour(xy, metric))


@pytest.mark.parametrize("n", [7, 515, 1025])
@pytest.mark.parametrize("cache", [1, 0])
@pytest.mark.parametrize("metric", list(METRICS))
def test_fp32_tier_off_with_and_without_the_cache(eng, ctx, monkeypatch, metric, cache, n):
    """the same cases on the bodies without the fp32 tier: with the cache what every small instance gets by default, without it
    what nothing ran before"""
    set_switches(monkeypatch, f32=0, cache=cache)
    xy = points(n)
    rnd = random_tour(n, np.random.default_rng(n + 1))
    both_rules(eng, ctx, xy, metric, cache, 0, rnd, rnd if n <= 300 else greedy_tour(xy, metric))


@pytest.mark.parametrize("cache", [1, 0])
@pytest.mark.parametrize("metric", list(METRICS))
def test_three_different_tours_in_one_call(eng, ctx, monkeypatch, metric, cache):
    set_switches(monkeypatch, f32=1, cache=cache)
    n = 257
    xy = points(n)
    starts = np.stack([random_tour(n, np.random.default_rng(n + 1 + k)) for k in range(3)])
    (_, cost, _), _ = both_rules(eng, ctx, xy, metric, cache, 1, starts, starts)
    assert len(set(cost.tolist())) > 1          # three descents of their own, not one three times


# ---- (b) geometry the slack is sized for ---------------------------------------------------------------------------------------------

def span_limit_points(n, c):
    xy = np.random.default_rng(n).integers(0, c + 1, size=(n, 2)).astype(np.float64)
    xy[0] = (0, 0)
    xy[1] = (c, c)
    return xy


def geometry_case(eng, ctx, monkeypatch, xy, metric, icoord=True):
    """F32 forced on, both rules: FIRST from a random tour (long edges: T near its largest), BEST from the greedy tour with eight
    segments reversed (a few very long edges among short ones: the bound falls far below zero after the first rows)"""
    set_switches(monkeypatch, f32=1)
    n = len(xy)
    rnd = random_tour(n, np.random.default_rng(n + 1))
    mixed = reversals(greedy_tour(xy, metric), 8, n)
    on = 1 if icoord else 0
    return both_rules(eng, ctx, xy, metric, on, on, rnd, mixed, icoord)


@pytest.mark.parametrize("metric", list(METRICS))
def test_coordinates_at_the_span_limit(eng, ctx, monkeypatch, metric):
    """uniform integer points in [0, c]^2 with (0, 0) and (c, c) among them, c sqrt(2) = 2 097 150.02: the largest distances, squares
    and T the fp32 tier is sized for"""
    geometry_case(eng, ctx, monkeypatch, span_limit_points(600, SPAN_C), metric)


@pytest.mark.parametrize("metric", list(METRICS))
def test_one_unit_beyond_the_span_limit_takes_the_general_body(eng, ctx, monkeypatch, metric):
    geometry_case(eng, ctx, monkeypatch, span_limit_points(600, SPAN_C + 1), metric, icoord=False)


def test_translation_changes_nothing(eng, ctx, monkeypatch):
    """the span-limit instance moved by (+2^40, -2^40): the floats are taken relative to the instance corner"""
    xy = span_limit_points(600, SPAN_C)
    moved = xy + np.array([2.0 ** 40, -2.0 ** 40])
    assert ((moved - np.array([2.0 ** 40, -2.0 ** 40])) == xy).all()
    a = geometry_case(eng, ctx, monkeypatch, xy, "EUC_2D")
    b = geometry_case(eng, ctx, monkeypatch, moved, "EUC_2D")
    for (s0, c0, k0), (s1, c1, k1) in zip(a, b):
        assert (s0 == s1).all() and (c0 == c1).all() and k0 == k1


@pytest.mark.parametrize("scale", [1, 4099])
@pytest.mark.parametrize("metric", list(METRICS))
def test_lattice_with_repeated_points(eng, ctx, monkeypatch, metric, scale):
    """a 20 x 20 lattice, every point once and 200 of them twice: new edges exactly as long as the bound allows, and edges of
    length zero; with the pitch 4 099 the tied lengths lie above 2^12, where their squares no longer fit a float"""
    rng = np.random.default_rng(20)
    cells = np.concatenate([np.arange(400), rng.integers(0, 400, 200)])
    rng.shuffle(cells)
    xy = np.stack([cells % 20, cells // 20], axis=1).astype(np.float64) * scale
    geometry_case(eng, ctx, monkeypatch, xy, metric)


@pytest.mark.parametrize("metric", list(METRICS))
def test_four_tight_clusters_at_the_corners_of_the_span_limit_box(eng, ctx, monkeypatch, metric):
    """removed edges of length 0 to 3 next to edges of 2 10^6: a BEST bound of -10^6 and less makes T negative"""
    n = 600
    rng = np.random.default_rng(n)
    corner = rng.integers(0, 4, n)
    off = rng.integers(0, 3, size=(n, 2)).astype(np.float64)
    xy = np.where(np.stack([corner % 2, corner // 2], axis=1) == 1, SPAN_C - off, off)
    xy[0] = (0, 0)
    xy[1] = (SPAN_C, SPAN_C)
    geometry_case(eng, ctx, monkeypatch, xy, metric)


@pytest.mark.parametrize("line", ["x", "y", "diagonal", "antidiagonal"])
@pytest.mark.parametrize("metric", list(METRICS))
def test_collinear_points(eng, ctx, monkeypatch, metric, line):
    n = 600
    rng = np.random.default_rng(n)
    if line in ("x", "y"):
        t = rng.integers(0, 2097151, n).astype(np.float64)           # span 2 097 150 at the most
        t[0], t[1] = 0, 2097150
        xy = np.stack([t, np.full(n, 7.0)] if line == "x" else [np.full(n, 7.0), t], axis=1)
    else:
        t = rng.integers(0, SPAN_C + 1, n).astype(np.float64)
        t[0], t[1] = 0, SPAN_C
        xy = np.stack([t, t if line == "diagonal" else SPAN_C - t], axis=1)
    geometry_case(eng, ctx, monkeypatch, xy, metric)


def planted_tie(n=2200, d=6000, h=500):
    """-> (xy, tour): a tour along a circle that zigzags A2, B2, A1, B1, A2, B2, x, A1, B1 between four sites at its start: A1
    and B1 d apart, A2 and B2 h above them.  Joining the two visits of A2 -- the pair (3, 2148) -- gains 2 d with two new edges of
    length zero, and so does joining the two visits of A1, the pair (5, 100); nothing else in the tour gains as much, and
    whichever of the two is carried out first undoes the other, so the descent depends on the choice.  One lane owns the columns
    100 and 2148; it meets (5, 100) first -- 2 048 columns go through the row block before the next 2 048 -- and then
    (3, 2148), which wins the tie by its smaller key, with bound + d(a, a1) + d(b, b1) = 0 exactly and a new edge of length zero:
    T is nothing but its margin."""
    A1, B1, A2, B2 = (900_000, 500_000), (900_000 + d, 500_000), (900_000, 500_000 + h), (900_000 + d, 500_000 + h)
    plants = {3: A2, 4: B2, 5: A1, 6: B1, 2148: A2, 2149: B2, 7: (900_000 + d // 2, 500_000 + h // 2), 100: A1, 101: B1}
    base = [v for v in range(n) if v not in plants]
    m = len(base)
    ang = 2 * np.pi * (np.arange(m) + 1.0) / (m + 1)
    xy = np.zeros((n, 2))
    xy[base] = np.rint(np.stack([500_000 + 400_000 * np.cos(ang), 500_000 + 400_000 * np.sin(ang)], axis=1))
    for v, site in plants.items():
        xy[v] = site
    seq = list(plants) + base
    succ = np.zeros(n, dtype=np.int32)
    succ[seq] = np.roll(seq, -1)
    return xy, succ


@pytest.mark.parametrize("metric", list(METRICS))
def test_best_keeps_a_tie_that_leaves_the_fp32_bound_nothing_but_its_margin(eng, ctx, monkeypatch, metric):
    """Beyond 2 048 nodes a lane of BEST no longer meets its pairs in key order, so a pair that only ties with the lane's best
    must pass every bound (the smaller key wins).  Here the tying pair has T = 0 + margin: with CEIL_2D and ATT the fp64 margin
    is 2 (1e-6 + span 2^-36), which the float sum loses, and only the two units of slack in the fp32 bound keep the pair."""
    set_switches(monkeypatch, f32=1)
    xy, succ = planted_tie()
    wt = METRICS[metric]
    dist = lambda a, b: O.dist(xy, a, b, wt)
    gain = 2 * dist(3, 4)
    assert (succ[3], succ[2148], succ[5], succ[100]) == (4, 2149, 6, 101)
    for a, b in ((3, 2148), (5, 100)):                      # the two pairs tie ...
        assert dist(a, succ[a]) + dist(b, succ[b]) - dist(a, b) - dist(succ[a], succ[b]) == gain and dist(a, b) == 0
    trace = O.two_opt_best(xy, wt, succ, trace_cap=2)[4]
    assert trace[0] == (3, 2148, -gain) and trace[1][:2] == (5, 100) and trace[1][2] > -gain, trace   # ... and the first undoes the second
    inst = eng.Instance(ctx, xy, wt, 1)
    try:
        check(eng, inst, xy, metric, succ, BEST, 1, 1)
    finally:
        inst.close()


# ---- (c) chunking and probe, (d) bounds off --------------------------------------------------------------------------------------------

def case_515(eng, ctx, cache=1):
    xy = points(515)
    rnd = random_tour(515, np.random.default_rng(516))
    return both_rules(eng, ctx, xy, "EUC_2D", cache, 1, rnd, greedy_tour(xy, "EUC_2D"))


@pytest.mark.parametrize("probe", [0, 1 << 30])
@pytest.mark.parametrize("min_rows", [1, 3, 7, 32])
def test_chunk_sizes_and_the_probe_change_nothing(eng, ctx, monkeypatch, min_rows, probe):
    set_switches(monkeypatch, f32=1, cache=1, TSP_LDS_MIN_ROWS=min_rows, TSP_LDS_PROBE=probe)
    case_515(eng, ctx)


@pytest.mark.parametrize("switch", ["TSP_NO_PRUNE", "TSP_NO_FILTER"])
def test_with_the_bounds_off_the_fp32_tier_passes_every_pair(eng, ctx, monkeypatch, switch):
    """the margin of the new-edge bound is then 1e300 and the fp32 bound infinite: the same descents"""
    set_switches(monkeypatch, f32=1, cache=1)
    on = case_515(eng, ctx)
    set_switches(monkeypatch, f32=1, cache=1, **{switch: 1})
    off = case_515(eng, ctx)
    for (s0, c0, k0), (s1, c1, k1) in zip(on, off):
        assert (s0 == s1).all() and (c0 == c1).all() and k0 == k1


# ---- (e) natural sizes, no switch set --------------------------------------------------------------------------------------------------

def natural(eng, ctx, monkeypatch, n, metric, cache, f32, best=0):
    """rand_instance(n), FIRST from the greedy tour; best = B > 0: then BEST on B copies of the tour FIRST returned (the oracle has
    just confirmed it), each with six seeded segment reversals of its own: a handful of sweeps"""
    set_switches(monkeypatch)
    xy = rand_instance(n)
    inst = eng.Instance(ctx, xy, METRICS[metric], 1)
    try:
        got, _, _ = check(eng, inst, xy, metric, greedy_tour(xy, metric), FIRST, cache, f32)
        if best:
            starts = np.stack([reversals(got[0], 6, n + k) for k in range(best)])
            assert len({s.tobytes() for s in starts}) == best
            _, _, counters = check(eng, inst, xy, metric, starts, BEST, cache, f32)
            assert all(c[2] > 0 for c in counters)          # every one of them had something to repair
    finally:
        inst.close()


@pytest.mark.parametrize("n,f32", [(2499, 0), (2500, 1)])
def test_the_fp32_tier_comes_on_at_2500_nodes(eng, ctx, monkeypatch, n, f32):
    natural(eng, ctx, monkeypatch, n, "EUC_2D", 1, f32)


def test_att_at_2501_nodes_first_then_best_on_two_tours(eng, ctx, monkeypatch):
    """n = 1 mod 4 with the cache and the fp32 tier: 12 bytes of padding behind pos[] and 12 more behind the edge lengths"""
    natural(eng, ctx, monkeypatch, 2501, "ATT", 1, 1, best=2)


def test_ceil_2d_at_2502_nodes(eng, ctx, monkeypatch):
    natural(eng, ctx, monkeypatch, 2502, "CEIL_2D", 1, 1)


@pytest.fixture(scope="module")
def cache_boundary(eng, ctx):
    """(the largest n that gets the cache, the largest n the engine takes), found through lds_variant alone; and the same two
    from csrc/lds_layout.hpp, built with the host compiler, for the LDS size the library reports"""
    def line(n):
        with pytest.MonkeyPatch.context() as mp:
            for k in ("TSP_LDS_F32_MIN_N", "TSP_LDS_EDGE_CACHE", "TSP_NO_ICOORD"):
                mp.delenv(k, raising=False)
            inst = eng.Instance(ctx, rand_instance(n), O.EUC_2D, 1)
        try:
            return inst.lds_variant(FIRST)
        except eng.TspDeviceError:
            return None
        finally:
            inst.close()

    def largest(pred, lo, hi):          # pred holds at lo and not at hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if pred(mid) else (lo, mid)
        return lo

    fits = largest(lambda n: line(n) is not None, 3, 65536)
    cached = largest(lambda n: "cache=1" in line(n), 3, fits + 1)
    lds = int(line(fits).rsplit(" of ", 1)[1])
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "lds_layout_check")
        subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "tsp_optimization_amd", "csrc"), "-o", exe,
                               os.path.join(ROOT, "tests", "lds_layout_check.cpp")])
        out = subprocess.run([exe, "max", str(lds)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    _, no_cache, with_cache = out.stdout.split()
    return cached, fits, int(with_cache), int(no_cache), lds


def test_the_boundaries_are_those_of_the_layout_header(cache_boundary):
    cached, fits, with_cache, no_cache, lds = cache_boundary
    assert (cached, fits) == (with_cache, no_cache)
    if lds == 160 * 1024:
        assert (cached, fits) == (6698, 8038)


@pytest.mark.parametrize("step", [0, 1])
def test_the_last_size_with_the_cache_and_the_first_without(eng, ctx, monkeypatch, cache_boundary, step):
    natural(eng, ctx, monkeypatch, cache_boundary[0] + step, "EUC_2D", 1 - step, 1)


def test_7001_nodes_fp32_tier_without_the_cache_first_then_best(eng, ctx, monkeypatch):
    natural(eng, ctx, monkeypatch, 7001, "EUC_2D", 0, 1, best=1)


def test_the_largest_size_that_fits_and_its_successor_refused(eng, ctx, monkeypatch, cache_boundary):
    fits = cache_boundary[1]
    natural(eng, ctx, monkeypatch, fits, "EUC_2D", 0, 1)
    xy = rand_instance(fits + 1)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    try:
        with pytest.raises(eng.TspDeviceError):
            inst.lds_variant(FIRST)
        succ = greedy_tour(xy, "EUC_2D")
        with pytest.raises(eng.TspDeviceError):
            inst.two_opt(succ, O.succ_cost(xy, O.EUC_2D, succ), mode=FIRST, engine=eng.ENGINE_LDS)
    finally:
        inst.close()
