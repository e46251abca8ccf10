"""GPU: k_exh's integer roots from an fp32 seed (csrc/exh_arith.hpp, the seed form) where an fp32 ulp is largest: full exhaustive
descents on instances in a thin box -- dx up to 2 090 000, dy a few thousand, the diagonal under the 2 097 151 the
integer-coordinate metrics admit -- whose distances from node 0 sit on or next to the rounding boundaries of the metric at roots
from 1 500 000 to 2 090 000 (the fp32 ulp is 0.125 there; tests/test_gpu_exh_arith.py stops at 1 440 000).  ATT's root is
sqrt(s / 10), so the diagonal bounds it at 663 000: its boundary points take the largest roots that admits, and its box is not
thin.  Tour, cost, sweeps, evals and moves must equal the oracle's."""
import numpy as np
import pytest

from oracle import oracle as O
from helpers import random_tour

pytestmark = pytest.mark.gpu
COUNTERS = ("sweeps", "evals", "moves")
DIAG_MAX = 2_097_151


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


def _descent(eng, ctx, monkeypatch, xy, wt, succ0):
    monkeypatch.setenv("TSP_NO_FILTER", "1")
    inst = eng.Instance(ctx, xy, wt, 1)
    t = eng.Tours(inst, 1)
    assert "k_exh" in t.describe(eng.BEST), t.describe(eng.BEST)
    t.upload(succ0, 0.0)
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID)
    s, o, st = t.download()
    t.close()
    inst.close()
    assert rc == 0 and done
    return s[0], o[0], {k: st[0][k] for k in COUNTERS}


def _boundary_points(wt, rng, count):
    """Integer (dx, dy), dx large and dy small, whose squared length s sits on or next to a rounding boundary of the metric:
    EUC_2D   (t^2, t): s = k^2 + k with k = t^2 (rounds down);  (t^2 - 1, t): s = k^2 + k + 1 (rounds up);  (k, 0): s = k^2
    CEIL_2D  (k, 0): s = k^2;  (k, 1): s = k^2 + 1;  (2 t^2, 2 t): s = k^2 - 1 with k = 2 t^2 + 1
    ATT      (3 k, k): s = 10 k^2;  (3 k, k + 1) and (3 k, k - 1): the nearest lattice points above and below it
    with k in [1 500 000, 2 090 000] (ATT: [560 000, 660 000], see the module's docstring)."""
    out = []
    while len(out) < count:
        if wt == O.EUC_2D:
            k, t = int(rng.integers(1_500_000, 2_090_001)), int(rng.integers(1225, 1446))      # t^2 in [1 500 625, 2 088 025]
            new = [(t * t, t), (t * t - 1, t), (k, 0)]
        elif wt == O.CEIL_2D:
            k, t = int(rng.integers(1_500_000, 2_090_001)), int(rng.integers(867, 1023))       # 2 t^2 in [1 503 378, 2 089 968]
            new = [(k, 0), (k, 1), (2 * t * t, 2 * t)]
        else:
            k = int(rng.integers(560_000, 660_001))
            new = [(3 * k, k), (3 * k, k + 1), (3 * k, k - 1)]
        out += new
    return out[:count]


def _instance(wt, rng, n):
    pts = _boundary_points(wt, rng, n - 1)
    if wt != O.ATT:
        pts[0] = (2_090_000, 0)                       # the box's full length, whatever the draws
    xy = np.array([[0, 0]] + [[dx, dy] for dx, dy in pts], dtype=np.float64)
    span = xy.max(axis=0) - xy.min(axis=0)
    assert float(np.hypot(*span)) < DIAG_MAX
    if wt != O.ATT:
        assert span[0] > 2_080_000 and span[1] < 3000                  # the thin box
    on = 0                                            # the construction does what it says: distances from node 0
    for dx, dy in pts[:60]:
        s = dx * dx + dy * dy
        k = int(np.floor(np.sqrt(float(s if wt != O.ATT else s // 10))))
        on += any(s - b in (-1, 0, 1) for kk in (k - 1, k, k + 1)
                  for b in ((kk * kk + kk, kk * kk) if wt == O.EUC_2D else ((kk * kk,) if wt == O.CEIL_2D else (10 * kk * kk,))))
    assert on >= 20, on
    return xy


def _check(eng, ctx, monkeypatch, xy, wt, rng):
    succ0 = random_tour(len(xy), rng)
    s, o, st = _descent(eng, ctx, monkeypatch, xy, wt, succ0)
    _, es, eo, est, _, _ = O.two_opt_best(xy, wt, succ0)
    assert (s == es).all() and o == eo and st == {k: est[k] for k in COUNTERS}, (o, eo, st, est)


@pytest.mark.parametrize("wt", [O.EUC_2D, O.CEIL_2D, O.ATT])
def test_boundary_distances_where_an_fp32_ulp_is_largest(eng, ctx, monkeypatch, wt):
    rng = np.random.default_rng(21 + wt)
    xy = _instance(wt, rng, 301)
    assert len(np.unique(xy, axis=0)) > 200            # (t has some 200 values: a few points coincide, which is s = 0 once more)
    _check(eng, ctx, monkeypatch, xy, wt, rng)


def test_two_nodes_on_one_point(eng, ctx, monkeypatch):
    """s = 0: the fp32 root of 0 is 0, k = 0 and the residual 0 -- the distance 0 for both roundings."""
    rng = np.random.default_rng(77)
    for wt in (O.EUC_2D, O.CEIL_2D):
        xy = _instance(wt, rng, 300)
        xy[17] = xy[211]
        xy[5] = xy[0]
        _check(eng, ctx, monkeypatch, xy, wt, rng)


def test_predicated_rows_where_strip_0_overlaps_strip_1(eng, ctx, monkeypatch):
    """n = 257: two strips of 255 pair-columns with a slack of 253, so strip 0 is clamped onto strip 1 and every one of its rows
    crosses the diagonal -- the predicated row steps take the seed form too."""
    rng = np.random.default_rng(257)
    xy = _instance(O.EUC_2D, rng, 257)
    _check(eng, ctx, monkeypatch, xy, O.EUC_2D, rng)
