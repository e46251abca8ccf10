"""GPU: the exhaustive sweep's arithmetic (csrc/exh_arith.hpp in k_move_pos + k_exh) where it could go wrong on the device:
positions stored relative to node 0 (instances of almost the widest admissible span, shifted by a few 1e15), squared
distances on the rounding boundaries of the three metrics at large roots, and right-aligned strips with the smallest and
the largest slack."""
import numpy as np
import pytest

from oracle import oracle as O
from helpers import rand_instance, random_tour

pytestmark = pytest.mark.gpu
COUNTERS = ("sweeps", "evals", "moves", "reversed")


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


def _descent(eng, ctx, monkeypatch, xy, wt, succ0, env=None, expect_exh=True):
    monkeypatch.setenv("TSP_NO_FILTER", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    inst = eng.Instance(ctx, xy, wt, 1)
    t = eng.Tours(inst, 1)
    assert ("k_exh" in t.describe(eng.BEST)) == expect_exh, t.describe(eng.BEST)
    t.upload(succ0, 0.0)
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID)
    s, o, st = t.download()
    t.close()
    inst.close()
    for k in (env or {}):
        monkeypatch.delenv(k)
    assert rc == 0 and done
    return s[0], o[0], {k: st[0][k] for k in COUNTERS}


@pytest.mark.parametrize("wt", [O.EUC_2D, O.CEIL_2D, O.ATT])
def test_widest_span_with_huge_absolute_coordinates(eng, ctx, monkeypatch, wt):
    """Diagonal 2 093 036 (the bound is 2 097 151), x shifted by +3e15 and y by -2.5e15: the relative positions k_move_pos
    stores are the same integers as without the shift, so tour, cost and counters must be too -- and the oracle's."""
    n, side = 320, 1_480_000
    rng = np.random.default_rng(41)
    xy = rng.integers(0, side + 1, size=(n, 2)).astype(np.float64)
    xy[7] = (0, 0)
    xy[11] = (side, side)
    xy[13] = (0, side)
    off = xy + np.array([3.0e15, -2.5e15])
    assert ((off - np.array([3.0e15, -2.5e15])) == xy).all()          # representable: nothing rounded by the shift
    succ0 = random_tour(n, rng)
    s0, o0, st0 = _descent(eng, ctx, monkeypatch, xy, wt, succ0)
    s1, o1, st1 = _descent(eng, ctx, monkeypatch, off, wt, succ0)
    _, es, eo, est, _, _ = O.two_opt_best(xy, wt, succ0)
    est = {k: est[k] for k in COUNTERS}
    assert (s0 == es).all() and o0 == eo and st0 == est
    assert (s1 == es).all() and o1 == eo and st1 == est
    _, fs, fo, fst, _, _ = O.two_opt_best(off, wt, succ0)
    assert (fs == es).all() and fo == eo                               # the oracle itself does not mind the shift


def _boundary_points(wt, rng, count):
    """Integer (dx, dy) whose squared length s sits on or next to a rounding boundary of the metric at a large root k:
    EUC_2D   (t^2, t): s = k^2 + k with k = t^2 (rounds down);  (t^2 - 1, t): s = k^2 + k + 1 (rounds up);  (k, 0): s = k^2
    CEIL_2D  (k, 0): s = k^2;  (k, 1): s = k^2 + 1;  (2 t^2, 2 t): s = k^2 - 1 with k = 2 t^2 + 1
    ATT      (3 k, k): s = 10 k^2;  (3 k, k + 1) and (3 k, k - 1): the nearest lattice points above and below it"""
    out = []
    while len(out) < count:
        t, flip = int(rng.integers(300, 1200)), bool(rng.integers(0, 2))
        if wt == O.EUC_2D:
            k = int(rng.integers(700_000, 1_440_000))
            new = [(t * t, t), (t * t - 1, t), (k, 0)]
        elif wt == O.CEIL_2D:
            k, t = int(rng.integers(700_000, 1_440_000)), int(rng.integers(300, 845))
            new = [(k, 0), (k, 1), (2 * t * t, 2 * t)]
        else:
            k = int(rng.integers(100_000, 480_000))
            new = [(3 * k, k), (3 * k, k + 1), (3 * k, k - 1)]
        out += [(dy, dx) if flip else (dx, dy) for dx, dy in new]
    return out[:count]


@pytest.mark.parametrize("wt", [O.EUC_2D, O.CEIL_2D, O.ATT])
def test_boundary_distances_at_large_roots_equal_the_tiled_path(eng, ctx, monkeypatch, wt):
    """Node 0 at the origin, every other node at a squared distance from it that sits on or next to a rounding boundary, roots
    from 9e4 to 1.44e6 (the instance's diagonal 2.04e6 bounds every root): the descent of k_exh (floor / rint of the raw root,
    residual test) must equal that of the tiled k_step under TSP_EXH_POS=0, which keeps tsp_dist.hpp's int_root -- and the
    oracle's."""
    rng = np.random.default_rng(8)
    pts = _boundary_points(wt, rng, 330)
    xy = np.array([[0, 0]] + [[dx, dy] for dx, dy in pts], dtype=np.float64)
    assert xy.max() <= 1_445_000 and len(np.unique(xy, axis=0)) > 300
    on = 0                                            # the construction does what it says: distances from node 0
    for dx, dy in pts[:60]:
        s = dx * dx + dy * dy
        k = int(np.floor(np.sqrt(float(s if wt != O.ATT else s // 10))))
        on += any(s - b in (-1, 0, 1) for kk in (k - 1, k, k + 1)
                  for b in ((kk * kk + kk, kk * kk) if wt == O.EUC_2D else ((kk * kk,) if wt == O.CEIL_2D else (10 * kk * kk,))))
    assert on >= 20, on
    succ0 = random_tour(len(xy), rng)
    s, o, st = _descent(eng, ctx, monkeypatch, xy, wt, succ0)
    s_old, o_old, st_old = _descent(eng, ctx, monkeypatch, xy, wt, succ0, {"TSP_EXH_POS": "0"}, expect_exh=False)
    assert (s == s_old).all() and o == o_old and st == st_old
    _, es, eo, est, _, _ = O.two_opt_best(xy, wt, succ0)
    assert (s == es).all() and o == eo and st == {k: est[k] for k in COUNTERS}


@pytest.mark.parametrize("n", [509, 764, 256, 511])
def test_right_aligned_strips_with_the_smallest_and_the_largest_slack(eng, ctx, monkeypatch, n):
    """Strips are 255 pair-columns wide and laid out from the right end; strips * 255 - n is 1 at n = 509 and 764 (strip 0 lacks
    one column) and 254 at n = 256 and 511 (strip 0 is one column wide and has no row at all)."""
    assert (-n) % 255 in (1, 254)
    xy = rand_instance(n, seed=500 + n, hi=900_000)
    rng = np.random.default_rng(n)
    for wt in (O.EUC_2D, O.ATT):
        succ0 = random_tour(n, rng)
        s, o, st = _descent(eng, ctx, monkeypatch, xy, wt, succ0)
        _, es, eo, est, _, _ = O.two_opt_best(xy, wt, succ0)
        assert (s == es).all() and o == eo and st == {k: est[k] for k in COUNTERS}, (n, wt)
