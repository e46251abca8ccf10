"""GPU: k_exh walks a wave's rows in batches of kRowBatch = 4 (csrc/two_opt_exh.hpp): the rows up to the strip's first column
as whole batches without a predicate, the rest row by row; the wave-uniform bound only filters which pairs reach the exact
bookkeeping.  Whatever the kernel does with a batch -- it was written once with one test of the bound per batch instead of one
per row, measured, and not kept; these are the cases that form had to pass and any later one has to -- every
decision must stay the reference's: whole descents against the oracle (tour, cost, sweeps, evaluations, moves, reversal length)
where a wave's range starts and ends at every row residue mod 4, where several rows of one batch reach the bound (the first
sweep from a random tour: the bound starts at -1), and where pairs in adjacent rows of one batch tie on the minimal delta."""
import numpy as np
import pytest

from oracle import oracle as O
from helpers import rand_instance, random_tour

pytestmark = pytest.mark.gpu
COUNTERS = ("sweeps", "evals", "moves", "reversed")
SHARES_REF = {}


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


def _oracle(xy, wt, succ0):
    _, es, eo, est, _, _ = O.two_opt_best(xy, wt, succ0)
    return es, eo, est


def _check(eng, ctx, monkeypatch, xy, wt, succ0, env=None, expect=None):
    monkeypatch.setenv("TSP_NO_FILTER", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    inst = eng.Instance(ctx, xy, wt, 1)
    t = eng.Tours(inst, 1)
    assert "k_exh" in t.describe(eng.BEST), t.describe(eng.BEST)
    t.upload(succ0, 0.0)
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID)
    s, o, st = t.download()
    t.close()
    inst.close()
    assert rc == 0 and done
    es, eo, est = expect if expect is not None else _oracle(xy, wt, succ0)
    assert (s[0] == es).all() and o[0] == eo, (len(xy), env)
    assert tuple(st[0][k] for k in COUNTERS) == tuple(est[k] for k in COUNTERS), (len(xy), env)


@pytest.mark.parametrize("n", list(range(255, 263)) + list(range(510, 518)) + [1021, 1022, 1023, 1024])
def test_row_batches_at_every_residue_of_the_rows_mod_4(eng, ctx, monkeypatch, n):
    """A strip holds 255 pair-columns, and its rows up to the first column are walked in batches of four: eight consecutive
    sizes around one strip and around two put the last plain batch, the rows left over for the per-row form and the strips'
    row counts at every residue mod 4; 1021 ... 1024 the same with several waves per strip.  From a random tour the first
    batches of every wave hold several hitting rows."""
    xy = rand_instance(n, seed=4000 + n, hi=5000)
    _check(eng, ctx, monkeypatch, xy, O.EUC_2D, random_tour(n, np.random.default_rng(n)))


@pytest.mark.parametrize("n", [777, 1023])
@pytest.mark.parametrize("shares", ["0", "97,1,1,1", "10,20,30,40"])
def test_row_batches_whatever_rows_a_wave_starts_and_ends_at(eng, ctx, monkeypatch, shares, n):
    """TSP_EXH_SHARES moves the first and the last row of every wave's range: equal shares, one lopsided split that leaves
    most waves a row or two (less than a batch), and one that grows with the age group; from the greedy tour."""
    if n not in SHARES_REF:   # one reference descent per size, shared by the three splits
        xy = rand_instance(n, seed=7 * n, hi=50000)
        _, succ0, _ = O.greedy(xy, O.EUC_2D)
        SHARES_REF[n] = (xy, succ0, _oracle(xy, O.EUC_2D, succ0))
    xy, succ0, expect = SHARES_REF[n]
    _check(eng, ctx, monkeypatch, xy, O.EUC_2D, succ0, {"TSP_EXH_SHARES": shares}, expect)


@pytest.mark.parametrize("side", [17, 23])
@pytest.mark.parametrize("wt", [O.EUC_2D, O.CEIL_2D, O.ATT])
def test_row_batches_with_ties_in_adjacent_rows_of_a_lattice(eng, ctx, monkeypatch, wt, side):
    """A square lattice from a random tour: many pairs share the minimal delta, some of them in rows of one batch that are
    met together, and the first pair in (i < j) NODE order must win.  17 x 17 has two strips, whose rows nearly all
    cross the diagonal (the per-row form); 23 x 23 has three, the right-hand one with 274 rows in batches."""
    g = np.array([(10 * (k % side), 10 * (k // side)) for k in range(side * side)], dtype=np.float64)
    _check(eng, ctx, monkeypatch, g, wt, random_tour(len(g), np.random.default_rng(31)))


@pytest.mark.parametrize("width", [64, 256])
@pytest.mark.parametrize("wt", [O.EUC_2D, O.CEIL_2D, O.ATT])
def test_row_batches_on_a_lattice_walked_row_by_row(eng, ctx, monkeypatch, wt, width):
    """4 x 64 points (and 4 x 256, where most rows of the right-hand strips lie above the diagonal and go in batches), tour
    order = lattice order: consecutive tour positions are consecutive rows of one batch, and along a lattice row they hold
    pairs of equal delta."""
    g = np.array([(10 * (k % width), 10 * (k // width)) for k in range(4 * width)], dtype=np.float64)
    succ0 = np.roll(np.arange(len(g), dtype=np.int32), -1)
    _check(eng, ctx, monkeypatch, g, wt, succ0)


def test_row_batches_on_a_batch_of_five_tours(eng, ctx, monkeypatch):
    """grid.z = tour: five descents at once, each the oracle's."""
    monkeypatch.setenv("TSP_NO_FILTER", "1")
    n = 400
    xy = rand_instance(n, seed=17, hi=30000)
    rng = np.random.default_rng(23)
    succ = np.stack([random_tour(n, rng) for _ in range(5)])
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    rc, s, o, st = inst.two_opt(succ, np.zeros(5), mode=eng.BEST, engine=eng.ENGINE_GRID)
    inst.close()
    assert rc == 0
    for b in range(5):
        _, es, eo, est, _, _ = O.two_opt_best(xy, O.EUC_2D, succ[b])
        assert (s[b] == es).all() and o[b] == eo, b
        assert tuple(st[b][k] for k in COUNTERS) == tuple(est[k] for k in COUNTERS), b
