"""GPU: the tail of k_exh and the decision behind it (csrc/two_opt_exh.hpp, csrc/exh_decide.hpp).  k_exh ends at one candidate
{delta, p, q} per workgroup, p < q tour positions, without loading a node id; k_move_pos (or k_exh_close before a poll) decides from the
positions, asks for ids only when two different pairs share the minimal delta, and orients the move by the ids at p and q --
k_move_pos<HOT> evaluates both orientations and keeps the one in which pa is the position of the smaller id.

Whole exhaustive descents (TSP_NO_FILTER=1) against the oracle (src/tabusearch.c:107-178): successor list, cost, sweeps, evals and
moves.  What each case pins is asserted on its INPUTS first (from the oracle's trace, or from a literal scan of every pair of a
sweep), then the device is compared:

  * n = 64 random: winners with the smaller id at the earlier position and at the later one (both orientations);
  * a 16 x 16 lattice with duplicate points, n = 320 (two strips), EUC_2D / CEIL_2D / ATT: a sweep with two different minimal pairs
    whose columns lie more than 255 apart (different strips, so different workgroups: k_move_pos's id fallback), one with two in
    neighbouring rows of one strip (waves of one workgroup: k_exh's fold of its waves) and one with two inside one lane's four
    columns (the tie path of a lane's own bookkeeping);
  * n = 257 with the winner in the overlap of strips 0 and 1: the same pair met twice is not ambiguous;
  * n = 255, 256, 511: strip 0 full, empty, one of two;
  * B = 3 tours that finish at different sweeps;
  * runs capped at 8 and 24 steps and continued: orientation and ties through k_exh_close and a pending move;
  * n = 1000 with equal shares and with a split that leaves half the waves without rows (they store empty candidates)."""
import numpy as np
import pytest

from oracle import oracle as O
from helpers import rand_instance, random_tour

pytestmark = pytest.mark.gpu
KEYS = ("sweeps", "evals", "moves")
WEFF = 255   # pair-columns per strip: 64 lanes x 4 columns of D, less one (two_opt_exh.hpp)


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


@pytest.fixture(autouse=True)
def _every_delta(monkeypatch):
    monkeypatch.setenv("TSP_NO_FILTER", "1")


_ORACLE = {}


def _oracle(key, xy, wt, succ0, max_sweeps=-1):
    """Computed once per (case, cap) and shared; never changed.  -> (succ, cost, counters, the moves (i, j, delta) in order)"""
    k = (key, max_sweeps)
    if k not in _ORACLE:
        _, es, eo, est, tr, _ = O.two_opt_best(xy, wt, succ0, max_sweeps=max_sweeps, trace_cap=4096)
        es.setflags(write=False)
        _ORACLE[k] = (es, eo, {q: est[q] for q in KEYS}, tuple(tr))
    return _ORACLE[k]


def _tours(eng, ctx, xy, wt, succ0, B=1):
    inst = eng.Instance(ctx, xy, wt, 1)
    t = eng.Tours(inst, B)
    assert "k_exh" in t.describe(eng.BEST), t.describe(eng.BEST)
    t.upload(succ0, 0.0)
    return inst, t


def _same(t, b, exp, what):
    es, eo, est = exp[:3]
    s, o, st = t.download()
    assert (s[b] == es).all(), what
    assert o[b] == eo, (what, o[b], eo)
    assert {k: st[b][k] for k in KEYS} == est, (what, st[b], est)


def _descent(eng, ctx, key, xy, wt, succ0, cap=-1):
    exp = _oracle(key, xy, wt, succ0, max_sweeps=cap)
    inst, t = _tours(eng, ctx, xy, wt, succ0)
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID, max_steps=cap)
    assert rc == 0 and bool(done) == (cap < 0)
    _same(t, 0, exp, what=key)
    t.close()
    inst.close()
    return exp[2]


def _rand_case(n, hi=20000):
    return rand_instance(n, seed=7000 + n, hi=hi), random_tour(n, np.random.default_rng(300 + n))


def _walk(succ):
    """The tour by position as the device numbers it: the walk from node 0."""
    out, v = [], 0
    for _ in range(len(succ)):
        out.append(v)
        v = int(succ[v])
    return out


def _reverse(order, i, j):
    """The reference's move for the pair i < j: the positions pos[i] + 1 .. pos[j] (cyclic) reversed, positions kept."""
    n = len(order)
    pa, pb = order.index(i), order.index(j)
    L = (pb - pa) % n
    for t in range(L // 2):
        a, b = (pa + 1 + t) % n, (pb - t) % n
        order[a], order[b] = order[b], order[a]


# ---- orientation -------------------------------------------------------------------------------------------------------------
def test_n_64_winners_with_the_smaller_id_at_the_earlier_and_at_the_later_position(eng, ctx):
    n = 64
    xy, succ0 = _rand_case(n)
    trace = _oracle(("rand", n), xy, O.EUC_2D, succ0)[3]
    assert len(trace) >= 20
    order, earlier, later = _walk(succ0), 0, 0
    for i, j, _ in trace:
        assert i < j
        if order.index(i) < order.index(j):
            earlier += 1
        else:
            later += 1
        _reverse(order, i, j)
    assert earlier >= 5 and later >= 5, (earlier, later)
    _descent(eng, ctx, ("rand", n), xy, O.EUC_2D, succ0)


# ---- ties: between workgroups (k_move_pos's id fallback), between a workgroup's waves and inside a lane ---------------------------------------------------------------
def _lattice(wt):
    """All 256 points of a 16 x 16 lattice and 64 of them once more, in an order of their own; the start is the greedy tour: its
    improving moves are small from the first sweep on, and on a lattice small deltas are shared by many pairs."""
    rng = np.random.default_rng(16)
    pts = np.array([(x, y) for x in range(16) for y in range(16)], dtype=np.float64) * 10.0
    xy = np.concatenate([pts, pts[rng.choice(256, size=64, replace=False)]])
    xy = np.ascontiguousarray(xy[rng.permutation(len(xy))])
    return xy, O.greedy(xy, wt)[1]


def _minimal_pairs(M, order):
    """Every non-adjacent pair of positions p < q of one sweep, literally: delta = d(u_p, u_q) + d(u_p+1, u_q+1) - d(u_p, u_p+1) -
    d(u_q, u_q+1).  -> the pairs that hold the minimal delta (none if it is not negative)."""
    n = len(order)
    o = np.array(order)
    o1 = np.roll(o, -1)
    D = M[np.ix_(o, o)] + M[np.ix_(o1, o1)] - M[o, o1][:, None] - M[o, o1][None, :]
    p, q = np.triu_indices(n, k=2)
    keep = ~((p == 0) & (q == n - 1))
    p, q = p[keep], q[keep]
    d = D[p, q]
    lo = d.min()
    if lo >= 0:
        return []
    at = np.flatnonzero(d == lo)
    return [(int(p[k]), int(q[k])) for k in at]


def _lanes(n, p, q):
    """The (strip, row, lane) triples in which k_exh evaluates the pair (p, q): D-column q + 1 of a strip that starts at q0 and
    has the pair-rows p < rows (exh_strip, exh_arith.hpp: right-aligned, strip 0 clamped to 0 over strip 1), four adjacent
    D-columns per lane.  A row is one wave's at the least, so two pairs that share a triple meet in one lane's bookkeeping
    whatever the dealing.  (At this size every wave of the grid has one row, in the order of the strips' rows laid end to end,
    and a workgroup has four waves: rows 4 m .. 4 m + 3 of a strip are one workgroup's -- strip 0 has 64 rows.)"""
    strips = (n + WEFF - 1) // WEFF
    out = set()
    for s in range(strips):
        q0 = s * WEFF - (strips * WEFF - n)
        rows = min(q0 + WEFF - 1, n - 1)
        q0 = max(0, q0)
        if q0 < q + 1 <= q0 + WEFF and p < rows:
            out.add((s, p, (q + 1 - q0) // 4))
    return out


@pytest.mark.parametrize("wt", [O.EUC_2D, O.CEIL_2D, O.ATT])
def test_ties_on_a_lattice_between_workgroups_between_waves_and_inside_one_lane(eng, ctx, wt):
    xy, succ0 = _lattice(wt)
    n = len(xy)
    assert n == 320
    trace = _oracle(("lattice", wt), xy, wt, succ0)[3]
    M = np.asarray(O.dist_matrix(xy, wt), dtype=np.int64)
    order, far, lane, block = _walk(succ0), 0, 0, 0
    for i, j, _ in trace:
        pairs = _minimal_pairs(M, order)
        assert pairs and (min(order.index(i), order.index(j)), max(order.index(i), order.index(j))) in pairs
        for a in range(len(pairs)):
            for b in range(a + 1, len(pairs)):
                far += abs(pairs[a][1] - pairs[b][1]) > 255
                la, lb = _lanes(n, *pairs[a]), _lanes(n, *pairs[b])
                lane += bool(la & lb)
                block += any(s == t and r != u and r // 4 == u // 4 for s, r, _ in la for t, u, _ in lb)
        _reverse(order, i, j)
    assert far > 0 and lane > 0 and block > 0, (far, lane, block)
    est = _descent(eng, ctx, ("lattice", wt), xy, wt, succ0)
    assert est["moves"] >= 30


# ---- the same pair in two slots ---------------------------------------------------------------------------------------------------
def test_winning_pair_in_the_overlap_of_strips_0_and_1_is_one_pair(eng, ctx):
    """n = 257: strip 0 is one row (p = 0) over the columns 0 .. 255 and strip 1 starts at row 0 too, so the pairs (0, q) are
    evaluated by two waves (of one workgroup at this size): the same pair twice is one pair, not a tie between two.  The start is a local optimum with the positions 1 .. k
    reversed, k chosen so that the first sweep's move takes exactly that back: the pair (0, k)."""
    n = 257
    xy, succ0 = _rand_case(n)
    opt = _walk(_oracle(("rand", n), xy, O.EUC_2D, succ0)[0])
    found = None
    for k in range(100, 140):
        order = [opt[0]] + opt[1:k + 1][::-1] + opt[k + 1:]
        start = np.empty(n, dtype=np.int32)
        start[order] = np.roll(order, -1)
        first = _oracle(("overlap", k), xy, O.EUC_2D, start, max_sweeps=1)
        back = _walk(first[0])
        if first[2]["moves"] == 1 and (back == opt or back == [opt[0]] + opt[1:][::-1]):
            found = (k, start, first)
            break
    assert found, "no k in 100 .. 139 whose reversal the first sweep takes back"
    k, start, first = found
    inst, t = _tours(eng, ctx, xy, O.EUC_2D, start)
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID, max_steps=1)
    assert rc == 0 and not done
    _same(t, 0, first, what=("overlap", k))
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID)
    assert rc == 0 and done
    _same(t, 0, _oracle(("overlap", k), xy, O.EUC_2D, start), what=("overlap", k, "rest"))
    t.close()
    inst.close()


# ---- strip 0 full, empty, one of two ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 511])
def test_whole_descent_where_strip_0_is_full_empty_or_one_of_two(eng, ctx, n):
    xy, succ0 = _rand_case(n)
    est = _descent(eng, ctx, ("rand", n), xy, O.EUC_2D, succ0)
    assert est["sweeps"] >= 2


# ---- a batch whose tours end at different times -----------------------------------------------------------------------------------
def test_three_tours_that_finish_at_different_sweeps(eng, ctx):
    n = 200
    xy, succ0 = _rand_case(n)
    _, greedy, _ = O.greedy(xy, O.EUC_2D)
    starts = [succ0, np.array(_oracle(("greedy", n), xy, O.EUC_2D, greedy)[0]), greedy]
    names = [("rand", n), ("opt", n), ("greedy", n)]
    exp = [_oracle(k, xy, O.EUC_2D, s) for k, s in zip(names, starts)]
    assert len({e[2]["sweeps"] for e in exp}) == 3 and exp[1][2]["sweeps"] == 1
    inst, t = _tours(eng, ctx, xy, O.EUC_2D, np.stack(starts), B=3)
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID)
    assert rc == 0 and done
    for b in range(3):
        _same(t, b, exp[b], what=("batch", b))
    t.close()
    inst.close()


# ---- k_exh_close and a pending move -----------------------------------------------------------------------------------------------
def test_runs_capped_at_8_and_24_steps_and_continued_to_the_end(eng, ctx):
    xy, succ0 = _lattice(O.EUC_2D)
    full = _oracle(("lattice", O.EUC_2D), xy, O.EUC_2D, succ0)
    assert full[2]["sweeps"] > 32
    inst, t = _tours(eng, ctx, xy, O.EUC_2D, succ0)
    total = 0
    for cap in (8, 24):
        rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID, max_steps=cap)
        assert rc == 0 and not done
        total += cap
        _same(t, 0, _oracle(("lattice", O.EUC_2D), xy, O.EUC_2D, succ0, max_sweeps=total), what=("capped", total))
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID)
    assert rc == 0 and done
    _same(t, 0, full, what="continued")
    t.close()
    inst.close()


# ---- waves without rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shares", ["0", "60,40,0,0"])
def test_n_1000_with_equal_shares_and_with_half_the_waves_without_rows(eng, ctx, monkeypatch, shares):
    monkeypatch.setenv("TSP_EXH_SHARES", shares)
    xy, succ0 = _rand_case(1000, hi=1_000_000)
    _descent(eng, ctx, ("rand", 1000), xy, O.EUC_2D, succ0, cap=60)
