"""GPU: the two ends of a k_exh launch (csrc/two_opt_exh.hpp).  k_move_pos and k_exh take their leading arguments from the
SGPRs the wave starts with (kernel-argument preload: both kernels' parameters are ordered for it, and k_exh no longer gets a struct),
so a wave asks for `done`, its descriptor and the candidates before any load of its own has come back; at the tail the block's
candidate, the winner's positions and `open` are stored through pointers that arrive by the entry's scalar loads.  Whole exhaustive
descents (TSP_NO_FILTER=1) must end in the oracle's tour (src/tabusearch.c:107-178) with its cost and its sweeps, evals and moves,
at the smallest shapes at which the start of a wave, its descriptor and its best pair can go wrong:

  * n = 254 .. 257, 511, 766: one strip, one strip filled, strip 0 without rows (256, 511), strip 0 clamped over strip 1 (257),
    three and four strips;
  * CEIL_2D and ATT once each;
  * ties: a 16 x 16 lattice with duplicate points (many pairs share the minimal delta inside a lane's history, between lanes,
    waves and workgroups) on all three metrics, and the winner in the overlap of strips 0 and 1;
  * n = 1000 with the default shares, equal shares and a split whose last parts are one row each;
  * a finished tour, alone and in a batch, run again once it is finished: every launch then starts with `done` set;
  * a capped run continued behind a poll (pending move through k_exh_close), reset, and a second descent on the same handle.

(The cases were chosen for two further changes to the ends of k_exh that were measured and not kept, DESIGN 4.9 -- the wave's
descriptor in closed form, the ids of a lane's best pair asked for where the pair is taken; they passed this file too.)"""
import numpy as np
import pytest

from oracle import oracle as O
from helpers import load_instance, rand_instance, random_tour

pytestmark = pytest.mark.gpu
KEYS = ("sweeps", "evals", "moves")


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


def _tours(eng, ctx, xy, wt, succ0, B=1, obj0=0.0):
    inst = eng.Instance(ctx, xy, wt, 1)
    t = eng.Tours(inst, B)
    assert "k_exh" in t.describe(eng.BEST), t.describe(eng.BEST)
    t.upload(succ0, obj0)
    return inst, t


_ORACLE = {}


def _oracle(key, xy, wt, succ0, max_sweeps=-1):
    """Computed once per (case, cap) and shared; never changed."""
    k = (key, max_sweeps)
    if k not in _ORACLE:
        _, es, eo, est, _, _ = O.two_opt_best(xy, wt, succ0, max_sweeps=max_sweeps)
        es.setflags(write=False)
        _ORACLE[k] = (es, eo, {q: est[q] for q in KEYS})
    return _ORACLE[k]


def _same(t, b, es, eo, est, what):
    s, o, st = t.download()
    assert (s[b] == es).all(), what
    assert o[b] == eo, (what, o[b], eo)
    assert {k: st[b][k] for k in KEYS} == est, (what, st[b], est)


def _descent(eng, ctx, key, xy, wt, succ0, cap=-1):
    es, eo, est = _oracle(key, xy, wt, succ0, max_sweeps=cap)
    inst, t = _tours(eng, ctx, xy, wt, succ0)
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID, max_steps=cap)
    assert rc == 0 and bool(done) == (cap < 0)
    _same(t, 0, es, eo, est, what=key)
    t.close()
    inst.close()
    return est


def _rand_case(n, hi=20000):
    return rand_instance(n, seed=9000 + n, hi=hi), random_tour(n, np.random.default_rng(100 + n))


# ---- the head: `done`, the descriptor and the walk over the strips ---------------------------------------------------------------
@pytest.mark.parametrize("n", [254, 255, 256, 257, 511, 766])
def test_whole_descent_where_the_strip_count_and_strip_0_change(eng, ctx, n):
    xy, succ0 = _rand_case(n)
    est = _descent(eng, ctx, ("rand", n), xy, O.EUC_2D, succ0)
    assert est["sweeps"] >= 2


def test_ceil_2d_with_strip_0_without_rows(eng, ctx):
    xy, succ0 = _rand_case(256)
    _descent(eng, ctx, ("ceil", 256), xy, O.CEIL_2D, succ0)


def test_att_on_the_first_300_nodes_of_att532(eng, ctx):
    xy, _ = load_instance("att532")
    xy = np.ascontiguousarray(xy[:300])
    _descent(eng, ctx, ("att", 300), xy, O.ATT, random_tour(300, np.random.default_rng(533)))


@pytest.mark.parametrize("shares", [None, "0", "60,40,0,0"])
def test_n_1000_with_the_default_shares_equal_shares_and_a_two_part_split(eng, ctx, monkeypatch, shares):
    if shares is not None:
        monkeypatch.setenv("TSP_EXH_SHARES", shares)
    xy, succ0 = _rand_case(1000, hi=1_000_000)
    _descent(eng, ctx, ("rand", 1000), xy, O.EUC_2D, succ0, cap=60)


# ---- the tail: the best pair, its tie-break on node ids and its positions --------------------------------------------------------
def _lattice():
    """All 256 points of a 16 x 16 lattice and 64 of them once more, in an order of their own."""
    rng = np.random.default_rng(16)
    pts = np.array([(x, y) for x in range(16) for y in range(16)], dtype=np.float64) * 10.0
    xy = np.concatenate([pts, pts[rng.choice(256, size=64, replace=False)]])
    return np.ascontiguousarray(xy[rng.permutation(len(xy))]), random_tour(len(xy), np.random.default_rng(17))


@pytest.mark.parametrize("wt", [O.EUC_2D, O.CEIL_2D, O.ATT])
def test_ties_on_a_lattice_with_duplicate_points(eng, ctx, wt):
    xy, succ0 = _lattice()
    est = _descent(eng, ctx, ("lattice", wt), xy, wt, succ0)
    assert est["moves"] >= 50


def _order_from(succ):
    out, v = [], 0
    for _ in range(len(succ)):
        out.append(v)
        v = int(succ[v])
    return out


def test_winning_pair_in_the_overlap_of_strips_0_and_1(eng, ctx):
    """n = 257: strip 0 is one row (p = 0) over the columns 0 .. 255 and strip 1 starts at row 0 too, so the pairs (0, q) are
    evaluated by two waves, which must build the same key and leave the same positions.  The start is a local optimum with the
    positions 1 .. k reversed, k chosen so that the first sweep's move takes exactly that back: the pair (0, k)."""
    n = 257
    xy, succ0 = _rand_case(n)
    opt = _order_from(_oracle(("rand", n), xy, O.EUC_2D, succ0)[0])
    found = None
    for k in range(100, 140):
        order = [opt[0]] + opt[1:k + 1][::-1] + opt[k + 1:]
        start = np.empty(n, dtype=np.int32)
        start[order] = np.roll(order, -1)
        es, eo, est = _oracle(("overlap", k), xy, O.EUC_2D, start, max_sweeps=1)
        back = _order_from(es)
        if est["moves"] == 1 and (back == opt or back == [opt[0]] + opt[1:][::-1]):
            found = (k, start, (es, eo, est))
            break
    assert found, "no k in 100 .. 139 whose reversal the first sweep takes back"
    k, start, first = found
    inst, t = _tours(eng, ctx, xy, O.EUC_2D, start)
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID, max_steps=1)
    assert rc == 0 and not done
    _same(t, 0, *first, what=("overlap", k))
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID)
    assert rc == 0 and done
    _same(t, 0, *_oracle(("overlap", k), xy, O.EUC_2D, start), what=("overlap", k, "rest"))
    t.close()
    inst.close()


# ---- finished tours ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_a_tour_that_is_finished_at_upload_alone_and_beside_running_ones(eng, ctx, B):
    n, cap = 1000, 40
    xy, succ0 = _rand_case(n, hi=1_000_000)
    _, greedy, _ = O.greedy(xy, O.EUC_2D)
    opt = np.array(_oracle(("greedy", n), xy, O.EUC_2D, greedy)[0])   # a local optimum: finished by its first sweep
    starts = [opt] if B == 1 else [succ0, opt, greedy]
    names = [("opt", n)] if B == 1 else [("rand", n), ("opt", n), ("greedy", n)]
    exp = [_oracle(k, xy, O.EUC_2D, s, max_sweeps=cap) for k, s in zip(names, starts)]
    fin = 0 if B == 1 else 1
    assert exp[fin][2]["sweeps"] == 1 and exp[fin][2]["moves"] == 0
    inst, t = _tours(eng, ctx, xy, O.EUC_2D, np.stack(starts), B=B)
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID, max_steps=cap)
    assert rc == 0 and bool(done) == (B == 1)
    for b in range(B):
        _same(t, b, *exp[b], what=(B, b))
    # once more: every launch of the finished tour now starts with `done` set
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID, max_steps=3)
    assert rc == 0
    _same(t, fin, *exp[fin], what=(B, fin, "again"))
    t.close()
    inst.close()


# ---- the decision by k_exh_close, reset and a second descent ---------------------------------------------------------------------
def test_capped_run_continued_behind_a_poll_then_reset_and_a_second_descent(eng, ctx):
    n = 320
    xy, succ0 = _rand_case(n)
    full = _oracle(("rand", n), xy, O.EUC_2D, succ0)
    assert full[2]["sweeps"] > 30
    inst, t = _tours(eng, ctx, xy, O.EUC_2D, succ0)
    for cap in (5, 9):
        rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID, max_steps=cap)
        assert rc == 0 and not done
    _same(t, 0, *_oracle(("rand", n), xy, O.EUC_2D, succ0, max_sweeps=14), what="5 + 9 sweeps")
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID)
    assert rc == 0 and done
    _same(t, 0, *full, what="continued")
    t.reset()
    rc, done = t.run_engine(eng.BEST, engine=eng.ENGINE_GRID)
    assert rc == 0 and done
    _same(t, 0, *full, what="after reset")
    t.close()
    inst.close()
