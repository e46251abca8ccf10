"""Windowed iterated local search with Lin-Kernighan chains on the device (tsp_dev_seg_ils_lk) against the CPU reference of the
definition in include/tsp_hip.h (tests/seg_lk_ref.py): one window of nine, small instances over the kinds 8, 9 and 15, the depths 1,
2 and 16, lists of one and of sixteen entries, every metric, pr299 over both kinds of lists with W = 149 and W = n - 1, a window
across position n - 1, the largest window, decisions with more chains than the kernel runs side by side, groups, chains of a batch,
the time limit, caps, two runs, bad arguments, the older entry points and the host library.  Tour, cost and every counter, the five
of the chain kind among them (deltas_executed and the times left out), must equal the reference's bit for bit.  GEO is compared as
in tests/test_gpu_seg_ils3.py: on the device's own distance matrix, and with non-integer costs its two tour costs to 1e-12.  A
parity case also asserts from the device's counters that chains were applied and that one of them was deeper than one reversal:
conditions on the inputs, which the reference alone meets.  Every device call passes a finite time limit."""
import ctypes as C

import numpy as np
import pytest

import nl_opt_ref as NL
import seg_groups_ref as SG
import seg_ils3_ref as S3
import seg_ils_ref as SR
import seg_lk_ref as SL
from helpers import HostInstance, Instance, load_instance, rand_instance, random_tour
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LIMIT = 300.0      # a call that does not end is a failure, not a hang
STATS = SL.COUNTERS + ("start_cost",)
CHAIN_GROUPS = 16  # chains the kernel runs side by side: 256 threads / 16 lanes


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


def _same(dev_succ, dev_obj, dev_st, ref_succ, ref_cost, ref_st, rel=0.0):
    """rel: of the two tour costs alone, for the one metric whose device matrix need not be symmetric to the bit (GEO, non-integer)"""
    assert O.is_tour(dev_succ)
    assert (dev_succ == np.asarray(ref_succ)).all(), "tour differs from the reference"
    close = lambda a, b: np.float64(a).tobytes() == np.float64(b).tobytes() or abs(a - b) <= rel * abs(b)   # noqa: E731
    assert close(dev_obj, ref_cost), (dev_obj, ref_cost)
    for k in STATS:
        assert dev_st[k] == ref_st[k] or (k == "start_cost" and close(dev_st[k], ref_st[k])), (k, dev_st[k], ref_st[k])


def _setup(eng, ctx, name, lists="knn", K=5, integer_cost=1, wt=None):
    xy, w = load_instance(name)
    wt = w if wt is None else wt
    inst = eng.Instance(ctx, xy, wt, integer_cost)
    # GEO is the tolerance tier (cos / acos differ in the last ulp between libraries): compared on the device's own distances
    D = inst.dist_matrix()[0] if wt == O.GEO else O.dist_matrix(xy, wt, integer_cost)
    K = min(K, len(xy) - 1)
    if lists == "alpha":
        nbr = inst.alpha_build(K)
        nbr = nbr[0] if isinstance(nbr, tuple) else nbr
    else:
        inst.knn_build(K)
        nbr = inst.knn()
    return xy, wt, D, inst, nbr


def _compare(inst, D, nbr, start, iterations, kinds=15, depth=6, groups=1, window=0, span=0, trials=1, seed=0, cap=-1, rel=0.0,
             log=None, glog=None):
    """one call against the reference -> the device's stats"""
    ref, cost, rst = SL.run(D, start, nbr, kinds, seed, 0, iterations, depth, groups, window, span, trials, max_moves=cap, log=log,
                            glog=glog)
    rc, s, o, st = inst.seg_ils_lk(start, iterations, kinds, depth, groups, window, span, trials, seed=seed, max_moves=cap,
                                   time_limit=LIMIT)
    assert rc == 0
    _same(s, o, st, ref, cost, rst, rel)
    assert st["deltas_executed"] > 0 or st["decisions"] == 0 or not kinds & 7
    assert st["moves"] == st["moves_2opt"] + st["moves_oropt"] + st["moves_3opt"] + st["moves_lk"]
    assert st["trials"] == st["iterations"] * st["windows"] * st["groups"] * trials
    return st


def _alive(st, deeper=True):
    """the case ran the chain code: chains were applied, and one of them was deeper than one reversal"""
    assert st["moves_lk"] > 0, st
    assert not deeper or st["lk_flips"] > st["moves_lk"], st


def _sum(total, st):
    for k in ("moves_lk", "lk_flips", "lk_steps", "lk_chains", "accepted", "trials"):
        total[k] = total.get(k, 0) + st[k]
    return total


# ---- 1. the smallest shapes, small instances, depths, list lengths, the metrics -----------------------------------------------------

@pytest.mark.parametrize("n", [10, 11])
def test_one_window_of_nine_nodes(eng, ctx, n):
    """a chain there has at most the slots i + 3 .. 8"""
    xy = rand_instance(n, seed=n, hi=1000)
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    total = {8: {}, 15: {}}
    for K in (n - 1, 3):
        inst.knn_build(K)
        nbr = inst.knn()
        for q in range(4):
            start = random_tour(n, np.random.default_rng(10 * n + q))
            for kinds in (8, 15):
                st = _compare(inst, D, nbr, start, 6, kinds, 6, 1, 9, 0, 2, seed=q)
                assert st["windows"] == 1 and st["trials"] == 12 and st["lk_depth"] == 6
                if kinds == 8:
                    assert st["moves"] == st["moves_lk"] and st["reversed"] == 0
                _sum(total[kinds], st)
    inst.close()
    _alive(total[8])
    _alive(total[15])


@pytest.mark.parametrize("kinds", [8, 9, 15])
@pytest.mark.parametrize("name,window,span,trials,seed", [("burma14", 9, 8, 2, 7), ("ulysses22", 11, 8, 2, 5), ("ulysses22", 9, 8, 2, 7),
                                                          ("att48", 23, 8, 2, 5), ("kroA100", 49, 12, 3, 5)])
def test_small_instances_equal_the_reference(eng, ctx, name, window, span, trials, seed, kinds):
    """the seeds: with a window of nine and every kind at work few applied moves are chains; under seed 7 some are"""
    xy, wt, D, inst, nbr = _setup(eng, ctx, name)
    n = len(xy)
    st = _compare(inst, D, nbr, random_tour(n, np.random.default_rng(n)), 3, kinds, 6, 1, window, span, trials, seed=seed)
    inst.close()
    assert st["windows"] == n // window and 0 < st["accepted"] <= st["trials"]
    _alive(st)


@pytest.mark.parametrize("depth", [1, 2, 16])
def test_the_depths_on_att48(eng, ctx, depth):
    """Or-opt and chains: beside 2-opt a chain of one reversal is never applied, it is a 2-opt move and loses the tie"""
    xy, wt, D, inst, nbr = _setup(eng, ctx, "att48")
    st = _compare(inst, D, nbr, random_tour(48, np.random.default_rng(48)), 3, 10, depth, 1, 23, 8, 2, seed=5)
    inst.close()
    assert st["lk_depth"] == depth
    _alive(st, deeper=depth > 1)                      # with D = 1 no chain is deeper than one reversal
    if depth == 1:
        assert st["lk_flips"] == st["moves_lk"] and st["lk_steps"] <= st["lk_chains"]
    if depth == 16:
        assert st["lk_steps"] > st["lk_flips"]        # reversals were made and not kept


def test_no_depth_given_is_the_constant(eng, ctx):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "att48")
    start = random_tour(48, np.random.default_rng(48))
    st = _compare(inst, D, nbr, start, 2, 9, 0, 1, 23, 8, 2, seed=5)
    assert st["lk_depth"] == eng.SEG_LK_DEFAULT_DEPTH == SL.DEFAULT_DEPTH
    for depth in (-4, eng.SEG_LK_DEFAULT_DEPTH):
        rc, s, o, st1 = inst.seg_ils_lk(start, 2, 9, depth, 1, 23, 8, 2, seed=5, time_limit=LIMIT)
        assert rc == 0 and all(st1[k] == st[k] for k in STATS)
    inst.close()


@pytest.mark.parametrize("K", [1, 16])
def test_lists_of_one_entry_and_of_sixteen(eng, ctx, K):
    """K = 16: the sixteen lanes of a chain are all at work"""
    assert eng.NL_MAX_K == 16
    xy, wt, D, inst, nbr = _setup(eng, ctx, "att48", K=K)
    assert nbr.shape == (48, K)
    st = _compare(inst, D, nbr, random_tour(48, np.random.default_rng(48)), 3, 8 if K == 1 else 15, 6, 1, 23, 8, 2, seed=5)
    inst.close()
    _alive(st)


@pytest.mark.parametrize("wt,integer_cost", [("MAN_2D", 1), ("MAX_2D", 1), ("CEIL_2D", 1), ("EUC_2D", 0), ("ATT", 0), ("GEO", 0)])
def test_the_other_metrics_and_non_integer_costs(eng, ctx, wt, integer_cost):
    name = {"ATT": "att48", "GEO": "ulysses22"}.get(wt, "kroA100")
    xy, wtype, D, inst, nbr = _setup(eng, ctx, name, integer_cost=integer_cost, wt=getattr(O, wt))
    n = len(xy)
    st = _compare(inst, D, nbr, random_tour(n, np.random.default_rng(n)), 3, 15, 6, 1, 11 if n < 30 else 20, 10, 2, seed=4,
                  rel=1e-12 if (wt, integer_cost) == ("GEO", 0) else 0.0)
    inst.close()
    assert st["accepted"] > 0
    _alive(st)


# ---- 2. pr299, a window that wraps, the largest window, more chains than one pass holds ------------------------------------------------

@pytest.mark.parametrize("window", [149, 298])
@pytest.mark.parametrize("lists", ["knn", "alpha"])
def test_pr299_over_lists_and_windows(eng, ctx, lists, window):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "pr299", lists)
    start = np.asarray(O.greedy(xy, wt)[1], dtype=np.int32)
    st = _compare(inst, D, nbr, start, 2, 15, 6, 1, window, 50, 2, seed=3)
    inst.close()
    assert st["windows"] == 299 // window and st["trials"] == 4 * st["windows"]
    _alive(st)


def _straddles(start, seed, W):
    """a window of iteration 0 lies across position n - 1 of the device's order, which starts at node 0"""
    n = len(start)
    p0 = int(np.flatnonzero(NL.R.tour_order(start) == SR.anchor(n, seed, 0, 0))[0])
    return any(p0 + w * W <= n - 1 < p0 + w * W + W - 1 for w in range(n // W))


def test_a_window_across_the_last_position_of_the_order(eng, ctx):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "kroA100")
    start = random_tour(100, np.random.default_rng(5))
    across = [seed for seed in range(40) if _straddles(start, seed, 30)]
    within = [seed for seed in range(40) if not _straddles(start, seed, 30)]
    assert across and within, "the seeds give no window across position n - 1, or none within"
    for seed in across[:2] + within[:1]:
        st = _compare(inst, D, nbr, start, 1, 9, 6, 1, 30, 20, 3, seed=seed)
        assert st["windows"] == 3
        _alive(st)
    inst.close()


def test_the_largest_window(eng, ctx):
    W = SR.MAX_WINDOW
    n = 2100
    assert W == eng.SEG_ILS_MAX_WINDOW
    xy = rand_instance(n, seed=n, hi=100000)
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    inst.knn_build(5)
    nbr = inst.knn()
    start = random_tour(n, np.random.default_rng(n))       # far from a local optimum: the active set grows
    log = []
    st = _compare(inst, D, nbr, start, 1, 15, 16, 1, W, 0, 1, seed=6, cap=6, log=log)
    assert st["windows"] == 1 and st["trials"] == 1 and st["moves"] == 6
    assert max(r[1] for r in log if r[0] == "decision") * 2 > 4 * CHAIN_GROUPS          # several passes of chains
    _alive(st)
    with pytest.raises(eng.TspDeviceError, match="-3"):
        inst.seg_ils_lk(start, 1, 15, 6, 1, W + 1, time_limit=LIMIT)
    inst.close()


def test_more_chains_in_a_decision_than_the_kernel_runs_side_by_side(eng, ctx):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "kroA100")
    log = []
    st = _compare(inst, D, nbr, random_tour(100, np.random.default_rng(100)), 2, 8, 6, 1, 49, 12, 2, seed=5, log=log)
    inst.close()
    sizes = [r[1] for r in log if r[0] == "decision"]
    assert max(sizes) * 2 > CHAIN_GROUPS and min(sizes) * 2 <= CHAIN_GROUPS, (min(sizes), max(sizes))
    assert any(2 * a % CHAIN_GROUPS for a in sizes)            # a last pass that is not full
    _alive(st)


# ---- 3. groups ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kro(eng, ctx):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "kroA100")
    start = random_tour(100, np.random.default_rng(100))
    yield D, inst, nbr, start
    inst.close()


@pytest.fixture(scope="module")
def kro_repaired(kro):
    """the tour that six iterations of the 3-opt windowed search leave of the random one: its trials change short intervals"""
    D, inst, nbr, start = kro
    return S3.run(D, start, nbr, 7, 1, 0, 6, 49, 8, 2)[0]


@pytest.mark.parametrize("kinds", [8, 15])
def test_six_groups_commit_several_chain_offers_of_a_window_and_drop_others(kro, kro_repaired, kinds):
    D, inst, nbr, _ = kro
    glog = []
    st = _compare(inst, D, nbr, kro_repaired, 3, kinds, 6, 6, 49, 8, 1, seed=7, glog=glog)
    assert st["groups"] == 6 and st["trials"] == 3 * 2 * 6
    assert any(len(keep) >= 2 for _, _, _, keep in glog), glog
    assert any(len(offers) > len(keep) for _, _, offers, keep in glog), glog
    assert sum(len(o) for _, _, o, _ in glog) == st["offers"] and sum(len(k) for _, _, _, k in glog) == st["commits"]
    _alive(st)


def test_no_groups_given_is_the_formula_of_the_groups(kro, kro_repaired):
    D, inst, nbr, _ = kro
    st = _compare(inst, D, nbr, kro_repaired, 1, 9, 6, 0, 49, 8, 1, seed=3, cap=2)
    assert st["groups"] == 64 == SG.default_groups(100, 49)
    _alive(st)


# ---- 4. the family's invariants ---------------------------------------------------------------------------------------------------------------

def test_chains_of_a_batch_are_single_calls_with_their_streams(kro):
    D, inst, nbr, start = kro
    rc, S, Ob, St = inst.seg_ils_lk(np.stack([start] * 3), 2, 15, 6, 2, 25, 10, 2, seed=11, time_limit=LIMIT)
    assert rc == 0
    for b in range(3):
        _same(S[b], Ob[b], St[b], *SL.run(D, start, nbr, 15, 11, b, 2, 6, 2, 25, 10, 2))
        _alive(St[b])
    assert len({tuple(s) for s in S}) > 1                    # the streams differ
    rc, s, o, st = inst.seg_ils_lk(start, 2, 15, 6, 2, 25, 10, 2, seed=11, time_limit=LIMIT)      # alone, it is stream 0
    assert (s == S[0]).all() and o == Ob[0] and all(st[k] == St[0][k] for k in STATS)


def test_a_time_limited_run_is_the_prefix_of_its_iterations_and_two_runs_return_the_same_bits(eng, ctx):
    n = 2000
    xy = rand_instance(n)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    inst.knn_build(5)
    start = np.asarray(O.greedy(xy, O.EUC_2D)[1], dtype=np.int32)
    rc, s, o, st = inst.seg_ils_lk(start, 10 ** 9, 15, 6, 4, 64, 50, 2, seed=3, time_limit=0.3)
    assert rc == eng.TIME_LIMIT_EXCEEDED
    assert O.is_tour(s) and o == O.succ_cost(xy, O.EUC_2D, s) and o < st["start_cost"] and st["iterations"] > 0
    assert st["groups"] == 4 and st["trials"] == st["iterations"] * 31 * 4 * 2
    _alive(st)
    for _ in range(2):
        rc2, s2, o2, st2 = inst.seg_ils_lk(start, st["iterations"], 15, 6, 4, 64, 50, 2, seed=3, time_limit=LIMIT)
        assert rc2 == 0 and (s2 == s).all() and o2 == o
        assert all(st2[k] == st[k] for k in STATS + ("deltas_executed",))
    inst.close()


def test_a_cap_of_no_move_and_of_one_move(eng, ctx):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "att48")
    start = random_tour(48, np.random.default_rng(2))
    st = _compare(inst, D, nbr, start, 3, 9, 6, 1, 16, 0, 2, seed=1, cap=0)
    assert st["decisions"] == st["moves"] == st["active_nodes"] == st["lk_chains"] == 0 and st["trials"] == 18
    st = _compare(inst, D, nbr, start, 3, 9, 6, 1, 16, 0, 2, seed=1, cap=1)
    assert 0 < st["moves"] == st["decisions"] <= st["trials"]       # a chain of several reversals is one move
    _alive(st)
    inst.close()


# ---- 5. refusals, the older path ----------------------------------------------------------------------------------------------------------

def test_bad_arguments_leave_the_tours_alone_and_the_handle_usable(eng, ctx):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "att48")
    n = len(xy)
    start = random_tour(n, np.random.default_rng(4))
    L = eng.lib()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    # (kinds, depth, groups, iterations, window, span, trials)
    bad = [(15, 17, 1, 5, 12, 0, 1), (8, 17, 1, 5, 12, 0, 1), (7, 17, 1, 5, 12, 0, 1), (15, 1000, 1, 5, 12, 0, 1)]
    bad += [(0, 6, 1, 5, 12, 0, 1), (16, 6, 1, 5, 12, 0, 1), (31, 6, 1, 5, 12, 0, 1), (-1, 6, 1, 5, 12, 0, 1)]
    bad += [(15, 6, 65, 5, 12, 0, 1), (15, 6, 1, -1, 12, 0, 1), (15, 6, 1, 5, 12, 0, 0), (15, 6, 1, 5, 8, 0, 1), (15, 6, 1, 5, n, 0, 1),
            (8, 6, 1, 5, 12, 7, 1), (8, 6, 1, 5, 12, 12, 1)]
    for kinds, depth, groups, iters, window, span, trials in bad:
        succ, obj = start.copy(), np.zeros(1)
        st = eng.SegIlsLkStats()
        rc = L.tsp_dev_seg_ils_lk(inst._h, kinds, depth, groups, 1, succ.ctypes.data_as(ip), 1, n, obj.ctypes.data_as(dp), 1, iters,
                                  window, span, trials, -1, LIMIT, C.byref(st))
        assert rc == eng.E_ARG and (succ == start).all(), (kinds, depth, groups, iters, window, span, trials)
        # the same handle, after each
        _alive(_compare(inst, D, nbr, start, 1, 8, 6, 1, 12, 8, 1, seed=2), deeper=False)
    # the three older entry points still refuse the chain kind
    for call in (lambda k: inst.seg_ils(start, 3, kinds=k, time_limit=LIMIT), lambda k: inst.seg_ils3(start, 3, kinds=k, time_limit=LIMIT),
                 lambda k: inst.seg_ils_groups(start, 3, 2, kinds=k, time_limit=LIMIT)):
        for k in (eng.NL_LK, 15):
            with pytest.raises(eng.TspDeviceError, match="-3"):
                call(k)
    # the limits themselves are arguments: D = 16, W = n - 1 with S = W - 1, W = 9 with S = 8
    _compare(inst, D, nbr, start, 1, 15, 16, 2, n - 1, n - 2, 1, seed=2, cap=3)
    _compare(inst, D, nbr, start, 1, 15, 1, 2, 9, 8, 1, seed=2, cap=3)
    inst.close()


def test_no_iterations_and_no_window_return_the_tour(eng, ctx):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "att48")
    start = random_tour(48, np.random.default_rng(1))
    rc, s, o, st = inst.seg_ils_lk(start, 0, 15, 3, 5, 12, time_limit=LIMIT)
    assert rc == 0 and (s == start).all() and o == st["start_cost"] == O.succ_cost(xy, wt, start)
    assert st["iterations"] == st["trials"] == st["moves_lk"] == st["lk_chains"] == 0 and st["windows"] == 4
    assert st["groups"] == 5 and st["lk_depth"] == 3
    inst.close()
    n = 9
    xy = rand_instance(n, seed=n, hi=100)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    start = random_tour(n, np.random.default_rng(n))
    rc, s, o, st = inst.seg_ils_lk(start, 7, time_limit=LIMIT)
    assert rc == 0 and (s == start).all() and o == st["start_cost"] == O.succ_cost(xy, O.EUC_2D, start)
    assert st["iterations"] == st["trials"] == st["windows"] == 0 and st["lk_depth"] == eng.SEG_LK_DEFAULT_DEPTH
    inst.close()


def test_without_the_chain_kind_it_returns_the_bits_of_seg_ils_groups(eng, ctx):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "pr299")
    start = np.asarray(O.greedy(xy, wt)[1], dtype=np.int32)
    shared = SG.COUNTERS + ("start_cost", "deltas_executed")
    for kinds in (1, 2, 3, 4, 7):
        for G in (1, 3):
            rcg, sg, og, stg = inst.seg_ils_groups(start, 4, G, 64, 50, 2, seed=3, kinds=kinds, time_limit=LIMIT)
            rc, s, o, st = inst.seg_ils_lk(start, 4, kinds, 5, G, 64, 50, 2, seed=3, time_limit=LIMIT)
            assert rc == rcg == 0 and (s == sg).all() and o == og and stg["moves"] > 0
            assert all(st[k] == stg[k] for k in shared)
            assert st["lk_depth"] == 5 and all(st[k] == 0 for k in SL.LK_COUNTERS[1:])
    inst.close()


# ---- 6. the host library ----------------------------------------------------------------------------------------------------------------------

def test_heu_seg_ils_greedy_edge_under_the_chain_setting_is_the_three_device_calls(eng, ctx):
    from tsp_optimization_amd.build import lib_path
    K, I, W, S, T = 5, 4, 64, 50, 2
    xy, wt = load_instance("pr299")
    inst = eng.Instance(ctx, xy, wt, 1)
    succ, obj = inst.greedy_edge()
    inst.knn_build(K)
    rc, s1, o1, _ = inst.nl_3opt_batch(succ, obj, kinds=7, time_limit=LIMIT)
    assert rc == 0
    want = {0: inst.seg_ils3(s1, I, W, S, T, seed=123, kinds=7, time_limit=LIMIT)}
    for depth in (4, 16, -1):
        want[depth] = inst.seg_ils_lk(s1, I, 15, max(depth, 0), 1, W, S, T, seed=123, time_limit=LIMIT)
    assert all(w[0] == 0 for w in want.values()) and want[-1][3]["lk_depth"] == eng.SEG_LK_DEFAULT_DEPTH
    _alive(want[4][3])
    inst.close()
    L = C.CDLL(lib_path("libtsp_host.so"))
    L.HEU_seg_ils_greedy_edge.argtypes = [C.POINTER(Instance)]
    L.tsp_host_last_seg_ils_lk_stats.argtypes = [C.POINTER(eng.SegIlsLkStats)]
    try:
        assert L.tsp_host_set_seg_ils_lk(17) == eng.E_ARG and L.tsp_host_set_seg_ils_lk(-2) == eng.E_ARG
        assert L.tsp_host_set_alpha(0, 0) == 0 and L.tsp_host_set_knn(K) == 0 and L.tsp_host_set_seg_ils(I, W, S, T) == 0
        assert L.tsp_host_set_seg_ils_kinds(7) == 0
        for depth in (None, 4, 16, -1, 0):
            if depth is not None:                               # None: the default, which is today's calls
                assert L.tsp_host_set_seg_ils_lk(depth) == 0
            rc, s2, o2, st = want[depth or 0]
            h = HostInstance("pr299")
            h.c.params.time_limit = int(LIMIT)
            assert L.HEU_seg_ils_greedy_edge(C.byref(h.c)) == 0
            assert (h.succ == s2).all() and h.obj == o2 == O.succ_cost(xy, wt, h.succ)
            hs = eng.SegIlsLkStats()
            L.tsp_host_last_seg_ils_lk_stats(C.byref(hs))
            d = hs.as_dict()
            assert all(d[k] == st[k] for k in S3.COUNTERS + ("start_cost", "deltas_executed"))
            if depth:
                assert all(d[k] == st[k] for k in SL.LK_COUNTERS + ("groups", "offers", "commits"))
            else:
                assert all(d[k] == 0 for k in SL.LK_COUNTERS)
    finally:
        L.tsp_host_set_seg_ils_lk(0)
        L.tsp_host_set_seg_ils_kinds(3)
        L.tsp_host_set_seg_ils(100, 0, 50, 1)
        L.tsp_host_set_knn(eng.NL_DEFAULT_K)
        L.tsp_host_shutdown()
