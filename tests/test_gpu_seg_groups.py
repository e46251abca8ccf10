"""Windowed iterated local search with groups on the device (tsp_dev_seg_ils_groups) against the CPU reference of the definition in
include/tsp_hip.h (tests/seg_groups_ref.py): the smallest shapes, kroA100 with windows that commit several groups and with offers
that lose, private accepts carried forward, 64 groups, the default number of groups, every metric, a window across position n - 1,
the largest window, more workgroups than the device holds at once, chains, the time limit, the older entry points at G = 1, bad
arguments and the host library.  Tour, cost and every counter, groups, offers and commits among them (deltas_executed and the
times left out), must equal the reference's bit for bit.  GEO is compared as in tests/test_gpu_seg_ils.py: on the device's own
distance matrix, and with non-integer costs its two tour costs to 1e-12.  Every device call passes a finite time limit."""
import ctypes as C

import numpy as np
import pytest

import nl_opt_ref as NL
import seg_groups_ref as SG
import seg_ils3_ref as S3
import seg_ils_ref as SR
from helpers import HostInstance, Instance, load_instance, rand_instance, random_tour
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LIMIT = 300.0      # a call that does not end is a failure, not a hang
STATS = SG.COUNTERS + ("start_cost",)


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


def _setup(eng, ctx, name, K=5, integer_cost=1, wt=None):
    xy, w = load_instance(name)
    wt = w if wt is None else wt
    inst = eng.Instance(ctx, xy, wt, integer_cost)
    # GEO is the tolerance tier (cos / acos differ in the last ulp between libraries): compared on the device's own distances
    D = inst.dist_matrix()[0] if wt == O.GEO else O.dist_matrix(xy, wt, integer_cost)
    inst.knn_build(min(K, len(xy) - 1))
    return xy, wt, D, inst, inst.knn()


def _compare(inst, D, nbr, start, iterations, groups, window=0, span=0, trials=1, seed=0, kinds=7, cap=-1, rel=0.0, log=None):
    """one call against the reference -> the device's stats"""
    ref, cost, rst = SG.run(D, start, nbr, kinds, seed, 0, iterations, groups, window, span, trials, max_moves=cap, log=log)
    rc, s, o, st = inst.seg_ils_groups(start, iterations, groups, window, span, trials, seed=seed, kinds=kinds,
                                       max_moves_per_trial=cap, time_limit=LIMIT)
    assert rc == 0
    _same(s, o, st, ref, cost, rst, rel)
    assert st["trials"] == st["iterations"] * st["windows"] * st["groups"] * trials
    assert st["commits"] <= st["offers"] <= st["accepted"] and (st["commits"] > 0) == (st["offers"] > 0)
    return st


def _by_window(log):
    """the log's records by (it, w) -> {(it, w): (offers, commits)}"""
    out = {}
    for it, w, g, offer, gain, lo, hi, committed in log:
        o, c = out.get((it, w), (0, 0))
        out[(it, w)] = (o + int(offer), c + int(committed))
    return out


# ---- 1. the smallest shapes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [10, 11])
def test_one_window_of_nine_nodes(eng, ctx, n):
    xy = rand_instance(n, seed=n, hi=1000)
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    offers = commits = 0
    for K in (n - 1, 3):
        inst.knn_build(K)
        nbr = inst.knn()
        for q in range(2):
            start = random_tour(n, np.random.default_rng(10 * n + q))
            for kinds in (4, 7):
                for G in (1, 2, 3, 4):
                    st = _compare(inst, D, nbr, start, 4, G, 9, 0, 2, seed=q, kinds=kinds)
                    assert st["windows"] == 1 and st["groups"] == G and st["trials"] == 8 * G
                    offers += st["offers"]
                    commits += st["commits"]
    inst.close()
    assert 0 < commits < offers, (offers, commits)


# ---- 2. kroA100: several commits in a window, offers that lose, hulls that span the window ----------------------------------------------------

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


def _several_and_losers(log, st):
    """conditions on the inputs: a set without both shows nothing of the commit rule"""
    per = _by_window(log)
    assert any(c >= 2 for _, c in per.values()), per
    assert any(o > c for o, c in per.values()), per
    assert sum(o for o, _ in per.values()) == st["offers"] and sum(c for _, c in per.values()) == st["commits"]


def test_kroA100_without_a_repair_commits_several_groups_of_a_window(kro):
    D, inst, nbr, start = kro
    log = []
    st = _compare(inst, D, nbr, start, 2, 6, 49, 8, 1, seed=5, cap=0, log=log)
    assert st["windows"] == 2 and st["trials"] == 24 and st["moves"] == 0
    _several_and_losers(log, st)


def test_kroA100_from_a_repaired_tour_commits_several_groups_of_a_window(kro, kro_repaired):
    D, inst, nbr, _ = kro
    log = []
    st = _compare(inst, D, nbr, kro_repaired, 2, 6, 49, 8, 1, seed=5, log=log)
    assert st["moves"] > 0
    _several_and_losers(log, st)


def test_kroA100_from_a_random_tour_every_hull_spans_its_window(kro):
    """an uncapped repair of a random tour rewrites the whole window: the offers of a window all conflict and the best alone commits"""
    D, inst, nbr, start = kro
    log = []
    st = _compare(inst, D, nbr, start, 2, 6, 49, 8, 1, seed=5, log=log)
    per = _by_window(log)
    assert all(c == 1 for _, c in per.values()) and any(o > 1 for o, _ in per.values()), per
    assert st["commits"] == 4 < st["offers"]


def test_private_accepts_carry_into_the_next_trial_of_their_group(kro, kro_repaired):
    D, inst, nbr, _ = kro
    st = _compare(inst, D, nbr, kro_repaired, 2, 4, 49, 8, 2, seed=2)
    assert st["trials"] == 2 * 2 * 4 * 2 and st["accepted"] > st["offers"] > 0      # some group accepted both of its trials


def test_sixty_four_groups(eng, kro, kro_repaired):
    D, inst, nbr, _ = kro
    assert eng.SEG_ILS_MAX_GROUPS == SG.MAX_GROUPS == 64
    st = _compare(inst, D, nbr, kro_repaired, 1, 64, 49, 8, 1, seed=2)
    assert st["groups"] == 64 and st["trials"] == 128 and st["commits"] >= 2


def test_no_groups_given_is_the_formula(kro, kro_repaired):
    """n = 100, W = 49: M = 2 windows, 1024 / 2 is above the ceiling of 64"""
    D, inst, nbr, _ = kro
    assert SG.default_groups(100, 49) == 64 == max(1, min(64, 1024 // (100 // 49)))
    st = _compare(inst, D, nbr, kro_repaired, 1, 0, 49, 8, 1, seed=3, cap=2)
    assert st["groups"] == 64
    for groups in (-3, 64):
        rc, s, o, st1 = inst.seg_ils_groups(kro_repaired, 1, groups, 49, 8, 1, seed=3, max_moves_per_trial=2, time_limit=LIMIT)
        assert rc == 0 and all(st1[k] == st[k] for k in STATS)


def test_the_formula_below_its_ceiling(eng, ctx):
    """n = 640, W = 9: M = 71 windows, 1024 / 71 = 14 groups"""
    n = 640
    xy = rand_instance(n, seed=n, hi=100000)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    inst.knn_build(5)
    start = np.asarray(O.greedy(xy, O.EUC_2D)[1], dtype=np.int32)
    rc, s0, o0, st0 = inst.seg_ils_groups(start, 2, 0, 9, 8, 1, seed=1, time_limit=LIMIT)
    rc1, s1, o1, st1 = inst.seg_ils_groups(start, 2, 14, 9, 8, 1, seed=1, time_limit=LIMIT)
    inst.close()
    assert rc == rc1 == 0 and st0["groups"] == 14 == SG.default_groups(n, 9) and st0["windows"] == 71
    assert (s0 == s1).all() and o0 == o1 and all(st0[k] == st1[k] for k in STATS + ("deltas_executed",))


# ---- 3. the metrics -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wt,integer_cost", [("EUC_2D", 1), ("MAN_2D", 1), ("MAX_2D", 1), ("CEIL_2D", 1), ("ATT", 1), ("GEO", 1),
                                             ("EUC_2D", 0), ("MAN_2D", 0), ("MAX_2D", 0), ("CEIL_2D", 0), ("ATT", 0), ("GEO", 0)])
def test_the_six_metrics_with_integer_and_non_integer_costs(eng, ctx, wt, integer_cost):
    n = 60
    xy = rand_instance(n, seed=7 * n, hi=90 if wt == "GEO" else 5000)       # GEO: degrees
    inst = eng.Instance(ctx, xy, getattr(O, wt), integer_cost)
    D = inst.dist_matrix()[0] if wt == "GEO" else O.dist_matrix(xy, getattr(O, wt), integer_cost)
    inst.knn_build(5)
    nbr = inst.knn()
    start = np.asarray(O.greedy(xy, getattr(O, wt))[1], dtype=np.int32)
    st = _compare(inst, D, nbr, start, 3, 3, 20, 10, 2, seed=4, kinds=7, rel=1e-12 if (wt, integer_cost) == ("GEO", 0) else 0.0)
    inst.close()
    assert st["windows"] == 3 and st["offers"] > 0


# ---- 4. windows that wrap -----------------------------------------------------------------------------------------------------------------

def _straddles(start, seed, W):
    """a window of iteration 0 lies across position n - 1 of the device's order, which starts at node 0"""
    n = len(start)
    p0 = int(np.flatnonzero(NL.R.tour_order(start) == SR.anchor(n, seed, 0, 0))[0])
    return any(p0 + w * W <= n - 1 < p0 + w * W + W - 1 for w in range(n // W))


def test_a_window_across_the_last_position_of_the_order(kro, kro_repaired):
    D, inst, nbr, _ = kro
    across = [seed for seed in range(40) if _straddles(kro_repaired, seed, 30)]
    within = [seed for seed in range(40) if not _straddles(kro_repaired, seed, 30)]
    assert across and within, "the seeds give no window across position n - 1, or none within"
    commits = 0
    for seed in across[:2] + within[:1]:
        st = _compare(inst, D, nbr, kro_repaired, 1, 3, 30, 20, 2, seed=seed)
        assert st["windows"] == 3 and st["groups"] == 3
        commits += st["commits"]
    assert commits > 0


# ---- 5. the largest window, more workgroups than the device holds ----------------------------------------------------------------------------

def test_the_largest_window(eng, ctx):
    W = SR.MAX_WINDOW
    n = 2100
    xy = rand_instance(n, seed=n, hi=100000)
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    inst.knn_build(5)
    nbr = inst.knn()
    start = random_tour(n, np.random.default_rng(n))
    st = _compare(inst, D, nbr, start, 1, 2, W, 0, 1, seed=6, kinds=7, cap=40)
    assert st["windows"] == 1 and st["trials"] == 2 and st["moves"] == 80 and st["commits"] == 1
    with pytest.raises(eng.TspDeviceError, match="-3"):
        inst.seg_ils_groups(start, 1, 2, W + 1, time_limit=LIMIT)
    inst.close()


def test_more_workgroups_than_the_device_holds_at_once(eng, ctx):
    """n = 640, W = 9, G = 16: 71 * 16 = 1 136 workgroups of one launch on 1 024 slots; the result does not depend on residency"""
    n = 640
    xy = rand_instance(n, seed=n, hi=100000)
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    inst.knn_build(5)
    nbr = inst.knn()
    start = np.asarray(O.greedy(xy, O.EUC_2D)[1], dtype=np.int32)
    st = _compare(inst, D, nbr, start, 1, 16, 9, 8, 1, seed=9)
    inst.close()
    assert st["windows"] * st["groups"] == 1136 == st["trials"] and st["commits"] > 0


# ---- 6. chains, prefixes, the time limit, two runs --------------------------------------------------------------------------------------------

def test_chains_of_a_batch_are_single_calls_with_their_streams(kro, kro_repaired):
    D, inst, nbr, _ = kro
    start = kro_repaired
    rc, S, Ob, St = inst.seg_ils_groups(np.stack([start] * 3), 2, 3, 25, 10, 2, seed=11, time_limit=LIMIT)
    assert rc == 0
    for b in range(3):
        _same(S[b], Ob[b], St[b], *SG.run(D, start, nbr, 7, 11, b, 2, 3, 25, 10, 2))
    assert len({tuple(s) for s in S}) > 1                    # the streams differ
    rc, s, o, st = inst.seg_ils_groups(start, 2, 3, 25, 10, 2, seed=11, time_limit=LIMIT)      # alone, it is stream 0
    assert (s == S[0]).all() and o == Ob[0] and all(st[k] == St[0][k] for k in STATS)


def test_a_time_limited_run_is_the_prefix_of_its_iterations_and_two_runs_return_the_same_bits(eng, ctx):
    n = 2000
    xy = rand_instance(n)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    inst.knn_build(5)
    start = np.asarray(O.greedy(xy, O.EUC_2D)[1], dtype=np.int32)
    rc, s, o, st = inst.seg_ils_groups(start, 10 ** 9, 8, 64, 50, 2, seed=3, time_limit=0.3)
    assert rc == eng.TIME_LIMIT_EXCEEDED
    assert O.is_tour(s) and o == O.succ_cost(xy, O.EUC_2D, s) and o < st["start_cost"] and st["iterations"] > 0
    assert st["groups"] == 8 and st["trials"] == st["iterations"] * 31 * 8 * 2 and 0 < st["commits"] < st["offers"]
    for _ in range(2):
        rc2, s2, o2, st2 = inst.seg_ils_groups(start, st["iterations"], 8, 64, 50, 2, seed=3, time_limit=LIMIT)
        assert rc2 == 0 and (s2 == s).all() and o2 == o
        assert all(st2[k] == st[k] for k in STATS + ("deltas_executed",))
    inst.close()


# ---- 7. against the older entry points -----------------------------------------------------------------------------------------------------

def test_one_group_returns_the_bits_of_seg_ils3_and_of_seg_ils(eng, ctx):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "pr299")
    start = np.asarray(O.greedy(xy, wt)[1], dtype=np.int32)
    shared3 = S3.COUNTERS + ("start_cost", "deltas_executed")
    for kinds in (1, 2, 3, 4, 7):
        rc3, s3, o3, st3 = inst.seg_ils3(start, 4, 64, 50, 2, seed=3, kinds=kinds, time_limit=LIMIT)
        rcg, sg, og, stg = inst.seg_ils_groups(start, 4, 1, 64, 50, 2, seed=3, kinds=kinds, time_limit=LIMIT)
        assert rc3 == rcg == 0 and (sg == s3).all() and og == o3 and st3["moves"] > 0
        assert all(stg[k] == st3[k] for k in shared3)
        assert stg["groups"] == 1 and 0 < stg["offers"] == stg["commits"] <= stg["accepted"]
        if kinds <= 3:
            rc, s, o, st = inst.seg_ils(start, 4, 64, 50, 2, seed=3, kinds=kinds, time_limit=LIMIT)
            assert rc == 0 and (sg == s).all() and og == o
            assert all(stg[k] == st[k] for k in SR.COUNTERS + ("start_cost", "deltas_executed"))
    inst.close()


# ---- 8. bad arguments ------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_leave_the_tours_alone_and_the_handle_usable(eng, ctx):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "att48")
    n = len(xy)
    start = random_tour(n, np.random.default_rng(4))
    L = eng.lib()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    # (kinds, groups, iterations, window, span, trials)
    bad = [(7, 65, 5, 12, 0, 1), (7, 1000, 5, 12, 0, 1), (7, 2 ** 31 - 1, 5, 12, 0, 1)]
    bad += [(0, 2, 5, 12, 0, 1), (8, 2, 5, 12, 0, 1), (15, 2, 5, 12, 0, 1), (-1, 2, 5, 12, 0, 1), (7, 2, -1, 12, 0, 1), (7, 2, 5, 12, 0, 0)]
    bad += [(7, 2, 5, w, 0, 1) for w in (1, 8, n, n + 5, SR.MAX_WINDOW + 1)]
    bad += [(4, 2, 5, 12, sp, 1) for sp in (1, 7, 12, 40)] + [(4, 2, 5, 0, 47, 1)]
    for kinds, groups, iters, window, span, trials in bad:
        succ, obj = start.copy(), np.zeros(1)
        st = eng.SegIlsGroupsStats()
        rc = L.tsp_dev_seg_ils_groups(inst._h, kinds, groups, 1, succ.ctypes.data_as(ip), 1, n, obj.ctypes.data_as(dp), 1, iters, window,
                                      span, trials, -1, LIMIT, C.byref(st))
        assert rc == eng.E_ARG and (succ == start).all(), (kinds, groups, iters, window, span, trials)
    # the same handle, after them
    _compare(inst, D, nbr, start, 1, 2, 12, 8, 1, seed=2, kinds=4)
    broken = start.copy()
    broken[0] = broken[1]
    with pytest.raises(eng.TspDeviceError, match="-4"):
        inst.seg_ils_groups(broken, 3, 2, 12, time_limit=LIMIT)
    # the limits themselves are arguments: W = n - 1 with S = W - 1, W = 9 with S = 8, 64 groups
    _compare(inst, D, nbr, start, 1, 2, n - 1, n - 2, 1, seed=2, cap=3)
    _compare(inst, D, nbr, start, 1, 64, 9, 8, 1, seed=2, cap=3)
    inst.close()


def test_no_iterations_and_no_window_return_the_tour(eng, ctx):
    xy, wt, D, inst, nbr = _setup(eng, ctx, "att48")
    start = random_tour(48, np.random.default_rng(1))
    rc, s, o, st = inst.seg_ils_groups(start, 0, 5, 12, time_limit=LIMIT)
    assert rc == 0 and (s == start).all() and o == st["start_cost"] == O.succ_cost(xy, wt, start)
    assert st["iterations"] == st["trials"] == st["offers"] == st["commits"] == 0 and st["windows"] == 4 and st["groups"] == 5
    inst.close()
    n = 9
    xy = rand_instance(n, seed=n, hi=100)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    start = random_tour(n, np.random.default_rng(n))
    for groups, G in ((0, 1), (3, 3)):
        rc, s, o, st = inst.seg_ils_groups(start, 7, groups, time_limit=LIMIT)
        assert rc == 0 and (s == start).all() and o == st["start_cost"] == O.succ_cost(xy, O.EUC_2D, start)
        assert st["iterations"] == st["trials"] == st["windows"] == 0 and st["groups"] == G
    inst.close()


# ---- 9. the host library ----------------------------------------------------------------------------------------------------------------------

def test_alg_seg_ils_under_the_groups_setting_is_the_device_call(eng, ctx):
    from tsp_optimization_amd.build import lib_path
    K, I, W, S, T = 5, 3, 64, 50, 2
    xy, wt = load_instance("pr299")
    inst = eng.Instance(ctx, xy, wt, 1)
    succ, obj = inst.greedy_edge()
    inst.knn_build(K)
    rc, s1, o1, _ = inst.nl_3opt_batch(succ, obj, kinds=7, time_limit=LIMIT)
    assert rc == 0
    rc, s3, o3, st3 = inst.seg_ils3(s1, I, W, S, T, seed=123, kinds=7, time_limit=LIMIT)
    rc4, s4, o4, st4 = inst.seg_ils_groups(s1, I, 4, W, S, T, seed=123, kinds=7, time_limit=LIMIT)
    rc0, s0, o0, st0 = inst.seg_ils_groups(s1, I, 0, W, S, T, seed=123, kinds=7, time_limit=LIMIT)
    assert rc == rc4 == rc0 == 0 and st4["groups"] == 4 and st0["groups"] == 64 and st4["commits"] > 0
    inst.close()
    L = C.CDLL(lib_path("libtsp_host.so"))
    L.alg_seg_ils.argtypes = [C.POINTER(Instance)]
    L.tsp_host_last_seg_ils3_stats.argtypes = [C.POINTER(eng.SegIls3Stats)]
    L.tsp_host_last_seg_ils_groups_stats.argtypes = [C.POINTER(eng.SegIlsGroupsStats)]
    try:
        assert L.tsp_host_set_seg_ils_groups(65) == eng.E_ARG and L.tsp_host_set_seg_ils_groups(-1) == eng.E_ARG
        assert L.tsp_host_set_alpha(0, 0) == 0 and L.tsp_host_set_knn(K) == 0 and L.tsp_host_set_seg_ils(I, W, S, T) == 0
        assert L.tsp_host_set_seg_ils_kinds(7) == 0
        for groups, (want_s, want_o, want_st) in ((None, (s3, o3, st3)), (4, (s4, o4, st4)), (0, (s0, o0, st0)), (1, (s3, o3, st3))):
            if groups is not None:                              # None: the default, which is today's calls
                assert L.tsp_host_set_seg_ils_groups(groups) == 0
            h = HostInstance("pr299")
            h.c.params.time_limit = int(LIMIT)
            h.c.params.seed = 123
            h.set_tour(s1, o1)
            assert L.alg_seg_ils(C.byref(h.c)) == 0
            assert (h.succ == want_s).all() and h.obj == want_o
            hs = eng.SegIlsGroupsStats()
            L.tsp_host_last_seg_ils_groups_stats(C.byref(hs))
            d = hs.as_dict()
            assert all(d[k] == want_st[k] for k in S3.COUNTERS + ("start_cost", "deltas_executed"))
            if groups in (4, 0):
                assert all(d[k] == want_st[k] for k in ("groups", "offers", "commits"))
            else:
                assert d["groups"] == d["offers"] == d["commits"] == 0
            h3 = eng.SegIls3Stats()
            L.tsp_host_last_seg_ils3_stats(C.byref(h3))
            assert all(v == d[k] for k, v in h3.as_dict().items())
    finally:
        L.tsp_host_set_seg_ils_groups(1)
        L.tsp_host_set_seg_ils_kinds(3)
        L.tsp_host_set_seg_ils(100, 0, 50, 1)
        L.tsp_host_set_knn(eng.NL_DEFAULT_K)
        L.tsp_host_shutdown()
