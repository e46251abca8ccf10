"""The list descent with the 3-opt kind on the device (tsp_dev_nl_3opt) against the CPU reference of the definition in
include/tsp_hip.h (tests/nl3_opt_ref.py): with K = n - 1 decision by decision against the brute force over all triples, on
att48 / kroA100 / pr299 to the end of the descent against the walk over the list entries, wrapping segments, every type, ties,
batches, caps, the masks, and HEU_greedy + alg_3opt of the host library."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import nl3_opt_ref as N3
import nl_opt_ref as NL
from helpers import GOLDEN, HostInstance, Instance, load_instance, rand_instance, random_tour
from oracle import oracle as O

pytestmark = pytest.mark.gpu

COUNTERS = ("decisions", "moves", "moves_2opt", "moves_oropt", "moves_by_len", "moves_reversed", "reversed", "moves_3opt",
            "moves_by_type")
METRICS = ("EUC_2D", "MAX_2D", "MAN_2D", "CEIL_2D", "GEO", "ATT")


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


def _run(inst, succ, **kw):
    kw.setdefault("time_limit", 300.0)     # a descent that does not end is a failure, not a hang
    return inst.nl_3opt(succ, **kw)


def _same(dev_succ, dev_obj, dev_st, ref_succ, ref_c, D):
    assert O.is_tour(dev_succ)
    assert (dev_succ == np.asarray(ref_succ)).all(), "tour differs from the reference"
    n = len(dev_succ)
    ref_obj = float(np.sum(D[np.arange(n), np.asarray(ref_succ)]))
    assert dev_obj == ref_obj or abs(dev_obj - ref_obj) <= 1e-9 * abs(ref_obj), (dev_obj, ref_obj)
    for k in COUNTERS:
        assert dev_st[k] == ref_c[k], (k, dev_st[k], ref_c[k])


def _matrix(inst, xy, wt, ic):
    """the reference's distances; GEO from the device's own matrix, as tests/test_gpu_nl_opt.py does"""
    return inst.dist_matrix()[0] if wt == O.GEO else O.dist_matrix(xy, wt, ic)


# ---- 1. K = n - 1: full 3-opt, decision by decision -------------------------------------------------------------------------------

@pytest.mark.parametrize("ic", [1, 0])
@pytest.mark.parametrize("metric", METRICS)
def test_full_lists_follow_the_brute_force_decision_by_decision(eng, ctx, metric, ic):
    wt = getattr(O, metric)
    seen = [0, 0, 0, 0]
    for n in (5, 6, 7, 9):
        rng = np.random.default_rng(n * 16 + wt * 2 + ic)
        xy = rng.uniform(0, 80, size=(n, 2)) if wt == O.GEO else np.round(rng.uniform(0, 300, size=(n, 2)), 1)
        inst = eng.Instance(ctx, xy, wt, ic)
        D = _matrix(inst, xy, wt, ic)
        inst.knn_build(n - 1)
        nbr = inst.knn()
        start = random_tour(n, rng)
        for kinds in range(1, 8):
            s, c, ended = start, N3.new_counters(), False
            for step in range(60):           # integer_cost = 0: a descent need not end (deltas of -1e-15)
                want = N3.decide(D, s, nbr, kinds)
                rc, got, o, st = _run(inst, s, kinds=kinds, max_moves=1)
                assert rc == 0 and st["decisions"] == 1
                if want is None:
                    assert st["moves"] == 0 and (got == s).all()
                    ended = True
                    break
                s = N3.apply_decision(s, want, c)
                assert (got == s).all(), (n, kinds, step, want)
            assert ended or ic == 0
            c["decisions"] = c["moves"] + (1 if ended else 0)
            rc, got, o, st = _run(inst, start, kinds=kinds, max_moves=-1 if ended else c["moves"])
            assert rc == 0
            _same(got, o, st, s, c, D)
            seen = [a + b for a, b in zip(seen, st["moves_by_type"])]
        inst.close()
    assert sum(seen) > 0


def test_fewer_than_five_nodes_have_no_move_of_the_kind(eng, ctx):
    for n in (3, 4):
        xy = rand_instance(n, seed=n, hi=100)
        inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
        for succ in (random_tour(n, np.random.default_rng(q)) for q in range(3)):
            rc, s, o, st = _run(inst, succ, kinds=eng.NL_3OPT)
            assert rc == 0 and (s == succ).all() and st["moves"] == 0 and st["decisions"] == 0
            assert o == O.succ_cost(xy, O.EUC_2D, succ)
            rc, s, o, st = _run(inst, succ, kinds=6)
            assert rc == 0 and (s == succ).all() and st["moves"] == 0
            rc, s, o, st = _run(inst, succ, kinds=7)          # four nodes have 2-opt moves: tsp_dev_nl_opt's
            rc1, s1, o1, st1 = inst.nl_opt(succ, kinds=1)
            assert rc == 0 and (s == s1).all() and o == o1 and st["moves"] == st1["moves"] and st["moves_3opt"] == 0
        inst.close()


# ---- 2. descents to their end against the walk over the list entries ------------------------------------------------------------

@pytest.mark.parametrize("name", ["att48", "kroA100"])
def test_descents_equal_the_sparse_reference(eng, ctx, name):
    xy, wt = load_instance(name)
    n = len(xy)
    D = O.dist_matrix(xy, wt, 1)
    inst = eng.Instance(ctx, xy, wt, 1)
    types = np.zeros(4, dtype=np.int64)
    for K in (1, 5, 10, 16):
        inst.knn_build(K)
        nbr = inst.knn()
        assert (nbr == NL.knn(D, K)).all()
        for start in (O.greedy(xy, wt)[1], random_tour(n, np.random.default_rng(K))):
            ref, c = N3.descent(D, start, nbr, 7)
            rc, s, o, st = _run(inst, start)
            assert rc == 0 and st["decisions"] == st["moves"] + 1
            _same(s, o, st, ref, c, D)
            assert o == O.succ_cost(xy, wt, s) and st["deltas_executed"] > 0
            assert N3.decide_sparse(D, s, nbr, 7) is None
            types += np.array(st["moves_by_type"])
    inst.close()
    assert (types > 0).all(), types          # every type was applied somewhere


def test_pr299_equals_the_recorded_descents(eng, ctx):
    """K = 5 alpha lists and K = 10 nearest-neighbour lists, kinds 4 and 7, greedy and random start, to the end; recorded by
    tests/golden/make_golden_nl3.py."""
    sys.path.insert(0, GOLDEN)
    import make_golden_nl3 as G
    with open(os.path.join(GOLDEN, "nl3_descents.json")) as f:
        rec = json.load(f)
    xy, wt = load_instance(G.NAME)
    D = O.dist_matrix(xy, wt, 1)
    inst = eng.Instance(ctx, xy, wt, 1)
    types = np.zeros(4, dtype=np.int64)
    for lists, K in G.LISTS:
        nbr = inst.alpha_build(K) if lists == "alpha" else (inst.knn_build(K), inst.knn())[1]
        assert (nbr == np.array(rec["lists"]["%s|%d" % (lists, K)])).all()
        for kinds in G.KINDS:
            for start in ("greedy", "random"):
                ref = rec["cases"][G.case_key(lists, K, kinds, start)]
                rc, s, o, st = _run(inst, G.start_tour(kinds, K, start), kinds=kinds)
                assert rc == 0
                _same(s, o, st, ref["succ"], ref["counters"], D)
                assert o == ref["cost"]
                types += np.array(st["moves_by_type"])
    inst.close()
    assert (types > 0).all(), types


# ---- 3. segments that wrap past position n - 1, ties -------------------------------------------------------------------------------

def test_wrapping_segments_of_every_type(eng, ctx):
    """order / pos start at node 0, so a segment that holds node 0 behind its first node wraps.  Random instances of 10 nodes
    are searched on the CPU until, for every type, a first decision has been seen whose S1 wraps, one whose S2 wraps and one
    whose S1 + S2 wraps at the joint of the two."""
    n = 10
    need = {(T, w) for T in range(4) for w in ("S1", "S2", "joint")}
    cases = []
    for seed in range(4000):
        if not need:
            break
        rng = np.random.default_rng(seed)
        xy = rng.integers(0, 100, size=(n, 2)).astype(np.float64)
        succ = random_tour(n, rng)
        D = O.dist_matrix(xy, O.EUC_2D, 1)
        d = N3.decide3(D, succ, NL.knn(D, n - 1))
        if d is None:
            continue
        a, b, c, T = N3.decode(d[2], n)
        pos = np.empty(n, dtype=np.int64)
        pos[NL.R.tour_order(succ)] = np.arange(n)
        pa1, pb, pb1, pc = pos[succ[a]], pos[b], pos[succ[b]], pos[c]
        w = "S1" if pa1 > pb else ("S2" if pb1 > pc else ("joint" if pb1 == 0 else None))
        if (T, w) in need:
            need.discard((T, w))
            cases.append((xy, succ, D, d))
    assert not need, need
    for xy, succ, D, d in cases:
        inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
        inst.knn_build(n - 1)
        rc, s, o, st = _run(inst, succ, kinds=eng.NL_3OPT, max_moves=1)
        c = N3.new_counters()
        c["decisions"] = 1
        _same(s, o, st, N3.apply_decision(succ, d, c), c, D)
        # and the whole descent from there, the order as the move left it
        ref, c = N3.descent(D, succ, inst.knn(), 7, sparse=False)
        rc, s, o, st = _run(inst, succ)
        _same(s, o, st, ref, c, D)
        inst.close()


def test_ties_on_an_integer_grid_are_decided_by_the_key(eng, ctx):
    g = np.array([(x, y) for x in range(5) for y in range(4)], dtype=np.float64) * 10.0     # 20 nodes, many equal deltas
    D = O.dist_matrix(g, O.MAN_2D, 1)
    inst = eng.Instance(ctx, g, O.MAN_2D, 1)
    tied = 0
    for K in (4, 16):
        inst.knn_build(K)
        nbr = inst.knn()
        for seed in range(4):
            succ = random_tour(len(g), np.random.default_rng(seed))
            delta, key = N3.moves(D, succ, nbr)
            tied += int((delta == delta.min()).sum() > 1)
            for kinds in (4, 7):
                ref, c = N3.descent(D, succ, nbr, kinds)
                rc, s, o, st = _run(inst, succ, kinds=kinds)
                assert rc == 0
                _same(s, o, st, ref, c, D)
    inst.close()
    assert tied > 0


# ---- 4. batches, caps, masks, determinism -------------------------------------------------------------------------------------

def test_batch_of_three_descents_of_different_length_and_caps(eng, ctx):
    xy, wt = load_instance("kroA100")
    n = len(xy)
    D = O.dist_matrix(xy, wt, 1)
    inst = eng.Instance(ctx, xy, wt, 1)
    inst.knn_build(5)
    nbr = inst.knn()
    greedy = O.greedy(xy, wt)[1]
    done = _run(inst, greedy)[1]                                  # a local optimum: a descent of no move
    starts = np.stack([done, greedy, random_tour(n, np.random.default_rng(2))])
    for cap in (-1, 0, 1, 7):
        rc, S, Ob, St = _run(inst, starts, max_moves=cap)
        assert rc == 0
        for q in range(3):
            ref, c = N3.descent(D, starts[q], nbr, 7, max_moves=cap)
            _same(S[q], Ob[q], St[q], ref, c, D)
        if cap < 0:
            assert St[0]["moves"] == 0 < St[1]["moves"] < St[2]["moves"]
        elif cap > 0:
            assert St[1]["moves"] == St[2]["moves"] == cap == St[2]["decisions"]
    inst.close()


def test_low_kinds_equal_nl_opt_and_two_runs_return_the_same_bits(eng, ctx):
    xy, wt = load_instance("pr299")
    succ = random_tour(len(xy), np.random.default_rng(5))
    for ic in (1, 0):
        inst = eng.Instance(ctx, xy, wt, ic)
        inst.knn_build(8)
        for kinds in (1, 2, 3):
            rc, s, o, st = _run(inst, succ, kinds=kinds, max_moves=150)
            rc0, s0, o0, st0 = inst.nl_opt(succ, kinds=kinds, max_moves=150)
            assert rc == rc0 == 0 and (s == s0).all() and o == o0 and st["moves_3opt"] == 0
            for k in st0:
                if k not in ("seconds", "device_ms"):
                    assert st[k] == st0[k], k
        r1 = _run(inst, succ, max_moves=150)
        r2 = _run(inst, succ, max_moves=150)
        assert (r1[1] == r2[1]).all() and np.float64(r1[2]).tobytes() == np.float64(r2[2]).tobytes()
        assert all(r1[3][k] == r2[3][k] for k in COUNTERS + ("deltas_executed",)) and r1[3]["moves_3opt"] > 0
        inst.close()


def test_bad_masks_and_bad_tours(eng, ctx):
    n = 50
    xy = rand_instance(n, seed=50)
    inst = eng.Instance(ctx, xy, O.EUC_2D, 1)
    succ = random_tour(n, np.random.default_rng(0))
    for kinds in (0, 8, -1):
        with pytest.raises(eng.TspDeviceError, match="-3"):
            inst.nl_3opt(succ, kinds=kinds)
    with pytest.raises(eng.TspDeviceError, match="-3"):
        inst.nl_opt(succ, kinds=eng.NL_3OPT)                      # the old entry point keeps refusing the new kind
    bad = succ.copy()
    bad[0] = bad[1]
    with pytest.raises(eng.TspDeviceError, match="-4"):
        inst.nl_3opt(bad)
    assert inst.knn() is None
    rc, s, o, st = _run(inst, succ)                               # the default lists are built on first use
    D = O.dist_matrix(xy, O.EUC_2D, 1)
    assert (inst.knn() == NL.knn(D, eng.NL_DEFAULT_K)).all()
    ref, c = N3.descent(D, succ, inst.knn(), 7)
    _same(s, o, st, ref, c, D)
    inst.close()


# ---- 5. the host library -------------------------------------------------------------------------------------------------------

def test_greedy_then_alg_3opt_ends_in_a_tour_no_move_improves(eng, ctx):
    from tsp_optimization_amd.build import lib_path
    L = C.CDLL(lib_path("libtsp_host.so"))
    for f in ("alg_3opt", "HEU_greedy"):
        getattr(L, f).argtypes = [C.POINTER(Instance)]
    L.tsp_host_set_knn.argtypes = [C.c_int]
    L.tsp_host_set_alpha.argtypes = [C.c_int, C.c_int]
    L.tsp_host_last_nl3_stats.argtypes = [C.POINTER(eng.Nl3OptStats)]
    try:
        h = HostInstance("kroA100")
        D = O.dist_matrix(h.xy, h.wt, 1)
        assert L.tsp_host_set_alpha(0, 0) == 0 and L.tsp_host_set_knn(6) == 0
        assert L.HEU_greedy(C.byref(h.c)) == 0 and L.alg_3opt(C.byref(h.c)) == 0
        hs = eng.Nl3OptStats()
        L.tsp_host_last_nl3_stats(C.byref(hs))
        st = hs.as_dict()
        nbr = NL.knn(D, 6)
        ref, c = N3.descent(D, O.greedy(h.xy, h.wt)[1], nbr, 7)
        _same(h.succ, h.obj, st, ref, c, D)
        assert st["moves_3opt"] > 0 and N3.decide(D, h.succ, nbr, 7) is None
        # over alpha lists: alg_3opt on the greedy tour equals the device API
        assert L.tsp_host_set_alpha(5, 0) == 0
        assert L.HEU_greedy(C.byref(h.c)) == 0
        start = h.succ
        assert L.alg_3opt(C.byref(h.c)) == 0
        inst = eng.Instance(ctx, h.xy, h.wt, 1)
        inst.alpha_build(5)
        rc, s, o, _ = _run(inst, start)
        assert rc == 0 and (h.succ == s).all() and h.obj == o
        inst.close()
    finally:
        L.tsp_host_set_alpha(0, 0)
        L.tsp_host_set_knn(eng.NL_DEFAULT_K)
        L.tsp_host_shutdown()
