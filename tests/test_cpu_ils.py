"""Iterated local search (extension): the tests' CPU reference (tests/ils_ref.py) against the definition in include/tsp_hip.h --
known answers of the random stream, the kick as a tour with exactly four new edges over sizes, windows and iterations, the
recorded chains of tests/golden/ils_runs.json -- and the new names of the C ABI.  No GPU needed."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import ils_ref as IR
import nl_opt_ref as NL
from helpers import GOLDEN, golden, load_instance, random_tour
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _edge_set(succ):
    return {frozenset((v, int(succ[v]))) for v in range(len(succ))}


def test_mix_is_the_splitmix64_step():
    # the first outputs of splitmix64 from state 0 (Vigna's reference implementation): mix of 0, g, 2g, 3g
    g = IR.GOLD
    want = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC)
    assert tuple(IR.mix((k * g) & IR.M64) for k in range(4)) == want
    assert IR.mix(IR.M64) == IR.mix(-1 & IR.M64) and 0 <= IR.mix(IR.M64) <= IR.M64


def test_draws_follow_the_definition():
    # seed 0, chain 0, iteration 0: u_j = mix(mix(mix(0)) + j); mix(0) is the vector above
    m1 = 0xE220A8397B1DCDAF
    base = IR.mix(IR.mix(0))
    assert IR.mix(0) == m1 and base == IR.mix(m1)
    assert IR.draws(0, 0, 0) == [IR.mix((base + j) & IR.M64) for j in range(5)]
    # the chain enters through b * 0x100000001B3 under the seed, the iteration by addition, both mod 2^64
    seed, b, it = 0xFFFFFFFFFFFFFFFF, 3, 5
    base = IR.mix((IR.mix(seed ^ (3 * 0x100000001B3)) + 5) & IR.M64)
    assert IR.draws(seed, b, it) == [IR.mix((base + j) & IR.M64) for j in range(5)]
    assert IR.draws(7, 3, 5) == [0x39D5F6D07151CA73, 0x266A4248A4FB0DE1, 0x177C0936297B73BB, 0xB3892D03E76D809C, 0xD4D3D7D8A0650AC8]
    seen = {tuple(IR.draws(7, b, it)) for b in range(4) for it in range(4)}
    assert len(seen) == 16


@pytest.mark.parametrize("n", range(8, 41))
def test_kick_is_a_tour_with_exactly_four_new_edges(n):
    rng = np.random.default_rng(n)
    wraps = full = four = 0
    for span in (0, 8, n):
        W = IR.window(n, span)
        for b in range(2):
            succ = random_tour(n, rng)
            order = NL.R.tour_order(succ)
            pos = np.empty(n, dtype=np.int64)
            pos[order] = np.arange(n)
            for it in range(48):
                s, o1, o2, o3, o4 = IR.cuts(n, span, IR.draws(n, b, it))
                assert 0 <= s < n and 1 <= o1 < o2 < o3 < o4 <= W
                wraps += int(pos[s] + o4 - 1 >= n)
                full += int(o4 == W)
                out = IR.kick(succ, n, b, it, span)
                assert O.is_tour(out)
                # exactly four successors change: those of the last nodes of P, Bk, Ck and Dk
                seq = [s]
                for _ in range(n - 1):
                    seq.append(int(succ[seq[-1]]))
                assert sorted(np.flatnonzero(out != succ)) == sorted(seq[o - 1] for o in (o1, o2, o3, o4)), (n, span, b, it)
                assert (out[seq[o1 - 1]], out[seq[o4 - 1]], out[seq[o3 - 1]], out[seq[o2 - 1]]) == \
                    (seq[o3], seq[o2], seq[o1], seq[o4 % n])
                # as undirected edges four leave and four enter, less one for every two single-node blocks that are neighbours
                # on the cycle R P | Bk | Ck | Dk (Bk = {x}, Ck = {y}: the edge x y leaves as (x, y) and enters as (y, x))
                one = [n - (o4 - o1) == 1, o2 - o1 == 1, o3 - o2 == 1, o4 - o3 == 1]
                same = sum(int(one[q] and one[(q + 1) % 4]) for q in range(4))
                old, new = _edge_set(succ), _edge_set(out)
                assert len(old - new) == len(new - old) == 4 - same, (n, span, b, it)
                four += int(same == 0)
    assert wraps > 0 and full > 0 and four > 0


def test_reference_reproduces_the_recorded_chains():
    rec = golden("ils_runs.json")["runs"]
    sys.path.insert(0, GOLDEN)
    import make_golden_ils as G
    ran = 0
    for r in rec:
        if r["name"] == "pr299" and r["chain"] != 1:     # one of the three pr299 chains: each takes about a second
            continue
        xy, wt = load_instance(r["name"])
        D = O.dist_matrix(xy, wt, 1)
        start = G.start_tour(r["name"], r["start"])
        succ, cost, st = IR.chain(D, start, NL.knn(D, r["K"]), r["kinds"], r["seed"], r["chain"], r["iterations"], r["span"])
        assert (succ == np.array(r["succ"])).all() and cost == r["cost"] and st == r["stats"]
        assert cost == O.succ_cost(xy, wt, succ) and cost <= st["start_cost"]
        assert (st["accepted"] == 0) == (st["last_improved"] == -1) and st["iterations"] == r["iterations"]
        ran += 1
    assert ran >= 2
    runs = [(r["name"], r["K"], r["start"], r["seed"], r["chain"], r["iterations"], r["span"], r["kinds"]) for r in rec]
    assert runs == G.RUNS


def test_chain_without_iterations_is_the_descent_and_small_n_has_no_kick():
    import nl3_opt_ref as N3
    xy, wt = load_instance("att48")
    D = O.dist_matrix(xy, wt, 1)
    nbr = NL.knn(D, 5)
    start = random_tour(len(xy), np.random.default_rng(3))
    ref, c = N3.descent(D, start, nbr, 7)
    s, cost, st = IR.chain(D, start, nbr, 7, 1, 0, 0)
    assert (s == ref).all() and st["iterations"] == 0 and st["last_improved"] == -1 and cost == st["start_cost"] == IR.cost(D, ref)
    assert all(st[k] == c[k] for k in IR.NL_COUNTERS)
    for n in (5, 6, 7):
        Dn = D[:n, :n]
        start = random_tour(n, np.random.default_rng(n))
        s, cost, st = IR.chain(Dn, start, NL.knn(Dn, n - 1), 7, 1, 0, 20)
        assert st["iterations"] == 0 and (s == N3.descent(Dn, start, NL.knn(Dn, n - 1), 7)[0]).all()


def test_headers_library_and_python_declare_the_new_entry_points():
    hip = open(os.path.join(ROOT, "include", "tsp_hip.h")).read()
    assert re.search(r"int\s+tsp_dev_ils\s*\(", hip) and re.search(r"int\s+tsp_dev_ils_kick\s*\(", hip)
    assert re.search(r"\}\s*tsp_ils_stats\s*;", hip)
    for word in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x100000001B3", "modulo bias"):
        assert word in hip, word
    host = open(os.path.join(ROOT, "include", "tsp_host.h")).read()
    for name in ("tsp_host_set_ils", "alg_ils", "HEU_ils_greedy", "tsp_host_last_ils_stats"):
        assert re.search(r"\b%s\s*\(" % name, host), name
    from tsp_optimization_amd import engine as E
    from tsp_optimization_amd.build import lib_path
    for name in ("tsp_dev_ils", "tsp_dev_ils_kick"):
        assert name in E.EXPORTED and hasattr(E.lib(), name), name
    assert hasattr(E.Instance, "ils") and hasattr(E.Instance, "ils_kick")
    old = [f for f, _ in E.Nl3OptStats._fields_]
    new = [f for f, _ in E.IlsStats._fields_]
    assert new[:len(old)] == old and new[len(old):] == ["iterations", "accepted", "last_improved", "start_cost"]
    H = C.CDLL(lib_path("libtsp_host.so"))
    for name in ("tsp_host_set_ils", "alg_ils", "HEU_ils_greedy", "tsp_host_last_ils_stats"):
        assert hasattr(H, name), name
    # the settings are checked before anything touches a device
    assert H.tsp_host_set_ils(-1, 0, 1) == E.E_ARG and H.tsp_host_set_ils(5, 7, 1) == E.E_ARG and H.tsp_host_set_ils(5, 0, 0) == E.E_ARG
    assert H.tsp_host_set_ils(100, 50, 1) == 0
