"""CPU (no GPU): the two greedy-edge references (tests/greedy_edge_ref.py) against each other -- the sort-and-walk definition and
the round rule the device follows -- and the new C ABI in the headers, the libraries and the binding."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import greedy_edge_ref as G
from helpers import INSTANCES
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tsplib(name):
    xy, wt = O.parse_tsplib(os.path.join(INSTANCES, name + ".tsp"))
    return O.dist_matrix(xy, wt, 1)


def euc(xy, integer_cost=1):
    return O.dist_matrix(xy, O.EUC_2D, integer_cost)


CASES = {
    "berlin52": lambda: tsplib("berlin52"),
    "att48": lambda: tsplib("att48"),
    "burma14": lambda: tsplib("burma14"),
    "pr299": lambda: tsplib("pr299"),
    "grid30": lambda: euc(G.tie_grid(30, 4)),
    "grid400": lambda: euc(G.tie_grid(400, 20)),
    "grid400_f": lambda: euc(G.tie_grid(400, 20), 0),
    "collinear200": lambda: euc(G.collinear(200)),
    "coincident64": lambda: euc(G.coincident(64)),
    "n3": lambda: euc(G.small(3)),
    "n4": lambda: euc(G.small(4)),
    "n5": lambda: euc(G.small(5)),
}


@pytest.fixture(scope="module")
def results():
    """name -> (D, sort-and-walk result, round-rule result), each computed once"""
    out = {}
    for name, make in CASES.items():
        D = make()
        out[name] = (D, G.sort_and_walk(D), G.round_rule(D))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_the_round_rule_builds_the_edges_of_the_definition(results, name):
    D, (e1, s1, c1), (e2, s2, c2, info) = results[name]
    n = len(D)
    print("%s: n %d, %d rounds, %.2f n rows scanned, at most %d edges in a round" % (name, n, info["rounds"], info["rows_scanned"] / n,
                                                                                     max(info["edges_per_round"])))
    assert e1.shape == (n - 1, 2) and (e1 == e2).all()
    assert (s1 == s2).all() and c1 == c2
    assert min(info["edges_per_round"]) >= 1 and sum(info["edges_per_round"]) == n - 1
    assert 1 <= info["rounds"] <= n - 1 and info["rows_scanned"] >= n


@pytest.mark.parametrize("name", list(CASES))
def test_the_result_is_one_oriented_hamiltonian_cycle(results, name):
    D, (edges, succ, cost), _ = results[name]
    n = len(D)
    assert sorted(succ.tolist()) == list(range(n))
    seen, v = 0, 0
    for _ in range(n):
        v = int(succ[v])
        seen += 1
        if v == 0:
            break
    assert seen == n   # one cycle through every node
    pred0 = int(np.flatnonzero(succ == 0)[0])
    assert succ[0] <= pred0 and (n == 3 or succ[0] < pred0)
    # the n - 1 accepted edges are tour edges, sorted, lo < hi; the one tour edge that is not among them closes the path
    tour = {(min(v, int(succ[v])), max(v, int(succ[v]))) for v in range(n)}
    acc = [tuple(e) for e in edges.tolist()]
    assert acc == sorted(acc) and all(a < b for a, b in acc) and len(set(acc)) == n - 1 and set(acc) <= tour
    assert cost == sum(float(D[min(v, int(succ[v])), max(v, int(succ[v]))]) for v in range(n))


def test_the_collinear_points_take_one_edge_per_round(results):
    _, _, (_, succ, _, info) = results["collinear200"]
    assert info["rounds"] == 199 and set(info["edges_per_round"]) == {1}
    assert info["rows_scanned"] <= 4 * 200   # the stale-only rule: not rounds x n
    assert succ[0] == 1


# ---- the C ABI ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def _header(path):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, path)).read(), flags=re.S)


def test_the_new_symbols_are_declared_exported_and_bound(built):
    from tsp_optimization_amd import engine as E
    from tsp_optimization_amd.build import lib_path
    hip_h, host_h = _header("include/tsp_hip.h"), _header("include/tsp_host.h")
    L = C.CDLL(E.lib_path())
    assert re.search(r"\btsp_dev_greedy_edge\s*\(", hip_h)
    assert "tsp_dev_greedy_edge" in E.EXPORTED and hasattr(L, "tsp_dev_greedy_edge")
    assert sorted(set(re.findall(r"\b(tsp_dev_\w+)\s*\(", hip_h))) == sorted(E.EXPORTED)
    H = C.CDLL(lib_path("libtsp_host.so"))
    for sym in ("HEU_greedy_edge", "HEU_2opt_greedy_edge", "HEU_nl_greedy_edge", "HEU_ils_greedy_edge",
                "tsp_host_last_greedy_edge_stats"):
        assert re.search(r"\b%s\s*\(" % sym, host_h), sym
        assert hasattr(H, sym), sym
    m = re.search(r"typedef struct \{([^}]*)\}\s*tsp_greedy_edge_stats;", hip_h)
    names = re.findall(r"(\w+)\s*[;,]", m.group(1))
    assert names == [f for f, _ in E.GreedyEdgeStats._fields_]
    assert C.sizeof(E.GreedyEdgeStats) == 5 * 8 + 2 * 8
    assert hasattr(E.Instance, "greedy_edge")


def test_no_method_row_and_no_solver_type(built):
    from tsp_optimization_amd.build import lib_path
    r = subprocess.run([lib_path("tsp"), "--methods"], capture_output=True, text=True)
    rows = [ln.split()[0] for ln in r.stdout.splitlines() if ln.strip()]
    assert r.returncode == 0 and len(rows) == 20 and not [m for m in rows if "EDGE" in m]
    assert "GREEDY_EDGE" not in _header("include/tsp_host.h").split("solver_type;")[0]
