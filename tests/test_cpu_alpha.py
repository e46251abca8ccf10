"""CPU (no GPU): the alpha-nearness reference (tests/alpha_ref.py) against the plain definition -- alpha(i,j) = W(minimum 1-tree
forced to contain {i,j}) - W(T) -- and the new C ABI in the headers, the libraries and the binding."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import alpha_ref as AR
import held_karp_ref as HK
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tie_grid(n, seed=5):
    """n nodes on a 4 x 4 integer grid: masses of equal distances and coincident nodes"""
    return np.random.default_rng(seed).integers(0, 4, size=(n, 2)).astype(np.float64)


def cases():
    """(name, D, integer metric?)"""
    out = [("grid12", O.dist_matrix(tie_grid(12), O.EUC_2D, 1), True), ("grid9", O.dist_matrix(tie_grid(9, 8), O.MAN_2D, 1), True)]
    for n, seed in ((3, 4), (4, 5), (5, 6), (8, 1), (12, 2)):
        xy = np.random.default_rng(seed).integers(0, 50, size=(n, 2)).astype(np.float64)
        out.append(("rand%d" % n, O.dist_matrix(xy, O.EUC_2D, 1), True))
        out.append(("rand%d_f" % n, O.dist_matrix(xy, O.EUC_2D, 0), False))
    return out


def penalties(name, D, integer):
    """(pi, every weight an integer?)"""
    n = len(D)
    rng = np.random.default_rng(n + 100)
    scale = D[np.triu_indices(n, 1)].mean()
    return [(None, integer), (np.round(rng.uniform(-3, 3, n)), integer), (rng.uniform(-0.5, 0.5, n) * scale, False)]


def forced_one_tree_weight(Wm, i, j, special):
    """Sum of the weights of the minimum 1-tree that contains {i, j}, from the plain definition: for i, j >= 1 Kruskal over
    nodes 1 .. n-1 with the edge pre-inserted, plus the two special edges; for an edge at node 0 the spanning tree is untouched
    and {0, j} replaces the larger special edge unless it is one of them."""
    n = len(Wm)
    all_e = sorted((Wm[a, b], a, b) for a in range(1, n) for b in range(a + 1, n))
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    terms = []
    lo, hi = min(i, j), max(i, j)
    if lo >= 1:
        parent[find(lo)] = find(hi)
        terms.append(Wm[lo, hi])
    for w, a, b in all_e:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            terms.append(w)
    (w1, c1), (w2, c2) = special
    if lo >= 1 or hi in (c1, c2):
        terms += [w1, w2]
    else:
        terms += [w1, Wm[0, hi]]
    assert len(terms) == n
    return math.fsum(terms)


@pytest.mark.parametrize("name,D,integer", cases(), ids=[c[0] for c in cases()])
def test_alpha_is_the_growth_of_the_forced_one_tree(name, D, integer):
    """Bit for bit where every weight is an integer (the sums are exact).  Elsewhere: both sums are math.fsum, correctly
    rounded whatever their length (0.5 ulp each), the subtraction of the two adds 0.5 ulp of a result of at most twice the
    larger sum (1 ulp of it), and alpha itself is one rounded subtraction of the same kind (1 ulp of it): 3 ulp of the larger
    of |W(forced)| and |W(T)|; 4 are allowed."""
    n = len(D)
    for pi, exact in penalties(name, D, integer):
        A, Wt, edges = AR.alpha_rows(D, pi)
        tree = {(a, b) for a, b in edges.tolist()}
        assert len(tree) == n
        special = sorted((Wt[0, b], b) for a, b in tree if a == 0)
        WT = math.fsum(Wt[a, b] for a, b in tree)
        assert (A == A.T).all()                                   # symmetric
        assert (np.diag(A) == 0).all()
        off = ~np.eye(n, dtype=bool)
        assert (A[off] >= 0).all()
        for i in range(n):
            for j in range(i + 1, n):
                if (i, j) in tree:
                    assert A[i, j] == 0.0 and not np.signbit(A[i, j])
                    continue
                WF = forced_one_tree_weight(Wt, i, j, special)
                if exact:
                    assert A[i, j] == WF - WT, (name, i, j)
                else:
                    tol = 4 * np.spacing(max(abs(WF), abs(WT)))
                    assert abs(A[i, j] - (WF - WT)) <= tol, (name, i, j, A[i, j], WF - WT, tol)
        # alpha is zero exactly on the n tree edges wherever no two weights are equal (elsewhere an edge as heavy as the one it
        # would replace has alpha 0 too, by the definition); random real penalties leave no equal weights
        w = Wt[np.triu_indices(n, 1)]
        distinct = len(np.unique(w)) == len(w)
        if pi is not None and not exact:
            assert distinct
        if distinct:
            assert int((A[np.triu_indices(n, 1)] == 0).sum()) == n


@pytest.mark.parametrize("name,D,integer", cases(), ids=[c[0] for c in cases()])
def test_the_row_walk_equals_the_matrix_recurrence_and_lists_start_with_the_tree(name, D, integer):
    n = len(D)
    for pi, _ in penalties(name, D, integer):
        A, Wt, edges = AR.alpha_rows(D, pi)
        rows = np.arange(n)[::-1]
        A2, Wt2, _ = AR.alpha_rows(D, pi, rows)
        assert A2.tobytes() == A[rows].tobytes() and Wt2.tobytes() == Wt[rows].tobytes()
        K = min(5, n - 1)
        nbr, al = AR.lists(A, Wt, np.arange(n), K)
        for v in range(n):
            tn = sorted((Wt[v, b if a == v else a], b if a == v else a) for a, b in edges.tolist() if v in (a, b))
            k = min(K, len(tn))
            if len({w for w, _ in tn}) == len(tn) and (A[v] == 0).sum() == len(tn) + 1:   # no other alpha-0 node competes
                assert nbr[v][:k].tolist() == [u for _, u in tn[:k]]
            assert (al[v][:k] == 0).all() and len(set(nbr[v].tolist())) == K and v not in nbr[v]


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
    for sym in ("tsp_dev_inst_alpha_build", "tsp_dev_alpha_rows"):
        assert re.search(r"\b%s\s*\(" % sym, hip_h), sym
        assert sym in E.EXPORTED and hasattr(L, sym), sym
    assert sorted(set(re.findall(r"\b(tsp_dev_\w+)\s*\(", hip_h))) == sorted(E.EXPORTED)
    H = C.CDLL(lib_path("libtsp_host.so"))
    assert re.search(r"\btsp_host_set_alpha\s*\(\s*int\s+K\s*,\s*int\s+ascent_iters\s*\)", host_h) and hasattr(H, "tsp_host_set_alpha")
    assert re.search(r"#define\s+TSP_ALPHA_DEFAULT_K\s+5\b", hip_h) and E.ALPHA_DEFAULT_K == 5
    m = re.search(r"typedef struct \{([^}]*)\}\s*tsp_alpha_stats;", hip_h)
    names = re.findall(r"(\w+)\s*[;,]", m.group(1))
    assert names == [f for f, _ in E.AlphaStats._fields_] == ["trees", "rounds", "pairs_executed", "tree_value", "seconds", "device_ms"]
    assert C.sizeof(E.AlphaStats) == 6 * 8
    assert hasattr(E.Instance, "alpha_build") and hasattr(E.Instance, "alpha_rows")
    # the setter checks its arguments without a device
    H.tsp_host_set_alpha.argtypes = [C.c_int, C.c_int]
    for bad in ((-1, 0), (17, 0), (5, -1), (0, 3)):
        assert H.tsp_host_set_alpha(*bad) == E.E_ARG, bad
    assert H.tsp_host_set_alpha(5, 30) == 0 and H.tsp_host_set_alpha(0, 0) == 0
