"""CPU references of the greedy-edge section of include/tsp_hip.h, numpy fp64 (restated here on purpose):

  d(i,j) with the lower node id first; edge order: lexicographic on (d, lo, hi) -- strict
  greedy edge (n >= 3): the edges are walked in that order; {u,v} is accepted iff both nodes have degree < 2 and they are not
  the two ends of one fragment; after n - 1 accepted edges the path is closed by the edge between its two ends
  output: the n - 1 accepted edges as (lo, hi) sorted; succ oriented so that succ[0] is the smaller of node 0's two tour
  neighbours; cost = the sum over nodes in node order of d(v, succ v)

Two constructions of the same edge set:
  sort_and_walk  the definition: every edge sorted, one walk
  round_rule     what the device does: per round every free node whose cached smallest valid edge is missing or
                 no longer valid is scanned again (one vectorised row scan each), and edge e = {u,v} is accepted iff
                 best(F_u) = e = best(F_v), best(F) being the smaller of the bests of F's one or two ends

`D` is the oracle's distance matrix, or any object with `n` and `row(t)` = d(min(t,u), max(t,u)) for every u
(held_karp_ref.Matrix, held_karp_ref.Euc2DRows)."""
import numpy as np

from held_karp_ref import Matrix


def _rows(D):
    return D if hasattr(D, "row") else Matrix(D)


def finish(R, adj):
    """adj: per node the list of its one or two path neighbours -> (edges [n-1,2] sorted, succ [n], cost)"""
    n = R.n
    edges = sorted((v, w) for v in range(n) for w in adj[v] if v < w)
    assert len(edges) == n - 1
    ends = [v for v in range(n) if len(adj[v]) == 1]
    assert len(ends) == 2 and all(1 <= len(a) <= 2 for a in adj)
    nb = [list(a) for a in adj]
    nb[ends[0]].append(ends[1])
    nb[ends[1]].append(ends[0])
    succ = np.full(n, -1, dtype=np.int32)
    prev, v = 0, min(nb[0])
    succ[0] = v
    while v != 0:
        a, b = nb[v]
        nx = b if a == prev else a
        assert succ[v] < 0, "the accepted edges closed a cycle"
        succ[v] = nx
        prev, v = v, nx
    assert (succ >= 0).all(), "the accepted edges are not one path"
    cost = 0.0
    for v in range(n):
        s = int(succ[v])
        cost += float(R.row(min(v, s))[max(v, s)])
    return np.array(edges, dtype=np.int32).reshape(-1, 2), succ, cost


def sort_and_walk(D):
    """The definition -> (edges, succ, cost)"""
    R = _rows(D)
    n = R.n
    assert n >= 3
    # the upper triangle in (lo, hi) order; a stable sort by d alone is then the order (d, lo, hi)
    d = np.concatenate([R.row(lo)[lo + 1:] for lo in range(n - 1)])
    lo_of = np.repeat(np.arange(n - 1), np.arange(n - 1, 0, -1))
    first = np.concatenate(([0], np.cumsum(np.arange(n - 1, 0, -1))[:-1]))
    hi_of = np.arange(len(d)) - first[lo_of] + lo_of + 1
    order = np.argsort(d, kind="stable")
    deg = np.zeros(n, dtype=np.int64)
    other = np.arange(n)
    adj = [[] for _ in range(n)]
    left = n - 1
    for at in range(0, len(order), 4096):
        blk = order[at:at + 4096]
        lo, hi = lo_of[blk], hi_of[blk]
        keep = (deg[lo] < 2) & (deg[hi] < 2)   # degrees only grow: what fails here fails in the walk too
        for u, v in zip(lo[keep].tolist(), hi[keep].tolist()):
            if deg[u] < 2 and deg[v] < 2 and other[u] != v:
                eu, ev = other[u], other[v]
                other[eu], other[ev] = ev, eu
                deg[u] += 1
                deg[v] += 1
                adj[u].append(v)
                adj[v].append(u)
                left -= 1
        if left == 0:
            break
    return finish(R, adj)


def round_rule(D):
    """The device's rounds -> (edges, succ, cost, info); info: rounds, rows_scanned, edges_per_round."""
    R = _rows(D)
    n = R.n
    assert n >= 3
    deg = np.zeros(n, dtype=np.int64)
    other = np.arange(n)
    bw = np.full(n, np.inf)
    bo = np.full(n, -1, dtype=np.int64)
    adj = [[] for _ in range(n)]
    stale = np.arange(n)
    rows_scanned, per_round, have = 0, [], 0
    while have < n - 1:
        free = deg < 2
        for u in stale.tolist():
            dd = np.where(free, R.row(u), np.inf)
            dd[u] = np.inf
            dd[other[u]] = np.inf
            c = int(dd.argmin())   # the first minimum: within a row (lo, hi) grows with the column
            bw[u], bo[u] = (dd[c], c) if dd[c] < np.inf else (np.inf, -1)
        rows_scanned += len(stale)
        u = np.flatnonzero(free & (bo >= 0))
        u = u[bo[bo[u]] == u]
        v = bo[u]

        def smaller_than_far_end(a, b):
            """edge {a, b} = best[a] is before best[other[a]] (or a's fragment is a alone)"""
            oa = other[a]
            ob = np.where(bo[oa] >= 0, bo[oa], oa)
            lo1, hi1, lo2, hi2 = np.minimum(a, b), np.maximum(a, b), np.minimum(oa, ob), np.maximum(oa, ob)
            lt = (bw[a] < bw[oa]) | ((bw[a] == bw[oa]) & ((lo1 < lo2) | ((lo1 == lo2) & (hi1 < hi2))))
            return (oa == a) | (bo[oa] < 0) | lt

        ok = smaller_than_far_end(u, v) & smaller_than_far_end(v, u)
        joins = [(int(a), int(b)) for a, b in zip(u[ok], v[ok]) if a < b]
        ends = [(int(other[a]), int(other[b])) for a, b in joins]
        for (a, b), (ea, eb) in zip(joins, ends):
            other[ea], other[eb] = eb, ea
            deg[a] += 1
            deg[b] += 1
            adj[a].append(b)
            adj[b].append(a)
        per_round.append(len(joins))
        have += len(joins)
        if not joins:
            break   # (never: the smallest valid edge always qualifies; the caller's assertion reports it)
        free = deg < 2
        stale = np.flatnonzero(free & ((bo < 0) | (deg[np.maximum(bo, 0)] >= 2) | (bo == other)))
    info = {"rounds": len(per_round), "rows_scanned": rows_scanned, "edges_per_round": per_round}
    return finish(R, adj) + (info,)


# ---- inputs both test files use ----------------------------------------------------------------------------------------------

def tie_grid(n, side, seed=5):
    """n nodes with integer coordinates in [0, side)^2: masses of equal distances and coincident nodes"""
    return np.random.default_rng(seed).integers(0, side, size=(n, 2)).astype(np.float64)


def collinear(n=200, step=10.0):
    """n equally spaced points on a line: every edge of the path has the same length and the order (d, lo, hi) lets exactly one
    of them qualify per round -- n - 1 rounds, the worst case"""
    return np.stack([np.arange(n) * step, np.zeros(n)], axis=1)


def coincident(n):
    return np.full((n, 2), 7.0)


def small(n):
    return np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 7.0], [0.0, 7.0], [4.0, 3.0]])[:n]
