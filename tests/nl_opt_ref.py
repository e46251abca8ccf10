"""CPU reference of the neighbour-list neighbourhood of include/tsp_hip.h (tsp_dev_inst_knn_*, tsp_dev_nl_opt), numpy over
the oracle's distance matrix.  A helper of the tests, not collected by pytest.

Lists: nbr[v] = the K nodes u != v smallest by (d(v,u), u).  u ~ v when u in N(v) or v in N(u): M = N | N^T.
kind 0, 2-opt: i < j, i1 = succ i, j1 = succ j, not (j == i1 or j1 == i); delta = ((d(i,j) + d(i1,j1)) - d(i,i1)) - d(j,j1);
    key = i*n + j; in the neighbourhood iff M[i,j] or M[i1,j1].
kind 1, Or-opt: the moves (f, L, a, o) of or_opt_ref; in the neighbourhood iff (o = 0) M[a,f] or M[l,b], (o = 1) M[a,l] or M[f,b].
Decision: smallest delta < 0, ties -> lower kind, then lower key."""
import numpy as np

import or_opt_ref as R

NL_2OPT, NL_OROPT = 1, 2


def knn(D, K):
    """(n, K) int32: per row the K nodes other than the row's own, by (distance, id)."""
    n = len(D)
    assert 1 <= K <= n - 1
    Dm = np.array(D, dtype=np.float64, copy=True)
    Dm[np.arange(n), np.arange(n)] = np.inf
    return np.argsort(Dm, axis=1, kind="stable")[:, :K].astype(np.int32)


def mask(nbr, n):
    """M = N | N^T as an n x n bool matrix (asymmetric lists and duplicates are fine)."""
    nbr = np.asarray(nbr)
    M = np.zeros((n, n), dtype=bool)
    M[np.repeat(np.arange(n), nbr.shape[1]), nbr.reshape(-1)] = True
    return M | M.T


def _better(c, best):
    return best is None or c < best


def decide(D, succ, nbr, kinds):
    """One decision by masking the full delta matrices -> (delta, kind, key) or None."""
    succ = np.asarray(succ, dtype=np.int64)
    n = len(succ)
    M = mask(nbr, n)
    best = None
    if kinds & NL_2OPT and n >= 4:
        i = np.arange(n)[:, None]
        j = np.arange(n)[None, :]
        si, sj = succ[:, None], succ[None, :]
        delta = ((D + D[np.ix_(succ, succ)]) - D[np.arange(n), succ][:, None]) - D[np.arange(n), succ][None, :]
        ok = (i < j) & (j != si) & (sj != i) & (M | M[np.ix_(succ, succ)])
        delta = np.where(ok, delta, np.inf)
        m = delta.min()
        if m < 0.0:
            ii, jj = np.nonzero(delta == m)
            best = (float(m), 0, int((ii * n + jj).min()))
    if kinds & NL_OROPT and n >= 5:
        order = R.tour_order(succ)
        Dp = D[np.ix_(order, order)]
        Mp = M[np.ix_(order, order)]
        Mp1 = np.roll(Mp, -1, axis=1)       # column j -> M(., position j + 1)
        E = Dp[np.arange(n), (np.arange(n) + 1) % n]
        for L, o, delta in R._decision_mats(Dp, E, order, n):
            i = np.arange(n)
            l = (i + L - 1) % n
            # rows: position i of f; columns: position j of a (b at j + 1)
            inlist = (Mp[i] | Mp1[l]) if o == 0 else (Mp[l] | Mp1[i])
            delta = np.where(inlist, delta, np.inf)
            m = delta.min()
            if not m < 0.0:
                continue
            ii, jj = np.nonzero(delta == m)
            k = int((((order[ii] * 3 + (L - 1)) * n + order[jj]) * 2 + o).min())
            c = (float(m), 1, k)
            if _better(c, best):
                best = c
    return best


def apply_two_opt(succ, i, j):
    """alg_2opt_tabu's move: succ i = j, succ i1 = j1, the forward path i1 .. j reversed -> (succ', successors rewritten by the walk)"""
    succ = np.array(succ, dtype=np.int32, copy=True)
    i1, j1 = int(succ[i]), int(succ[j])
    path = [i1]
    while path[-1] != j:
        path.append(int(succ[path[-1]]))
    succ[i] = j
    for k in range(len(path) - 1, 0, -1):
        succ[path[k]] = path[k - 1]
    succ[i1] = j1
    return succ, len(path) - 1


def new_counters():
    return {"decisions": 0, "moves": 0, "moves_2opt": 0, "moves_oropt": 0, "moves_by_len": [0, 0, 0], "moves_reversed": 0,
            "reversed": 0}


def apply_decision(succ, d, c):
    n = len(succ)
    _, kind, key = d
    c["moves"] += 1
    if kind == 0:
        succ, rev = apply_two_opt(succ, key // n, key % n)
        c["moves_2opt"] += 1
        c["reversed"] += rev
        return succ
    f, L, a, o = R.decode(key, n)
    c["moves_oropt"] += 1
    c["moves_by_len"][L - 1] += 1
    c["moves_reversed"] += o
    return R.apply_move(succ, f, L, a, o)


def effective_kinds(kinds, n):
    if n < 4:
        kinds &= ~NL_2OPT
    if n < 5:
        kinds &= ~NL_OROPT
    return kinds


def descent(D, succ, nbr, kinds, max_moves=-1, decide_fn=None):
    """-> (succ', counters as tsp_nl_opt_stats without deltas_executed and the times)"""
    succ = np.array(succ, dtype=np.int32, copy=True)
    n = len(succ)
    c = new_counters()
    kinds = effective_kinds(kinds, n)
    if kinds == 0:
        return succ, c
    while max_moves < 0 or c["moves"] < max_moves:
        c["decisions"] += 1
        d = decide_fn(succ) if decide_fn else decide(D, succ, nbr, kinds)
        if d is None:
            break
        succ = apply_decision(succ, d, c)
    return succ, c


# ---- without an n x n matrix: only the (v, u, role) candidates, EUC_2D computed directly ------------------------------------

def _euc(xy, a, b, integer_cost):
    """calc_dist of EUC_2D (src/distutil.c:13-18) for arrays of node pairs."""
    dx = xy[a, 0] - xy[b, 0]
    dy = xy[a, 1] - xy[b, 1]
    d = np.sqrt(dx * dx + dy * dy)
    return np.floor(d + 0.5) if integer_cost else d


def _take(best, delta, key, kind):
    ok = delta < 0.0
    if not ok.any():
        return best
    delta, key = delta[ok], key[ok]
    m = delta.min()
    c = (float(m), kind, int(key[delta == m].min()))
    return c if _better(c, best) else best


def entry_moves(v, u, succ, order, pos, pred, d, kind):
    """The delta expressions of the list entries (v, u), arrays with u != v, of one kind: 0, the two 2-opt moves {i, j} = {v, u}
    and {i1, j1} = {v, u}; 1, the Or-opt moves one of whose attaching edges is {v, u}: for (x, y) = (v, u) and (u, v), with the
    edge x -> y in the new tour, (a, f) = (x, y) and (l, b) = (x, y) forward, (a, l) = (x, y) and (f, b) = (x, y) reversed.
    d(x, y): the distance of two arrays of nodes.  Yields (owner v, delta, key) per expression."""
    n = len(succ)
    if kind == 0:
        for x, y in ((v, u), (pred[v], pred[u])):
            i, j = np.minimum(x, y), np.maximum(x, y)
            i1, j1 = succ[i], succ[j]
            ok = (i != j) & (j != i1) & (j1 != i)
            own, i, j, i1, j1 = v[ok], i[ok], j[ok], i1[ok], j1[ok]
            yield own, ((d(i, j) + d(i1, j1)) - d(i, i1)) - d(j, j1), i * n + j
        return
    for x, y in ((v, u), (u, v)):
        for L in (1, 2, 3):
            back = lambda z: order[(pos[z] - (L - 1)) % n]   # noqa: E731  the first node of the segment that ends at z
            for o, f, a in ((0, y, x), (0, back(x), pred[y]), (1, back(y), x), (1, x, pred[y])):
                if o == 1 and L == 1:
                    continue
                ok = ((pos[a] - pos[f] + 1) % n) > L      # a not in {p, f .. l}
                own, f, a = v[ok], f[ok], a[ok]
                pf = pos[f]
                p, l, s, b = order[(pf - 1) % n], order[(pf + L - 1) % n], order[(pf + L) % n], succ[a]
                rem = (d(p, f) + d(l, s)) - d(p, s)
                ins = (d(a, f) + d(l, b)) if o == 0 else (d(a, l) + d(f, b))
                yield own, (ins - d(a, b)) - rem, R.key(f, L, a, o, n)


def decide_sparse(xy, succ, nbr, kinds, integer_cost=1):
    """decide() for EUC_2D from the related pairs alone: every move is generated from the list edge that puts it into the
    neighbourhood and then evaluated from its own definition -> (delta, kind, key) or None."""
    xy = np.asarray(xy, dtype=np.float64)
    succ = np.asarray(succ, dtype=np.int64)
    n = len(succ)
    kinds = effective_kinds(kinds, n)
    nbr = np.asarray(nbr, dtype=np.int64)
    order = R.tour_order(succ)
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    pred = np.empty(n, dtype=np.int64)
    pred[succ] = np.arange(n)
    # the related pairs, once each: the enumeration takes both directions of an entry
    v = np.repeat(np.arange(n, dtype=np.int64), nbr.shape[1])
    u = nbr.reshape(-1)
    code = np.unique(np.minimum(v, u) * n + np.maximum(v, u))
    v, u = code // n, code % n
    v, u = v[v != u], u[v != u]
    best = None
    for kind in (0, 1):
        if kinds & (NL_2OPT, NL_OROPT)[kind]:
            for _, delta, key in entry_moves(v, u, succ, order, pos, pred, lambda a, b: _euc(xy, a, b, integer_cost), kind):
                best = _take(best, delta, key, kind)
    return best
