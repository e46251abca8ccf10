"""CPU reference of the partition crossover, written from the definition in include/tsp_hip.h ("partition crossover"): union-find,
plain loops, Python ints for q.  Nothing here is shared with the device code: the device scans positions, this walks nodes.

gpx(succ_a, succ_b, dist) -> (succ_child, stats).  dist(i, j) takes two equally long integer arrays with i < j element-wise and returns
the distances as floats: the device's own tsp_dev_dist_pairs in the GPU tests, a numpy metric in the CPU tests.
"""
import math

import numpy as np

Q_LIMIT = 1 << 62


def order_of(succ):
    """Node sequence from node 0; raises when succ is not one Hamiltonian cycle."""
    n = len(succ)
    seen = [False] * n
    out = []
    v = 0
    for _ in range(n):
        if not (0 <= v < n) or seen[v]:
            raise ValueError("not a tour")
        seen[v] = True
        out.append(v)
        v = int(succ[v])
    if v != 0:
        raise ValueError("not a tour")
    return out


def _edge(u, v):
    return (u, v) if u < v else (v, u)


def q_of(d):
    """llrint(ldexp(d, 20)): round-half-even of an exactly scaled double."""
    return int(round(math.ldexp(float(d), 20)))


def edge_q(edges, dist):
    """{edge: q} for a collection of (lo, hi) edges, one dist call."""
    es = sorted(set(edges))
    d = dist(np.array([e[0] for e in es], dtype=np.int32), np.array([e[1] for e in es], dtype=np.int32))
    return {e: q_of(x) for e, x in zip(es, d)}


def tour_cost(succ, dist):
    """Sum over nodes in node order of d(v, succ v) (lower id first), added left to right like a host loop."""
    n = len(succ)
    lo = np.minimum(np.arange(n), succ).astype(np.int32)
    hi = np.maximum(np.arange(n), succ).astype(np.int32)
    total = 0.0
    for x in dist(lo, hi):
        total += float(x)
    return total


class _UF:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, v):
        while self.p[v] != v:
            self.p[v] = self.p[self.p[v]]
            v = self.p[v]
        return v

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.p[max(a, b)] = min(a, b)


def _runs_and_stretches(order, common, c):
    """Walks one tour.  Returns (runs, stretches): runs = [(end, other end, external)], stretches = node lists from portal to portal
    in the tour's direction (empty when there is no external run)."""
    n = len(order)
    is_c = [_edge(order[p], order[(p + 1) % n]) in common for p in range(n)]
    if all(is_c) or not any(is_c):
        return [], []
    runs = []
    ext_edge = [False] * n
    for p in range(n):
        if is_c[p] and not is_c[p - 1]:   # a run starts at the node at p
            e = p
            while is_c[e % n]:
                e += 1
            a, b = order[p], order[e % n]
            external = c[a] != c[b]
            runs.append((a, b, external))
            if external:
                for k in range(p, e):
                    ext_edge[k % n] = True
    stretches = []
    if any(ext_edge):
        for p in range(n):
            if ext_edge[p - 1] and not ext_edge[p]:   # the stretch starts with the node at p
                seq = [order[p]]
                k = p
                while not ext_edge[k % n]:
                    k += 1
                    seq.append(order[k % n])
                stretches.append(seq)
    return runs, stretches


def gpx(succ_a, succ_b, dist):
    succ_in = [np.asarray(succ_a).astype(np.int64), np.asarray(succ_b).astype(np.int64)]
    n = len(succ_in[0])
    assert n >= 3 and len(succ_in[1]) == n
    orders = [order_of(s) for s in succ_in]
    edges = [[_edge(o[p], o[(p + 1) % n]) for p in range(n)] for o in orders]
    q = edge_q(edges[0] + edges[1], dist)
    sums = [sum(q[e] for e in es) for es in edges]
    if max(sums) >= Q_LIMIT:
        raise OverflowError("a parent's fixed-point length reaches 2^62")
    base = 1 if sums[1] < sums[0] else 0
    A, B = orders[base], orders[1 - base]
    eA, eB = edges[base], edges[1 - base]
    common = set(eA) & set(eB)
    stats = dict(common_edges=len(common), components=0, exchangeable=0, taken=0, stretches=0, gain_q=0, base=base,
                 cost_a=tour_cost(succ_in[0], dist), cost_b=tour_cost(succ_in[1], dist))
    child = succ_in[base].copy()

    uf = _UF(n)
    in_h = [False] * n
    for e in list(eA) + list(eB):
        if e not in common:
            uf.union(e[0], e[1])
            in_h[e[0]] = in_h[e[1]] = True
    c = [uf.find(v) for v in range(n)]   # union keeps the smaller id on top: the root is the smallest id
    comps = sorted({c[v] for v in range(n) if in_h[v]})
    stats["components"] = len(comps)

    _, sA = _runs_and_stretches(A, common, c)
    _, sB = _runs_and_stretches(B, common, c)
    stats["stretches"] = len(sA)
    assert len(sA) == len(sB)
    by_comp_a, by_comp_b = {}, {}
    for seq in sA:
        assert len({c[v] for v in seq if in_h[v]}) == 1
        by_comp_a.setdefault(c[seq[0]], []).append(seq)
    for seq in sB:
        by_comp_b.setdefault(c[seq[0]], {})[frozenset((seq[0], seq[-1]))] = seq
    qa = {k: 0 for k in comps}
    qb = {k: 0 for k in comps}
    for e in eA:
        if e not in common:
            qa[c[e[0]]] += q[e]
    for e in eB:
        if e not in common:
            qb[c[e[0]]] += q[e]
    stats["taken_components"] = []
    stats["tied_components"] = []
    for k in comps:
        mine = by_comp_a.get(k, [])
        theirs = by_comp_b.get(k, {})
        exch = len(mine) > 0 and all(frozenset((s[0], s[-1])) in theirs for s in mine)
        if not exch:
            continue
        stats["exchangeable"] += 1
        if qb[k] == qa[k]:
            stats["tied_components"].append(k)
        if not qb[k] < qa[k]:
            continue
        stats["taken"] += 1
        stats["gain_q"] += qa[k] - qb[k]
        stats["taken_components"].append(k)
        assert sorted(v for s in mine for v in s) == sorted(v for s in theirs.values() for v in s)
        for s in mine:
            t = theirs[frozenset((s[0], s[-1]))]
            if t[0] != s[0]:
                t = t[::-1]
            for u, v in zip(t[:-1], t[1:]):
                child[u] = v
    order_of(child)   # one cycle
    stats["cost_child"] = tour_cost(child, dist)
    stats["sum_q"] = sums
    stats["sum_q_child"] = sum(edge_q([_edge(v, int(child[v])) for v in range(n)], dist).values())
    return child.astype(np.int32), stats


def tournament(tours, dist):
    """Rounds of pairwise gpx over [T, n]: pairs (0,1), (2,3), ..., an odd one passes through, until one tour is left.
    -> (succ, cost, per-round list of per-pair stats)."""
    tours = [np.asarray(t).astype(np.int32) for t in tours]
    rounds = []
    while len(tours) > 1:
        nxt, st = [], []
        for k in range(0, len(tours) - 1, 2):
            ch, s = gpx(tours[k], tours[k + 1], dist)
            nxt.append(ch)
            st.append(s)
        if len(tours) % 2:
            nxt.append(tours[-1])
        tours = nxt
        rounds.append(st)
    return tours[0], tour_cost(tours[0], dist), rounds


# ---- fixtures shared by the CPU and GPU tests -------------------------------------------------------------------------------

def euc(xy, integer):
    """numpy EUC_2D on coordinates xy [n, 2]: nint(sqrt) when integer, as the instance's own metric computes it."""
    xy = np.asarray(xy, dtype=np.float64)

    def dist(i, j):
        d = xy[i] - xy[j]
        r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        return np.trunc(r + 0.5) if integer else r
    return dist


def succ_from_order(order):
    order = np.asarray(order)
    s = np.empty(len(order), dtype=np.int32)
    s[order] = np.roll(order, -1)
    return s


def nearest_neighbour_order(xy):
    xy = np.asarray(xy, dtype=np.float64)
    n = len(xy)
    left = np.ones(n, dtype=bool)
    o = [0]
    left[0] = False
    for _ in range(n - 1):
        d = ((xy - xy[o[-1]]) ** 2).sum(1)
        d[~left] = np.inf
        v = int(np.argmin(d))
        o.append(v)
        left[v] = False
    return o


def _two_opt_window(o, xy):
    """2-opt (first improvement, until none) on the open path o with fixed ends, plain Euclidean lengths."""
    pts = np.asarray([xy[v] for v in o], dtype=np.float64)
    dd = pts[:, None, :] - pts[None, :, :]
    D = np.sqrt((dd * dd).sum(2)).tolist()   # by slot of the incoming path
    idx = list(range(len(o)))
    improved = True
    while improved:
        improved = False
        for i in range(1, len(idx) - 2):
            for j in range(i + 1, len(idx) - 1):
                a, b, c, e = idx[i - 1], idx[i], idx[j], idx[j + 1]
                if D[a][c] + D[b][e] < D[a][b] + D[c][e] - 1e-9:
                    idx[i:j + 1] = idx[i:j + 1][::-1]
                    improved = True
    return [o[k] for k in idx]


def windowed_parents(xy, seed, window=40, prob=0.6, offset=13, start=None):
    """Two tours from one start (nearest neighbour unless given): 2-opt inside windows of `window` nodes, each with probability
    `prob`; the second parent's windows are shifted by `offset`.  -> (succ_a, succ_b)."""
    rng = np.random.default_rng(seed)
    start = nearest_neighbour_order(xy) if start is None else list(start)
    n = len(start)
    out = []
    for shift in (0, offset):
        o = start[shift:] + start[:shift]
        for w in range(0, n - window + 1, window):
            if rng.random() < prob:
                o[w:w + window] = _two_opt_window(o[w:w + window], xy)
        out.append(succ_from_order(o))
    return out[0], out[1]
