"""CPU reference of the Held-Karp definitions in include/tsp_hip.h, numpy fp64 (restated here on purpose):

  weight of edge {i,j}, lo = min, hi = max:  w = (d(lo,hi) + pi[lo]) + pi[hi]
  edge order: lexicographic on (w, lo, hi) -- strict, so the minimum spanning tree is unique
  1-tree: the minimum spanning tree of nodes 1 .. n-1 under that order + the two smallest edges at node 0
  value:  W(pi) = sum of w(e) - 2 sum of pi   (math.fsum here)
  ascent: pi as given, lambda = lambda0, best = -inf, stall = 0; per iteration the 1-tree, W, g = deg - 2; W > best keeps
          best / pi_best and clears stall, else stall += 1 and at `patience` lambda is halved; |g|^2 == 0 stops (a tour);
          t = lambda (ub - W) / |g|^2, pi += t (0.7 g + 0.3 g_prev), g_prev = g in the first iteration.

`D` is the oracle's distance matrix (oracle.oracle.dist_matrix), or any object with `n` and `row(t)` = d(min(t,u), max(t,u))
for every u (Euc2DRows: sizes whose matrix does not fit)."""
import math

import numpy as np


class Matrix:
    def __init__(self, D):
        self.D = np.asarray(D, dtype=np.float64)
        self.n = len(self.D)

    def row(self, t):
        r = self.D[t].copy()
        r[:t] = self.D[:t, t]   # d(lo, hi) with lo first (GEO through a device matrix is not symmetric to the bit)
        return r


class Euc2DRows:
    """EUC_2D with integer costs, row by row: nint(sqrt(dx^2 + dy^2)) as src/distutil.c:13-18 (exact operands for integer
    coordinates below 2^26, a correctly rounded root, (int)(x + 0.5))."""

    def __init__(self, xy):
        self.xy = np.asarray(xy, dtype=np.float64)
        self.n = len(self.xy)

    def row(self, t):
        dx = self.xy[t, 0] - self.xy[:, 0]
        dy = self.xy[t, 1] - self.xy[:, 1]
        return np.trunc(np.sqrt(dx * dx + dy * dy) + 0.5)


def _rows(D):
    return D if hasattr(D, "row") else Matrix(D)


def _weights(R, pi, t, idx):
    d = R.row(t)
    below = idx < t
    return (d + np.where(below, pi, pi[t])) + np.where(below, pi[t], pi)


def one_tree(D, pi=None):
    """-> (edges [n,2] sorted (lo, hi), deg [n], value, weights [n] in the edges' order).  Prim, vectorised over the
    frontier; every choice is the smallest (w, lo, hi) across the cut."""
    R = _rows(D)
    n = R.n
    assert n >= 3
    pi = np.zeros(n) if pi is None else np.asarray(pi, dtype=np.float64)
    idx = np.arange(n)
    done = np.zeros(n, dtype=bool)
    done[0] = True   # node 0 is not part of the spanning tree
    bw = np.full(n, np.inf)
    blo = np.full(n, -1, dtype=np.int64)
    bhi = np.full(n, -1, dtype=np.int64)
    t = 1
    done[1] = True
    E = []
    for _ in range(n - 2):
        w = _weights(R, pi, t, idx)
        lo, hi = np.minimum(idx, t), np.maximum(idx, t)
        better = ~done & ((w < bw) | ((w == bw) & ((lo < blo) | ((lo == blo) & (hi < bhi)))))
        bw[better], blo[better], bhi[better] = w[better], lo[better], hi[better]
        cw = np.where(done, np.inf, bw)
        c = np.flatnonzero(cw == cw.min())
        u = int(c[0]) if len(c) == 1 else int(min(c, key=lambda q: (blo[q], bhi[q])))
        E.append((int(blo[u]), int(bhi[u]), float(bw[u])))
        done[u] = True
        t = u
    w0 = _weights(R, pi, 0, idx)
    w0[0] = np.inf
    for c in np.lexsort((idx, w0))[:2]:
        E.append((0, int(c), float(w0[c])))
    E.sort(key=lambda e: (e[0], e[1]))
    edges = np.array([(a, b) for a, b, _ in E], dtype=np.int32)
    deg = np.bincount(edges.ravel(), minlength=n).astype(np.int32)
    ws = np.array([w for _, _, w in E])
    value = math.fsum(ws) - 2.0 * math.fsum(pi)
    return edges, deg, value, ws


def kruskal_one_tree(D, pi=None):
    """The same 1-tree from the plain definition: every edge sorted by (w, lo, hi), union-find over nodes 1 .. n-1."""
    R = _rows(D)
    n = R.n
    pi = np.zeros(n) if pi is None else np.asarray(pi, dtype=np.float64)
    idx = np.arange(n)
    all_e = []
    for lo in range(n):
        w = _weights(R, pi, lo, idx)
        all_e += [(float(w[hi]), lo, hi) for hi in range(lo + 1, n)]
    all_e.sort()
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    E, zero = [], 0
    for w, lo, hi in all_e:
        if lo == 0:
            if zero < 2:
                E.append((lo, hi, w))
                zero += 1
            continue
        a, b = find(lo), find(hi)
        if a != b:
            parent[a] = b
            E.append((lo, hi, w))
    E.sort(key=lambda e: (e[0], e[1]))
    return np.array([(a, b) for a, b, _ in E], dtype=np.int32), np.array([w for _, _, w in E])


def default_patience(n):
    return max(10, n // 20)


def ascent(D, ub, iters=300, lambda0=2.0, patience=0, pi=None):
    """-> (best, pi_best, info); info: iterations, tour_found, lambda, trace (best after every iteration)."""
    R = _rows(D)
    n = R.n
    pi = np.zeros(n) if pi is None else np.array(pi, dtype=np.float64)
    patience = patience if patience > 0 else default_patience(n)
    lam, best, stall = float(lambda0), -math.inf, 0
    pi_best = pi.copy()
    g_prev = None
    trace = []
    tour = False
    k = 0
    for k in range(1, iters + 1):
        _, deg, W, _ = one_tree(R, pi)
        g = deg.astype(np.float64) - 2.0
        if W > best:
            best, pi_best, stall = W, pi.copy(), 0
        else:
            stall += 1
            if stall >= patience:
                lam, stall = lam * 0.5, 0
        trace.append(best)
        g2 = float(np.dot(g, g))
        if g2 == 0.0:
            tour = True
            break
        if g_prev is None:
            g_prev = g
        t = lam * (ub - W) / g2
        pi = pi + t * (0.7 * g + 0.3 * g_prev)
        g_prev = g
    return best, pi_best, {"iterations": k, "tour_found": tour, "lambda": lam, "trace": trace}
