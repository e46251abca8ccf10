"""CPU reference of the Held-Karp definitions in include/tsp_hip.h, numpy fp64 (restated here on purpose):

  weight of edge {i,j}, lo = min, hi = max:  w = (d(lo,hi) + pi[lo]) + pi[hi]
  edge order: lexicographic on (w, lo, hi) -- strict, so the minimum spanning tree is unique
  1-tree: the minimum spanning tree of nodes 1 .. n-1 under that order + the two smallest edges at node 0
  value:  W(pi) = sum of w(e) - 2 sum of pi   (math.fsum here; `sum_order`: plain sums in a random order instead)
  ascent: pi as given, lambda = lambda0, best = -inf, stall = 0; per iteration the 1-tree, W, g = deg - 2; W > best keeps
          best / pi_best and clears stall, else stall += 1 and at `patience` lambda is halved; |g|^2 == 0 stops (a tour);
          t = lambda (ub - W) / |g|^2, pi += t (0.7 g + 0.3 g_prev), g_prev = g in the first iteration.
  Boruvka rounds (what the device's `rounds` counts): over nodes 1 .. n-1, every component takes its smallest outgoing edge
          under the same order, all chosen edges are contracted; a round counts while more than one component exists.

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


def _plain_sum(x, rng):
    """x summed left to right in double, in an order drawn from rng: some summation order other than fsum's"""
    s = 0.0
    for v in x[rng.permutation(len(x))].tolist():
        s += v
    return s


def one_tree(D, pi=None, sum_order=None):
    """-> (edges [n,2] sorted (lo, hi), deg [n], value, weights [n] in the edges' order).  Prim, vectorised over the
    frontier; every choice is the smallest (w, lo, hi) across the cut.  sum_order: None = math.fsum, or a numpy generator:
    the value from plain sums of the randomly permuted weights and penalties."""
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
    if sum_order is None:
        value = math.fsum(ws) - 2.0 * math.fsum(pi)
    else:
        value = _plain_sum(ws, sum_order) - 2.0 * _plain_sum(pi, sum_order)
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


class Step:
    """One iteration of the ascent: `pi` the penalties its tree was built for, `W`, `deg`, `g2` = |g|^2 of that tree, and
    `best`, `lam`, `pi_best` after the iteration's bookkeeping."""
    __slots__ = ("k", "pi", "W", "deg", "g2", "best", "lam", "pi_best")

    def __init__(self, **kw):
        for f, v in kw.items():
            setattr(self, f, v)


def ascent_trace(D, ub, iters, lambda0=2.0, patience=0, pi=None, sum_order=None):
    """The ascent, every iteration kept -> [Step]; it ended on a tour iff the last step's g2 is 0.  sum_order as one_tree's."""
    R = _rows(D)
    n = R.n
    pi = np.zeros(n) if pi is None else np.array(pi, dtype=np.float64)
    patience = patience if patience > 0 else default_patience(n)
    lam, best, stall = float(lambda0), -math.inf, 0
    pi_best = pi.copy()
    g_prev = None
    steps = []
    for k in range(1, iters + 1):
        _, deg, W, _ = one_tree(R, pi, sum_order)
        g = deg.astype(np.float64) - 2.0
        if W > best:
            best, pi_best, stall = W, pi.copy(), 0
        else:
            stall += 1
            if stall >= patience:
                lam, stall = lam * 0.5, 0
        g2 = float(np.dot(g, g))
        steps.append(Step(k=k, pi=pi, W=W, deg=deg, g2=g2, best=best, lam=lam, pi_best=pi_best))
        if g2 == 0.0:
            break
        if g_prev is None:
            g_prev = g
        t = lam * (ub - W) / g2
        pi = pi + t * (0.7 * g + 0.3 * g_prev)
        g_prev = g
    return steps


def ascent(D, ub, iters=300, lambda0=2.0, patience=0, pi=None):
    """-> (best, pi_best, info); info: iterations, tour_found, lambda, trace (best after every iteration)."""
    steps = ascent_trace(D, ub, iters, lambda0, patience, pi)
    last = steps[-1]
    return last.best, last.pi_best, {"iterations": last.k, "tour_found": last.g2 == 0.0, "lambda": last.lam,
                                     "trace": [s.best for s in steps]}


def boruvka(D, pi=None, hi_first=False):
    """Boruvka over nodes 1 .. n-1 -> (rounds, the spanning tree's edges, sorted).  In a round every component takes its
    smallest outgoing edge under (w, lo, hi), all chosen edges are contracted, and the round counts while more than one
    component exists at its start.  hi_first: the order (w, hi, lo) instead (to show that the order matters)."""
    R = _rows(D)
    n = R.n
    pi = np.zeros(n) if pi is None else np.asarray(pi, dtype=np.float64)
    idx = np.arange(n)
    w = np.array([_weights(R, pi, t, idx) for t in range(n)])
    w[0, :] = w[:, 0] = np.inf   # node 0 is not part of the spanning tree
    comp = idx.copy()
    E = set()
    rounds = 0
    while len(set(comp[1:].tolist())) > 1:
        rounds += 1
        out = np.where(comp[:, None] != comp[None, :], w, np.inf)
        other = out.argmin(axis=1)   # of a node's equal weights the lowest other end: its smallest (lo, hi) and (hi, lo) alike
        pick = {}
        for v in range(1, n):
            u = int(other[v])
            lo, hi = min(u, v), max(u, v)
            key = (float(out[v, u]), hi, lo) if hi_first else (float(out[v, u]), lo, hi)
            c = int(comp[v])
            if c not in pick or key < pick[c][0]:
                pick[c] = (key, lo, hi)
        for _, lo, hi in pick.values():
            E.add((lo, hi))
            a, b = comp[lo], comp[hi]
            if a != b:   # (equal when both chose this edge and the first pick has joined them)
                comp[comp == b] = a
    return rounds, sorted(E)


def boruvka_rounds(D, pi=None):
    return boruvka(D, pi)[0]
