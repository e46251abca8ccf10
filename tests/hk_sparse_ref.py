"""CPU reference of the sparse Held-Karp definitions in include/tsp_hip.h (numpy fp64, restated here on purpose; the dense
definitions are held_karp_ref.py's):

  candidate graph C: the undirected edges {v, nbr[v][k]} of the lists, each once
  sparse 1-tree T_C: Kruskal over the edges of C among nodes 1 .. n-1 in the order (w, lo, hi); if several components are left,
          Kruskal goes on over ALL edges among nodes 1 .. n-1 (the completion); node 0 takes the two smallest edges of C at
          node 0, or, when C has fewer than two there, the two smallest of all its n - 1 edges
  W_C:    the same sum as W, over T_C
  rounds: sparse_rounds = Boruvka rounds over C in which at least one component hooks; completion_rounds = Boruvka rounds over
          the complete graph behind them, counted while more than one component exists
  ascent: a sparse phase (the dense schedule on T_C / W_C, except that |g|^2 == 0 ends it without a tour being claimed and
          W_C >= ub ends it before the step), then held_karp_ref.ascent_trace from pi_best_C with the sparse phase's lambda.

`D`: a distance matrix or an object with `n` and `row(t)`, as in held_karp_ref.py.  `nbr`: (n, K) integer lists."""
import math

import numpy as np

import held_karp_ref as HK


def cand_edges(nbr):
    """-> sorted [(lo, hi)] of the candidate graph"""
    nbr = np.asarray(nbr)
    v = np.repeat(np.arange(len(nbr)), nbr.shape[1])
    u = nbr.ravel()
    return sorted(set(zip(np.minimum(v, u).tolist(), np.maximum(v, u).tolist())))


def _weigh(R, pi, pairs):
    """[(lo, hi)] -> [(w, lo, hi)] with w = (d(lo, hi) + pi[lo]) + pi[hi]"""
    rows = {}
    out = []
    for lo, hi in pairs:
        if lo not in rows:
            rows[lo] = R.row(lo)
        out.append((float((rows[lo][hi] + pi[lo]) + pi[hi]), lo, hi))
    return out


def _all_pairs(n, first):
    return [(lo, hi) for lo in range(first, n) for hi in range(lo + 1, n)]


class _Sets:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, a):
        while self.p[a] != a:
            self.p[a] = self.p[self.p[a]]
            a = self.p[a]
        return a

    def join(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.p[max(a, b)] = min(a, b)
        return True


def _node0(R, pi, C, n):
    at0 = [(lo, hi) for lo, hi in C if lo == 0]
    if len(at0) < 2:
        at0 = [(0, c) for c in range(1, n)]
    return sorted(_weigh(R, pi, at0))[:2]


def _finish(E, pi, n, sum_order):
    E = sorted(E, key=lambda e: (e[1], e[2]))
    edges = np.array([(lo, hi) for _, lo, hi in E], dtype=np.int32)
    deg = np.bincount(edges.ravel(), minlength=n).astype(np.int32)
    ws = np.array([w for w, _, _ in E])
    if sum_order is None:
        value = math.fsum(ws) - 2.0 * math.fsum(pi)
    else:
        value = HK._plain_sum(ws, sum_order) - 2.0 * HK._plain_sum(pi, sum_order)
    return edges, deg, value, ws


def one_tree_sparse(D, nbr, pi=None, sum_order=None):
    """T_C by the two-stage Kruskal -> (edges [n,2] sorted (lo, hi), deg [n], W_C, weights in the edges' order, components of C
    on nodes 1 .. n-1)"""
    R = HK._rows(D)
    n = R.n
    assert n >= 3
    pi = np.zeros(n) if pi is None else np.asarray(pi, dtype=np.float64)
    C = cand_edges(nbr)
    S = _Sets(n)
    E = []
    for w, lo, hi in sorted(_weigh(R, pi, [e for e in C if e[0] >= 1])):
        if S.join(lo, hi):
            E.append((w, lo, hi))
    components = n - 1 - len(E)
    if components > 1:
        for w, lo, hi in sorted(_weigh(R, pi, _all_pairs(n, 1))):
            if S.join(lo, hi):
                E.append((w, lo, hi))
    assert len(E) == n - 2
    E += _node0(R, pi, C, n)
    return _finish(E, pi, n, sum_order) + (components,)


def _boruvka_stage(keyed, comp):
    """Boruvka rounds over the edges `keyed` = sorted [(w, lo, hi)] from the component labels `comp` (changed in place) ->
    (rounds, chosen edges).  A round in which no component has an outgoing edge ends the stage and is not counted."""
    rounds, chosen = 0, []
    while len(set(comp[1:].tolist())) > 1:
        pick = {}
        for key in keyed:   # ascending: the first edge seen from a component is its smallest
            a, b = int(comp[key[1]]), int(comp[key[2]])
            if a != b:
                pick.setdefault(a, key)
                pick.setdefault(b, key)
        if not pick:
            break
        rounds += 1
        for key in set(pick.values()):
            chosen.append(key)
            a, b = comp[key[1]], comp[key[2]]
            if a != b:
                comp[comp == max(a, b)] = min(a, b)
    return rounds, chosen


def boruvka_sparse(D, nbr, pi=None, sum_order=None):
    """The same tree by Boruvka, first over C, then over the complete graph -> (sparse_rounds, completion_rounds, components,
    edges, deg, W_C, weights)"""
    R = HK._rows(D)
    n = R.n
    pi = np.zeros(n) if pi is None else np.asarray(pi, dtype=np.float64)
    C = cand_edges(nbr)
    comp = np.arange(n)
    rs, E = _boruvka_stage(sorted(_weigh(R, pi, [e for e in C if e[0] >= 1])), comp)
    components = len(set(comp[1:].tolist()))
    rc = 0
    if components > 1:
        rc, more = _boruvka_stage(sorted(_weigh(R, pi, _all_pairs(n, 1))), comp)
        E += more
    assert len(E) == n - 2, (len(E), n)
    E += _node0(R, pi, C, n)
    return (rs, rc, components) + _finish(E, pi, n, sum_order)


class SparseTrace:
    """sparse: [HK.Step] of the sparse phase (W = W_C); tree_rounds: [(sparse_rounds, completion_rounds)] of its trees when
    `rounds` was asked for; ended: "iters", "tour" or "ub"; lam, best, pi_best: what the phase hands over (lambda0, -inf and the
    start when it has no iteration); dense: [HK.Step] of the dense phase."""

    def __init__(self, **kw):
        for f, v in kw.items():
            setattr(self, f, v)

    @property
    def bound(self):
        return self.dense[-1].best

    @property
    def pi_out(self):
        return self.dense[-1].pi_best

    @property
    def tour_found(self):
        return self.dense[-1].g2 == 0.0


def sparse_phase(D, nbr, ub, sparse_iters, lambda0=2.0, patience=0, pi=None, sum_order=None, rounds=False):
    """-> (steps, ended, lam, best, pi_best, tree_rounds)"""
    R = HK._rows(D)
    n = R.n
    pi = np.zeros(n) if pi is None else np.array(pi, dtype=np.float64)
    patience = patience if patience > 0 else HK.default_patience(n)
    lam, best, stall = float(lambda0), -math.inf, 0
    pi_best = pi.copy()
    g_prev = None
    steps, ended, tree_rounds = [], "iters", []
    for k in range(1, sparse_iters + 1):
        if rounds:
            rs, rc, _, _, deg, W, _ = boruvka_sparse(R, nbr, pi, sum_order)
        else:
            _, deg, W, _, _ = one_tree_sparse(R, nbr, pi, sum_order)
        g = deg.astype(np.float64) - 2.0
        if W > best:
            best, pi_best, stall = W, pi.copy(), 0
        else:
            stall += 1
            if stall >= patience:
                lam, stall = lam * 0.5, 0
        g2 = float(np.dot(g, g))
        steps.append(HK.Step(k=k, pi=pi, W=W, deg=deg, g2=g2, best=best, lam=lam, pi_best=pi_best))
        if rounds:
            tree_rounds.append((rs, rc))
        if g2 == 0.0:
            ended = "tour"
            break
        if W >= ub:
            ended = "ub"
            break
        if g_prev is None:
            g_prev = g
        t = lam * (ub - W) / g2
        pi = pi + t * (0.7 * g + 0.3 * g_prev)
        g_prev = g
    return steps, ended, lam, best, pi_best, tree_rounds


def hand_over(D, ub, steps, k, dense_iters, lambda0=2.0, patience=0, pi=None, sum_order=None):
    """The dense phase behind the first k steps of a sparse phase (k = 0: from the start) -> [HK.Step]"""
    if k == 0:
        return HK.ascent_trace(D, ub, dense_iters, lambda0, patience, pi, sum_order)
    s = steps[k - 1]
    return HK.ascent_trace(D, ub, dense_iters, s.lam, patience, s.pi_best, sum_order)


def ascent_trace_sparse(D, nbr, ub, sparse_iters, dense_iters=1, lambda0=2.0, patience=0, pi=None, sum_order=None, rounds=False):
    """The two phases -> SparseTrace"""
    steps, ended, lam, best, pi_best, tree_rounds = sparse_phase(D, nbr, ub, sparse_iters, lambda0, patience, pi, sum_order, rounds)
    dense = hand_over(D, ub, steps, len(steps), dense_iters, lambda0, patience, pi, sum_order)
    return SparseTrace(sparse=steps, ended=ended, lam=lam, best=best, pi_best=pi_best, dense=dense, tree_rounds=tree_rounds)


def knn_lists(D, K):
    """(n, K) nearest-neighbour lists by (d, id) on a symmetric matrix (the tests' own lists; the device's are its own)"""
    D = np.asarray(D, dtype=np.float64)
    n = len(D)
    out = np.zeros((n, K), dtype=np.int32)
    for v in range(n):
        d = D[v].copy()
        d[v] = np.inf
        out[v] = np.lexsort((np.arange(n), d))[:K]
    return out
