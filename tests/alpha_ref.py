"""CPU reference of the alpha-nearness definitions in include/tsp_hip.h, numpy fp64 (restated here on purpose):

  d, pi, w = (d(lo,hi) + pi[lo]) + pi[hi], the edge order (w, lo, hi) and the minimum 1-tree T with special node 0 are those of
  tests/held_karp_ref.py.  For i != j:
    {i,j} an edge of T:   alpha = 0
    else i = 0 or j = 0:  alpha = w(i,j) - w0, w0 = the weight of the larger of the two 1-tree edges at node 0
    else:                 alpha = w(i,j) - beta(i,j), beta = the largest weight on the path from i to j in the spanning tree of
                          nodes 1 .. n-1
  lists: nbr[v][0 .. K-1] = the K nodes u != v smallest by (alpha(v,u), w(v,u), u).

The tree comes from held_karp_ref.one_tree; beta comes from an explicit walk over the tree (from the row's node outwards, or
parents before children for a whole matrix), NOT from the dendrogram order the device uses."""
import numpy as np

import held_karp_ref as HK


def weight_row(R, pi, t):
    n = R.n
    return HK._weights(R, pi, t, np.arange(n))


def tree_parts(D, pi=None):
    """-> (R, pi, edges, ws, adj, c1, c2, w0): adj[v] = [(u, w)] over the spanning tree of nodes 1 .. n-1; (0, c1), (0, c2) the
    special edges, smaller first; w0 the larger one's weight"""
    R = HK._rows(D)
    n = R.n
    pi = np.zeros(n) if pi is None else np.asarray(pi, dtype=np.float64)
    edges, _, _, ws = HK.one_tree(R, pi)
    adj = [[] for _ in range(n)]
    special = []
    for (a, b), w in zip(edges.tolist(), ws.tolist()):
        if a == 0:
            special.append((w, b))
        else:
            adj[a].append((b, w))
            adj[b].append((a, w))
    special.sort()
    assert len(special) == 2
    return R, pi, edges, ws, adj, special[0][1], special[1][1], special[1][0]


def beta_row(adj, n, i):
    """beta(i, .) by a walk from i over the spanning tree (i >= 1); -inf at i itself and at node 0"""
    beta = np.full(n, -np.inf)
    stack = [(i, -1, -np.inf)]
    while stack:
        v, dad, m = stack.pop()
        beta[v] = m
        for u, w in adj[v]:
            if u != dad:
                stack.append((u, v, w if w > m else m))
    return beta


def beta_matrix(adj, n):
    """beta for every pair of nodes 1 .. n-1: the tree rooted at node 1, parents before children (Helsgaun's recurrence
    beta(i, j) = max(beta(dad i, j), w(i, dad i)) for every j met before i)"""
    B = np.full((n, n), -np.inf)
    order, dad, wdad = [1], {1: -1}, {}
    k = 0
    while k < len(order):
        v = order[k]
        k += 1
        for u, w in adj[v]:
            if u != dad[v]:
                dad[u] = v
                wdad[u] = w
                order.append(u)
    assert len(order) == n - 1
    for k in range(1, len(order)):
        i = order[k]
        prev = np.array(order[:k])
        b = np.maximum(B[dad[i], prev], wdad[i])
        B[i, prev] = b
        B[prev, i] = b
    return B


def _finish_row(i, w, beta, edges_at, c1, c2, w0):
    """alpha(i, .) from the row's weights and betas"""
    n = len(w)
    if i == 0:
        a = w - w0
    else:
        a = w - beta
        a[0] = w[0] - w0
    for u in edges_at:
        a[u] = 0.0
    a[i] = 0.0
    return a


def alpha_rows(D, pi=None, rows=None):
    """-> (A [m, n], Wt [m, n], edges): alpha and weight rows of the nodes `rows` (None: every node), A[r][rows[r]] = 0"""
    R, pi, edges, ws, adj, c1, c2, w0 = tree_parts(D, pi)
    n = R.n
    nb = [[] for _ in range(n)]
    for a, b in edges.tolist():
        nb[a].append(b)
        nb[b].append(a)
    full = rows is None
    rows = np.arange(n) if full else np.asarray(rows)
    B = beta_matrix(adj, n) if full else None
    A = np.zeros((len(rows), n))
    Wt = np.zeros((len(rows), n))
    for r, i in enumerate(rows.tolist()):
        w = weight_row(R, pi, i)
        beta = None if i == 0 else (B[i] if full else beta_row(adj, n, i))
        A[r] = _finish_row(i, w, beta, nb[i], c1, c2, w0)
        Wt[r] = w
    return A, Wt, edges


def lists(A, Wt, rows, K):
    """-> (nbr [m, K] int32, alpha [m, K]) by a lexsort on (alpha, w, u) over u != the row's node"""
    m, n = A.shape
    nbr = np.zeros((m, K), dtype=np.int32)
    al = np.zeros((m, K))
    idx = np.arange(n)
    for r, v in enumerate(np.asarray(rows).tolist()):
        o = np.lexsort((idx, Wt[r], A[r]))
        o = o[o != v][:K]
        nbr[r] = o
        al[r] = A[r][o]
    return nbr, al
