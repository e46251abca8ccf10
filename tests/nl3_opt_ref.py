"""CPU reference of the candidate-list 3-opt kind of include/tsp_hip.h (tsp_dev_nl_3opt), numpy over the oracle's distance
matrix.  A helper of the tests, not collected by pytest.

Three distinct tour edges are removed, named by their tails a, b, c (heads a1, b1, c1): a is the tail of lowest node id, b and c
follow it in tour order.  S1 = a1 .. b, S2 = b1 .. c, S3 = c1 .. a.  The four pure reconnections, new edges (e1, e2, e3):
    0: (a,b1) (c,a1) (b,c1)   a S2 S1 c1 ..        1: (a,b) (a1,c) (b1,c1)   a S1' S2' c1 ..
    2: (a,c) (b1,a1) (b,c1)   a S2' S1 c1 ..       3: (a,b1) (c,b) (a1,c1)   a S2 S1' c1 ..      (' = reversed)
(a, b, c, type) is a move iff none of its new edges is a tour edge.
    delta = ((d(e1) + d(e2)) + d(e3)) - ((d(a,a1) + d(b,b1)) + d(c,c1)), every d with the lower node id first;
    key = ((a*n + b)*n + c)*4 + type.
List neighbourhood: a removed edge (p, q = succ p) and two different new edges {p,u}, {q,w} with u in N(p), w in N(q); the
lists are directed, as stored.  Decision over the kinds: smallest delta < 0, ties -> lower kind (2-opt 0, Or-opt 1, 3-opt 2),
then lower key."""
import itertools

import numpy as np

import nl_opt_ref as NL

R = NL.R
NL_2OPT, NL_OROPT, NL_3OPT = 1, 2, 4


def n_moves(n):
    return 2 * n * (n - 2) * (n - 4) // 3 if n >= 5 else 0


def new_edges(T, a, a1, b, b1, c, c1):
    return (((a, b1), (c, a1), (b, c1)), ((a, b), (a1, c), (b1, c1)), ((a, c), (b1, a1), (b, c1)), ((a, b1), (c, b), (a1, c1)))[T]


def key(a, b, c, T, n):
    return ((a * n + b) * n + c) * 4 + T


def decode(k, n):
    T = k & 3
    k >>= 2
    return k // (n * n), (k // n) % n, k % n, T


def directed(nbr, n):
    """Nm[v, u] = u in N(v)"""
    nbr = np.asarray(nbr)
    Nm = np.zeros((n, n), dtype=bool)
    Nm[np.repeat(np.arange(n), nbr.shape[1]), nbr.reshape(-1)] = True
    return Nm


def _tour(succ):
    succ = np.asarray(succ, dtype=np.int64)
    order = R.tour_order(succ)
    pos = np.empty(len(succ), dtype=np.int64)
    pos[order] = np.arange(len(succ))
    return succ, order, pos


def _d(D, x, y):
    return D[np.minimum(x, y), np.maximum(x, y)]


def _evaluate(D, succ, pos, a, b, c, T):
    """arrays of (a, b, c) and a type -> (is a move, delta, key, the new edges)"""
    n = len(succ)
    a1, b1, c1 = succ[a], succ[b], succ[c]
    E = new_edges(T, a, a1, b, b1, c, c1)
    move = np.ones(len(a), dtype=bool)
    for x, y in E:
        gap = (pos[x] - pos[y]) % n
        move &= (gap != 1) & (gap != n - 1)
    delta = ((_d(D, *E[0]) + _d(D, *E[1])) + _d(D, *E[2])) - ((_d(D, a, a1) + _d(D, b, b1)) + _d(D, c, c1))
    return move, delta, key(a, b, c, T, n), E


def all_triples(succ):
    """every choice of three tour edges as (a, b, c) arrays: a the lowest tail, b and c after it in tour order"""
    succ, order, pos = _tour(succ)
    n = len(succ)
    idx = np.array(list(itertools.combinations(range(n), 3)), dtype=np.int64).reshape(-1, 3)
    t = order[idx]
    r = np.argmin(t, axis=1)
    rows = np.arange(len(idx))
    return t[rows, r], t[rows, (r + 1) % 3], t[rows, (r + 2) % 3]


def in_lists(Nm, succ, a, b, c, E):
    """the list rule for arrays of moves with new edges E"""
    ok = np.zeros(len(a), dtype=bool)
    for p in (a, b, c):
        q = succ[p]
        for i, j in itertools.permutations(range(3), 2):
            (xi, yi), (xj, yj) = E[i], E[j]
            at_p = ((xi == p) & Nm[p, yi]) | ((yi == p) & Nm[p, xi])
            at_q = ((xj == q) & Nm[q, yj]) | ((yj == q) & Nm[q, xj])
            ok |= at_p & at_q
    return ok


def moves(D, succ, nbr=None):
    """every move (of the list neighbourhood when nbr is given) -> (delta, key) arrays"""
    succ, order, pos = _tour(succ)
    n = len(succ)
    if n < 5:
        return np.zeros(0), np.zeros(0, dtype=np.int64)
    a, b, c = all_triples(succ)
    Nm = directed(nbr, n) if nbr is not None else None
    ds, ks = [], []
    for T in range(4):
        move, delta, k, E = _evaluate(D, succ, pos, a, b, c, T)
        if Nm is not None:
            move &= in_lists(Nm, succ, a, b, c, E)
        ds.append(delta[move])
        ks.append(k[move])
    return np.concatenate(ds), np.concatenate(ks)


def _best(delta, k):
    ok = delta < 0.0
    if not ok.any():
        return None
    delta, k = delta[ok], k[ok]
    m = delta.min()
    return (float(m), 2, int(k[delta == m].min()))


def decide3(D, succ, nbr):
    """the 3-opt kind alone, by brute force over all triples x 4 types, masked by the list rule"""
    return _best(*moves(D, succ, nbr))


def sparse_moves(D, succ, nbr, owners=None, with_owner=False):
    """The moves of the list neighbourhood as the kernel finds them: (p, k1, k2) and the <= 4 choices of the removed edges at
    u = nbr[p][k1] and w = nbr[succ p][k2] ((u, succ u) or (pred u, u); the same at w), the third new edge forced.  A move with a
    segment of one node has the same new edges as a second type (0 and 3 for S1, 0 and 2 for S2, 0 and 1 for S3): both are
    moves of the neighbourhood, so both are offered.  owners: the nodes p whose entries are walked (default: all).
    -> (delta, key) arrays, a move as often as it is reached; with_owner: (owner p, delta, key)"""
    succ, order, pos = _tour(succ)
    n = len(succ)
    own = np.arange(n) if owners is None else np.asarray(owners, dtype=np.int64)
    if n < 5 or len(own) == 0:
        none = np.zeros(0, dtype=np.int64)
        return ((none,) if with_owner else ()) + (np.zeros(0), none)
    nbr = np.asarray(nbr, dtype=np.int64)
    K = nbr.shape[1]
    pred = np.empty(n, dtype=np.int64)
    pred[succ] = np.arange(n)
    p, k1, k2, su, sw = [g.reshape(-1) for g in np.meshgrid(own, np.arange(K), np.arange(K), [0, 1], [0, 1], indexing="ij")]
    q = succ[p]
    u, w = nbr[p, k1], nbr[q, k2]

    def apart(x, y):   # two different nodes that are not tour neighbours
        gap = (pos[x] - pos[y]) % n
        return (gap != 0) & (gap != 1) & (gap != n - 1)

    tY, hY = np.where(su == 0, u, pred[u]), np.where(su == 0, succ[u], u)
    tZ, hZ = np.where(sw == 0, w, pred[w]), np.where(sw == 0, succ[w], w)
    yo, zo = np.where(su == 0, hY, tY), np.where(sw == 0, hZ, tZ)
    keep = apart(p, u) & apart(q, w) & apart(yo, zo) & (tY != p) & (tZ != p) & (tY != tZ)
    p, q, u, w, su, sw, tY, tZ = (v[keep] for v in (p, q, u, w, su, sw, tY, tZ))
    # roles 0, 1, 2 = a, b, c of the removed edges X = (p, q), Y, Z
    tails = np.stack([p, tY, tZ], axis=1)
    rows = np.arange(len(p))
    pa = pos[tails[rows, np.argmin(tails, axis=1)]]
    off = (pos[tails] - pa[:, None]) % n
    role = (off[:, :, None] > off[:, None, :]).sum(axis=2)
    rX, rY, rZ = role[:, 0], role[:, 1], role[:, 2]
    # slots: role * 2 + (0 tail, 1 head); the three new edges as a matching of the six slots
    partner = np.zeros((len(p), 6), dtype=np.int64)
    for s, t in ((rX * 2, rY * 2 + su), (rX * 2 + 1, rZ * 2 + sw), (rY * 2 + 1 - su, rZ * 2 + 1 - sw)):
        partner[rows, s] = t
        partner[rows, t] = s
    T = np.full(len(p), -1, dtype=np.int64)
    T[(partner[:, 0] == 3) & (partner[:, 4] == 1)] = 0
    T[(partner[:, 0] == 3) & (partner[:, 4] == 2)] = 3
    T[(partner[:, 0] == 2) & (partner[:, 1] == 4)] = 1
    T[(partner[:, 0] == 4) & (partner[:, 3] == 1)] = 2
    by_role = np.empty((len(p), 3), dtype=np.int64)
    by_role[rows[:, None], role] = tails
    a, b, c = by_role[:, 0], by_role[:, 1], by_role[:, 2]
    s1, s2, s3 = (pos[b] - pos[a]) % n, (pos[c] - pos[b]) % n, (pos[a] - pos[c]) % n
    ps, ds, ks = [], [], []
    for Tq in range(4):
        twin = (s1 == 1, s3 == 1, s2 == 1, s1 == 1)   # type Tq <-> its twin when that segment has one node
        if Tq == 0:
            sel = (T == 0) | ((T == 3) & (s1 == 1)) | ((T == 2) & (s2 == 1)) | ((T == 1) & (s3 == 1))
        else:
            sel = (T == Tq) | ((T == 0) & twin[Tq])
        move, delta, k, _ = _evaluate(D, succ, pos, a[sel], b[sel], c[sel], Tq)
        assert move.all()
        ps.append(p[sel])
        ds.append(delta)
        ks.append(k)
    return ((np.concatenate(ps),) if with_owner else ()) + (np.concatenate(ds), np.concatenate(ks))


def decide3_sparse(D, succ, nbr):
    return _best(*sparse_moves(D, succ, nbr))


def effective_kinds(kinds, n):
    low = NL.effective_kinds(kinds & 3, n)
    return low | (NL_3OPT if kinds & NL_3OPT and n >= 5 else 0)


def _decide(D, succ, nbr, kinds, three, low=None):
    n = len(succ)
    kinds = effective_kinds(kinds, n)
    best = (low or NL.decide)(D, succ, nbr, kinds & 3) if kinds & 3 else None
    if kinds & NL_3OPT:
        c = three(D, succ, nbr)
        if c is not None and NL._better(c, best):
            best = c
    return best


def decide(D, succ, nbr, kinds):
    """One decision over the enabled kinds -> (delta, kind, key) or None; the 3-opt kind by brute force."""
    return _decide(D, succ, nbr, kinds, decide3)


def decide_sparse(D, succ, nbr, kinds, low=None):
    """decide() with the 3-opt kind generated from the list entries, as the kernel walks them.  low(D, succ, nbr, kinds): the
    decision of the 2-opt and Or-opt kinds, nl_opt_ref.decide over the masked n x n matrices unless given."""
    return _decide(D, succ, nbr, kinds, decide3_sparse, low)


def apply_three_opt(succ, a, b, c, T):
    """the new tour of the table, in forward orientation"""
    succ = np.asarray(succ)

    def path(x, y):
        out = [int(x)]
        while out[-1] != y:
            out.append(int(succ[out[-1]]))
        return out

    S1, S2, S3 = path(succ[a], b), path(succ[b], c), path(succ[c], a)
    mid = (S2 + S1, S1[::-1] + S2[::-1], S2[::-1] + S1, S2 + S1[::-1])[T]
    seq = np.array(mid + S3, dtype=np.int32)
    out = np.empty(len(succ), dtype=np.int32)
    out[seq] = np.roll(seq, -1)
    return out


def new_counters():
    c = NL.new_counters()
    c["moves_3opt"] = 0
    c["moves_by_type"] = [0, 0, 0, 0]
    return c


def apply_decision(succ, d, c):
    if d[1] != 2:
        return NL.apply_decision(succ, d, c)
    a, b, cc, T = decode(d[2], len(succ))
    c["moves"] += 1
    c["moves_3opt"] += 1
    c["moves_by_type"][T] += 1
    return apply_three_opt(succ, a, b, cc, T)


def descent(D, succ, nbr, kinds, max_moves=-1, sparse=True, trace=None, low=None):
    """-> (succ', counters as tsp_nl3_opt_stats without deltas_executed and the times); trace: a list that receives the decisions;
    low: see decide_sparse (for sizes at which the masked matrices take seconds per decision)"""
    succ = np.array(succ, dtype=np.int32, copy=True)
    c = new_counters()
    if effective_kinds(kinds, len(succ)) == 0:
        return succ, c
    assert sparse or low is None
    fn = (lambda *a: decide_sparse(*a, low=low)) if sparse else decide
    while max_moves < 0 or c["moves"] < max_moves:
        c["decisions"] += 1
        d = fn(D, succ, nbr, kinds)
        if d is None:
            break
        if trace is not None:
            trace.append(d)
        succ = apply_decision(succ, d, c)
    return succ, c
