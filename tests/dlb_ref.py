"""CPU reference of the don't-look bits of include/tsp_hip.h (tsp_dev_nl_3opt_dlb, tsp_dev_ils_dlb), numpy over the oracle's
distance matrix, on top of nl3_opt_ref.py / nl_opt_ref.py / ils_ref.py.  A helper of the tests, not collected by pytest.

cand(v) is gathered through the n x K lists: every delta expression of the three kinds is evaluated as an array over the
entries (v, k) of the active nodes (the entries of the full delta matrices those lanes look at), never one masked decision per
node.  A candidate is (owner v, delta, kind, key); the decision is the smallest (delta, kind, key) among delta < 0, and the
owners of the improving candidates are the nodes that stay active."""
import numpy as np

import ils_ref as IR
import nl3_opt_ref as N3
import nl_opt_ref as NL

R = NL.R
OFF, ON, CLOSE = 0, 1, 2
COUNTERS = IR.NL_COUNTERS + ("active_nodes", "closing_scans")


def _d(D, x, y):
    return D[np.minimum(x, y), np.maximum(x, y)]


def _tour(succ):
    succ = np.asarray(succ, dtype=np.int64)
    n = len(succ)
    order = R.tour_order(succ)
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    pred = np.empty(n, dtype=np.int64)
    pred[succ] = np.arange(n)
    return succ, order, pos, pred


def candidates(D, succ, nbr, kinds, active):
    """The improving candidates of the active nodes -> (owner, delta, kind, key) arrays."""
    succ, order, pos, pred = _tour(succ)
    n = len(succ)
    kinds = N3.effective_kinds(kinds, n)
    nbr = np.asarray(nbr, dtype=np.int64)
    K = nbr.shape[1]
    act = np.flatnonzero(np.asarray(active))
    v = np.repeat(act, K)
    u = nbr[act].reshape(-1)
    ok = u != v
    v, u = v[ok], u[ok]
    d = lambda x, y: _d(D, x, y)   # noqa: E731
    found = []
    for kind in (0, 1):
        if kinds & (N3.NL_2OPT, N3.NL_OROPT)[kind]:
            found += [(kind,) + c for c in NL.entry_moves(v, u, succ, order, pos, pred, d, kind)]
    if kinds & N3.NL_3OPT:
        found.append((2,) + N3.sparse_moves(D, succ, nbr, owners=act, with_owner=True))
    own = np.concatenate([c[1] for c in found] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    delta = np.concatenate([c[2] for c in found] + [np.zeros(0)])
    kind = np.concatenate([np.full(len(c[1]), c[0], dtype=np.int64) for c in found] + [np.zeros(0, dtype=np.int64)])
    key = np.concatenate([np.asarray(c[3], dtype=np.int64) for c in found] + [np.zeros(0, dtype=np.int64)])
    imp = delta < 0.0
    return own[imp], delta[imp], kind[imp], key[imp]


def decide(D, succ, nbr, kinds, active):
    """One decision over the active set -> ((delta, kind, key) or None, the bool array of the nodes v with m_v.delta < 0)"""
    own, delta, kind, key = candidates(D, succ, nbr, kinds, active)
    hit = np.zeros(len(succ), dtype=bool)
    if len(own) == 0:
        return None, hit
    hit[own] = True
    m = delta.min()
    sel = delta == m
    kd = kind[sel].min()
    return (float(m), int(kd), int(key[sel & (kind == kd)].min())), hit


def ends(succ, d):
    """the tails and heads of the edges that the move removes, in the tour before the move"""
    succ = np.asarray(succ)
    n = len(succ)
    _, kind, key = d
    if kind == 0:
        t = [key // n, key % n]
    elif kind == 1:
        f, L, a, o = R.decode(key, n)
        l = f
        for _ in range(L - 1):
            l = int(succ[l])
        t = [int(np.flatnonzero(succ == f)[0]), l, a]
    else:
        t = list(N3.decode(key, n)[:3])
    return sorted({int(x) for x in t} | {int(succ[x]) for x in t})


def new_counters():
    c = N3.new_counters()
    c["active_nodes"] = 0
    c["closing_scans"] = 0
    return c


def descent(D, succ, nbr, kinds, mode, active=None, max_moves=-1, trace=None):
    """-> (succ', counters as tsp_nl_dlb_stats without deltas_executed and the times, the active set at the end)"""
    succ = np.array(succ, dtype=np.int32, copy=True)
    n = len(succ)
    if mode == OFF:
        s, c = N3.descent(D, succ, nbr, kinds, max_moves=max_moves, sparse=True)
        c["active_nodes"] = c["closing_scans"] = 0
        return s, c, np.ones(n, dtype=bool)
    A = np.ones(n, dtype=bool) if active is None else (np.asarray(active).reshape(n) != 0)
    c = new_counters()
    if N3.effective_kinds(kinds, n) == 0:
        return succ, c, A
    while max_moves < 0 or c["moves"] < max_moves:
        c["decisions"] += 1
        c["active_nodes"] += int(A.sum())
        full = bool(A.all())
        d, hit = decide(D, succ, nbr, kinds, A)
        if trace is not None:
            trace.append((d, int(A.sum())))
        if d is not None:
            e = ends(succ, d)
            succ = N3.apply_decision(succ, d, c)
            A = hit
            A[e] = True
        elif mode == ON or full:
            break
        else:
            A = np.ones(n, dtype=bool)
            c["closing_scans"] += 1
    return succ, c, A


def kick_nodes(succ, seed, b, it, span):
    """the active set behind the kick of iteration `it`: seq[o - 1] and seq[o mod n] of the four cuts, as a bool array"""
    succ = np.asarray(succ)
    n = len(succ)
    s, o1, o2, o3, o4 = IR.cuts(n, span, IR.draws(seed, b, it))
    seq = [s]
    for _ in range(n - 1):
        seq.append(int(succ[seq[-1]]))
    A = np.zeros(n, dtype=bool)
    for o in (o1, o2, o3, o4):
        A[seq[o - 1]] = True
        A[seq[o % n]] = True
    return A


def chain(D, succ, nbr, kinds, seed, b, iterations, span=0, mode=ON, max_moves=-1):
    """ils_ref.chain with every descent under `mode` -> (succ', cost, stats with active_nodes and closing_scans)"""
    n = len(succ)
    total = new_counters()

    def add(c):
        IR._add(total, c)
        total["active_nodes"] += c["active_nodes"]
        total["closing_scans"] += c["closing_scans"]

    inc, c, _ = descent(D, succ, nbr, kinds, mode, max_moves=max_moves)
    add(c)
    best = IR.cost(D, inc)
    st = {"iterations": 0, "accepted": 0, "last_improved": -1, "start_cost": best}
    if n >= 8:
        for it in range(iterations):
            A = kick_nodes(inc, seed, b, it, span) if mode != OFF else None
            work, c, _ = descent(D, IR.kick(inc, seed, b, it, span), nbr, kinds, mode, active=A, max_moves=max_moves)
            add(c)
            cw = IR.cost(D, work)
            if cw < best:
                inc, best = work, cw
                st["accepted"] += 1
                st["last_improved"] = it
            st["iterations"] += 1
    st.update(total)
    return inc, best, st
