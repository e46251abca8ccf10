"""CPU reference of the batched list descent of include/tsp_hip.h (tsp_dev_nl_3opt_batch), built on the list entries as the
kernels walk them (nl_opt_ref.entry_moves, nl3_opt_ref.sparse_moves with owners).  A helper of the tests, not collected by pytest.

A move is (delta, kind, key) with kind 0 2-opt, 1 Or-opt, 2 3-opt: tuples compare as the device's (delta, key with the kind bits).
Positions are along the successor orientation from node 0; arcs and their disjointness do not depend on that origin."""
import numpy as np

import nl3_opt_ref as N3

NL = N3.NL
R = NL.R


def tour(succ):
    succ = np.asarray(succ, dtype=np.int64)
    order = R.tour_order(succ)
    n = len(succ)
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    pred = np.empty(n, dtype=np.int64)
    pred[succ] = np.arange(n)
    return succ, order, pos, pred


def arc(move, pos, n):
    """(start, len) of the rule, len clipped to n"""
    _, kind, key = move
    if kind == 0:
        i, j = key // n, key % n
        start, ln = int(pos[i]), int((pos[j] - pos[i]) % n) + 2
    elif kind == 2:
        a, _, c, _ = N3.decode(key, n)
        start, ln = int(pos[a]), int((pos[c] - pos[a]) % n) + 2
    else:
        f, L, a, _ = R.decode(key, n)
        m1 = int((pos[a] - (pos[f] + L)) % n) + 1   # nodes s .. a
        m2 = n - L - m1                             # nodes b .. p
        if m1 <= m2:
            start, ln = int((pos[f] - 1) % n), m1 + L + 2
        else:
            start, ln = int(pos[a]), m2 + L + 2
    return start, min(ln, n)


def disjoint(x, y, n):
    (s1, l1), (s2, l2) = x, y
    return (s2 - s1) % n >= l1 and (s1 - s2) % n >= l2


def positions(a, n):
    return [(a[0] + q) % n for q in range(a[1])]


def removed_ends(move, succ, pred, n):
    """the tails and heads of the edges the move removes"""
    _, kind, key = move
    if kind == 0:
        i, j = key // n, key % n
        return [i, int(succ[i]), j, int(succ[j])]
    if kind == 2:
        a, b, c, _ = N3.decode(key, n)
        return [a, int(succ[a]), b, int(succ[b]), c, int(succ[c])]
    f, L, a, _ = R.decode(key, n)
    l = f
    for _ in range(L - 1):
        l = int(succ[l])
    return [int(pred[f]), f, l, int(succ[l]), a, int(succ[a])]


def arc_lens(kind, key, pos, n):
    """arc(...)[1] for arrays of moves"""
    ln = np.empty(len(key), dtype=np.int64)
    two, three, oro = kind == 0, kind == 2, kind == 1
    k = key[two]
    ln[two] = (pos[k % n] - pos[k // n]) % n + 2
    k = key[three] >> 2
    ln[three] = (pos[k % n] - pos[k // (n * n)]) % n + 2
    t = key[oro] >> 1
    fl = t // n
    L = fl % 3 + 1
    m1 = (pos[t % n] - (pos[fl // 3] + L)) % n + 1
    ln[oro] = np.minimum(m1, n - L - m1) + L + 2
    return np.minimum(ln, n)


def improving_arrays(D, succ, nbr, kinds):
    """every improving move as the lanes of the scans reach it -> arrays (owner, delta, kind, key), a move as often as reached"""
    succ, order, pos, pred = tour(succ)
    n = len(succ)
    kinds = N3.effective_kinds(kinds, n)
    nbr = np.asarray(nbr, dtype=np.int64)
    out = [(np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))]
    v = np.repeat(np.arange(n, dtype=np.int64), nbr.shape[1])
    u = nbr.reshape(-1)
    v, u = v[v != u], u[v != u]
    d = lambda a, b: D[np.minimum(a, b), np.maximum(a, b)]   # noqa: E731
    found = []
    for kind in (0, 1):
        if kinds & (1, 2)[kind]:
            found += [(kind,) + m for m in NL.entry_moves(v, u, succ, order, pos, pred, d, kind)]
    if kinds & 4:
        found.append((2,) + N3.sparse_moves(D, succ, nbr, with_owner=True))
    for kind, own, delta, key in found:
        q = np.nonzero(delta < 0.0)[0]
        out.append((np.asarray(own)[q], np.asarray(delta, dtype=np.float64)[q], np.full(len(q), kind), np.asarray(key)[q]))
    return tuple(np.concatenate(col) for col in zip(*out))


def improving_moves(D, succ, nbr, kinds):
    """improving_arrays as a list of (owner, (delta, kind, key))"""
    own, delta, kind, key = improving_arrays(D, succ, nbr, kinds)
    return [(int(o), (float(d), int(t), int(k))) for o, d, t, k in zip(own, delta, kind, key)]


def candidates(D, succ, nbr, kinds, max_arc):
    """-> ({node: its best move of an arc of at most max_arc positions}, the overall best move or None)"""
    _, _, pos, _ = tour(succ)
    n = len(succ)
    own, delta, kind, key = improving_arrays(D, succ, nbr, kinds)
    if len(own) == 0:
        return {}, None
    at = np.lexsort((key, kind, delta))          # by (delta, kind, key), as the tuples compare
    best = (float(delta[at[0]]), int(kind[at[0]]), int(key[at[0]]))
    at = at[arc_lens(kind, key, pos, n)[at] <= max_arc]
    cand = {}
    for o, d, t, k in zip(own[at], delta[at], kind[at], key[at]):
        cand.setdefault(int(o), (float(d), int(t), int(k)))    # sorted: a node's first move is its best
    return cand, best


def select(cand, pos, n, rounds):
    """the claim rounds over the per-node candidates -> the accepted moves in (delta, key) order"""
    live = dict(cand)
    accepted = set()
    for _ in range(rounds):
        if not live:
            break
        holder = {}
        for m in live.values():
            for p in positions(arc(m, pos, n), n):
                if p not in holder or m < holder[p]:
                    holder[p] = m
        won = {m for m in live.values() if all(holder[p] == m for p in positions(arc(m, pos, n), n))}
        accepted |= won
        arcs = [arc(m, pos, n) for m in won]
        live = {v: m for v, m in live.items() if all(disjoint(arc(m, pos, n), a, n) for a in arcs)}
    return sorted(accepted)


def greedy(cand, pos, n):
    """the sequential greedy selection by (delta, key) over the candidates"""
    out, arcs = [], []
    for m in sorted(set(cand.values())):
        a = arc(m, pos, n)
        if all(disjoint(a, b, n) for b in arcs):
            out.append(m)
            arcs.append(a)
    return out


def decision(D, succ, nbr, kinds, max_arc, rounds):
    """-> the moves of one decision in (delta, key) order ([] ends the descent)"""
    cand, best = candidates(D, succ, nbr, kinds, max_arc)
    if not cand:
        return [] if best is None else [best]
    _, _, pos, _ = tour(succ)
    return select(cand, pos, len(succ), rounds)


def normal(n, max_arc, rounds, default_rounds=2):
    """max_arc and rounds as the entry point reads them"""
    max_arc = n // 2 if max_arc <= 0 else min(max_arc, n)
    rounds = default_rounds if rounds <= 0 else min(rounds, n)
    return max_arc, rounds


def descent(D, succ, nbr, kinds, max_arc, rounds, max_moves=-1, trace=None):
    """max_arc and rounds are taken literally (max_arc = 0: no candidates, every decision falls back to the single best move).
    -> (succ', counters as tsp_nl3_opt_stats without deltas_executed and the times); trace receives every decision's moves"""
    succ = np.array(succ, dtype=np.int32, copy=True)
    c = N3.new_counters()
    if N3.effective_kinds(kinds, len(succ)) == 0:
        return succ, c
    while max_moves < 0 or c["moves"] < max_moves:
        c["decisions"] += 1
        moves = decision(D, succ, nbr, kinds, max_arc, rounds)
        if not moves:
            break
        if max_moves >= 0:
            moves = moves[:max_moves - c["moves"]]
        if trace is not None:
            trace.append(list(moves))
        for m in moves:
            succ = N3.apply_decision(succ, m, c)
    return succ, c
