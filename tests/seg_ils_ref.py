"""CPU reference of the windowed iterated local search of include/tsp_hip.h (tsp_dev_seg_ils), on top of dlb_ref.candidates /
ends, the family's apply_decision and ils_ref's mix.  A helper of the tests, not collected by pytest.

A window is a list of W nodes along succ.  cand(v) of the active nodes is computed on the whole tour, as the family does, and
then cut down to window moves: every removed edge is a window edge (and an Or-opt segment is a window path).  A move is applied
by the family's apply_decision; when that turned the part of the tour outside the window round (succ[last] != out) the whole
tour is turned back.  O(n K) and more per decision."""
import numpy as np

import dlb_ref as DL
import ils_ref as IR
import nl3_opt_ref as N3
import nl_opt_ref as NL

R = NL.R
MAX_WINDOW, DEFAULT_WINDOW = 2048, 1024
COUNTERS = ("decisions", "moves", "moves_2opt", "moves_oropt", "moves_by_len", "moves_reversed", "reversed", "iterations",
            "windows", "trials", "accepted", "active_nodes")


def base(seed, b, it):
    return IR.mix((IR.mix((seed & IR.M64) ^ ((b * IR.CHAIN) & IR.M64)) + it) & IR.M64)


def anchor(n, seed, b, it):
    return IR.mix(base(seed, b, it)) % n


def resolve(n, window=0, span=0):
    """-> (W, S) of a call's arguments; None where they are a bad argument"""
    W = min(DEFAULT_WINDOW, n - 1) if window <= 0 else window
    if W < 9 or W > min(MAX_WINDOW, n - 1):
        return None
    S = W - 1 if span <= 0 else span
    if S < 8 or S > W - 1:
        return None
    return W, S


def walk(succ, v, count):
    seq = [int(v)]
    for _ in range(count - 1):
        seq.append(int(succ[seq[-1]]))
    return seq


def windows(succ, seed, b, it, W):
    """seq_w of the M windows of iteration `it`"""
    n = len(succ)
    M = n // W
    seq = walk(succ, anchor(n, seed, b, it), M * W)
    return [seq[w * W:(w + 1) * W] for w in range(M)]


def trial_draws(seed, b, it, w, T, t):
    bw = IR.mix((base(seed, b, it) + 8 + int(w) * T + t) & IR.M64)
    return [IR.mix((bw + j) & IR.M64) for j in range(5)]


def window_cost(D, seq):
    W = len(seq)
    P = 1
    while P < W - 1:
        P *= 2
    a, c = np.asarray(seq[:-1]), np.asarray(seq[1:])
    x = np.zeros(P, dtype=np.float64)
    x[:W - 1] = D[np.minimum(a, c), np.maximum(a, c)]
    h = P // 2
    while h >= 1:
        x[:h] = x[:h] + x[h:2 * h]
        h //= 2
    return float(x[0])


def kick(seq, S, v):
    """-> (the kicked window, the eight ends of its cuts read before the kick)"""
    W = len(seq)
    off = v[0] % (W - S)
    _, o1, o2, o3, o4 = IR.cuts(S, S, [0] + list(v[1:5]))
    assert off + o4 <= W - 1
    q = seq[off:]
    new = seq[:off] + q[:o1] + q[o3:o4] + q[o2:o3] + q[o1:o2] + q[o4:]
    ends = [q[o + d] for o in (o1, o2, o3, o4) for d in (-1, 0)]
    return new, ends


def set_path(succ, seq):
    succ = np.array(succ, dtype=np.int32, copy=True)
    succ[seq[:-1]] = seq[1:]
    return succ


def _slots(n, seq):
    slot = np.full(n, -1, dtype=np.int64)
    slot[seq] = np.arange(len(seq))
    return slot


def is_window_move(succ, slot, W, kind, key):
    n = len(succ)
    tail = lambda x: 0 <= slot[x] <= W - 2   # noqa: E731  (x, succ x) is a window edge
    if kind == 0:
        return bool(tail(key // n) and tail(key % n))
    f, L, a, _ = R.decode(int(key), n)
    p = int(np.flatnonzero(succ == f)[0])
    l = walk(succ, f, L)[-1]
    return bool(tail(p) and tail(l) and tail(a) and slot[l] == slot[f] + L - 1)


def window_candidates(D, succ, nbr, kinds, active, seq):
    """dlb_ref.candidates cut down to the window moves of the window `seq` -> (owner, delta, kind, key) arrays"""
    own, delta, kind, key = DL.candidates(D, succ, nbr, kinds, active)
    slot = _slots(len(succ), seq)
    keep = np.array([is_window_move(succ, slot, len(seq), int(kd), int(k)) for kd, k in zip(kind, key)], dtype=bool)
    if len(keep) == 0:
        return own, delta, kind, key
    return own[keep], delta[keep], kind[keep], key[keep]


def apply_window_move(succ, d, seq, c=None):
    """The family's move, the tour turned back when the move turned the outside of the window round -> succ'.  c: counters."""
    n = len(succ)
    last, out = seq[-1], int(succ[seq[-1]])
    tmp = N3.new_counters()
    new = N3.apply_decision(succ, d, tmp)
    if int(new[last]) != out:
        back = np.empty(n, dtype=np.int32)
        back[new] = np.arange(n, dtype=np.int32)
        new = back
    if d[1] == 0:
        slot = _slots(n, seq)
        tmp["reversed"] = abs(int(slot[d[2] // n]) - int(slot[d[2] % n]))   # the nodes of the reversed window sub-path
    if c is not None:
        for k in ("moves", "moves_2opt", "moves_oropt", "moves_reversed", "reversed"):
            c[k] += tmp[k]
        c["moves_by_len"] = [x + y for x, y in zip(c["moves_by_len"], tmp["moves_by_len"])]
    return new


def new_counters():
    c = {k: 0 for k in COUNTERS}
    c["moves_by_len"] = [0, 0, 0]
    return c


def trial(D, succ, nbr, kinds, seq, v, S, cap, c, log=None):
    """One trial of the window seq of the tour succ -> (succ', seq', accepted)"""
    n, W = len(succ), len(seq)
    c0 = window_cost(D, seq)
    kicked, e = kick(seq, S, v)
    work = set_path(succ, kicked)
    A = np.zeros(n, dtype=bool)
    A[e] = True
    moves = 0
    while cap < 0 or moves < cap:
        c["decisions"] += 1
        c["active_nodes"] += int(A.sum())
        cur = walk(work, seq[0], W)
        own, delta, kind, key = window_candidates(D, work, nbr, kinds, A, cur)
        if len(own) == 0:
            break
        hit = np.zeros(n, dtype=bool)
        hit[own] = True
        m = delta.min()
        kd = kind[delta == m].min()
        d = (float(m), int(kd), int(key[(delta == m) & (kind == kd)].min()))
        ends = DL.ends(work, d)
        work = apply_window_move(work, d, cur, c)
        A = hit
        A[ends] = True
        moves += 1
    cur = walk(work, seq[0], W)
    c1 = window_cost(D, cur)
    ok = c1 < c0
    if log is not None:
        log.append({"c0": c0, "c1": c1, "accepted": ok, "seq": list(seq), "kicked": kicked, "moves": moves})
    c["accepted"] += int(ok)
    return (work, cur, True) if ok else (succ, seq, False)


def run(D, succ, nbr, kinds, seed, b, iterations, window=0, span=0, trials=1, max_moves=-1, order=None, log=None):
    """tsp_dev_seg_ils of one chain -> (succ', cost, stats without deltas_executed and the times).  order(it, M): the order in
    which the windows of an iteration are processed (default 0 .. M-1).  log: a list that takes one record per trial."""
    succ = np.array(succ, dtype=np.int32, copy=True)
    n = len(succ)
    c = new_counters()
    c["start_cost"] = IR.cost(D, succ)
    if n < 10:
        return succ, c["start_cost"], c
    W, S = resolve(n, window, span)
    c["windows"] = n // W
    for it in range(iterations):
        wins = windows(succ, seed, b, it, W)
        for w in (order(it, len(wins)) if order else range(len(wins))):
            seq = wins[w]
            for t in range(trials):
                mark = len(log) if log is not None else 0
                succ, seq, _ = trial(D, succ, nbr, kinds, seq, trial_draws(seed, b, it, w, trials, t), S, max_moves, c, log)
                if log is not None:
                    log[mark].update({"it": it, "w": w, "t": t})
                c["trials"] += 1
        c["iterations"] += 1
    return succ, IR.cost(D, succ), c
