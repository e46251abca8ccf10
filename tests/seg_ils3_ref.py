"""CPU reference of the windowed iterated local search with the 3-opt kind (include/tsp_hip.h, tsp_dev_seg_ils3), on top of
seg_ils_ref.py: the window filter gains kind 2 (all three decoded tails at slots 0 .. W - 2), the window move carries the 3-opt
counters through, and trial / run are restated over these two.  dlb_ref.candidates and dlb_ref.ends already know kind 2.  A
helper of the tests, not collected by pytest."""
import numpy as np

import dlb_ref as DL
import nl3_opt_ref as N3
import seg_ils_ref as SR

COUNTERS = SR.COUNTERS + ("moves_3opt", "moves_by_type")


def is_window_move(succ, slot, W, kind, key):
    if kind != 2:
        return SR.is_window_move(succ, slot, W, kind, key)
    a, b, c, _ = N3.decode(int(key), len(succ))
    return bool(all(0 <= slot[x] <= W - 2 for x in (a, b, c)))


def window_candidates(D, succ, nbr, kinds, active, seq):
    """dlb_ref.candidates cut down to the window moves of the window `seq` -> (owner, delta, kind, key) arrays"""
    own, delta, kind, key = DL.candidates(D, succ, nbr, kinds, active)
    slot = SR._slots(len(succ), seq)
    keep = np.array([is_window_move(succ, slot, len(seq), int(kd), int(k)) for kd, k in zip(kind, key)], dtype=bool)
    if len(keep) == 0:
        return own, delta, kind, key
    return own[keep], delta[keep], kind[keep], key[keep]


def apply_window_move(succ, d, seq, c=None):
    """seg_ils_ref.apply_window_move; a 3-opt move is nl3_opt_ref's, the tour turned back when the move turned the outside of the
    window round, and counts in moves, moves_3opt and moves_by_type alone -> succ'.  c: counters."""
    if d[1] != 2:
        return SR.apply_window_move(succ, d, seq, c)
    n = len(succ)
    last, out = seq[-1], int(succ[seq[-1]])
    tmp = N3.new_counters()
    new = N3.apply_decision(succ, d, tmp)
    if int(new[last]) != out:
        back = np.empty(n, dtype=np.int32)
        back[new] = np.arange(n, dtype=np.int32)
        new = back
    if c is not None:
        c["moves"] += tmp["moves"]
        c["moves_3opt"] += tmp["moves_3opt"]
        c["moves_by_type"] = [x + y for x, y in zip(c["moves_by_type"], tmp["moves_by_type"])]
    return new


def new_counters():
    c = SR.new_counters()
    c["moves_3opt"] = 0
    c["moves_by_type"] = [0, 0, 0, 0]
    return c


def relabel(seq, cur_succ, d):
    """(r, type) of the 3-opt move d on the window `seq`: r = 0, 1, 2 where a sits at the lowest, middle, highest of the three
    tails' slots"""
    a, b, c, T = N3.decode(int(d[2]), len(cur_succ))
    slot = SR._slots(len(cur_succ), seq)
    return sorted(int(slot[x]) for x in (a, b, c)).index(int(slot[a])), T


def trial(D, succ, nbr, kinds, seq, v, S, cap, c, log=None):
    """One trial of the window seq of the tour succ -> (succ', seq', accepted)"""
    n, W = len(succ), len(seq)
    c0 = SR.window_cost(D, seq)
    kicked, e = SR.kick(seq, S, v)
    work = SR.set_path(succ, kicked)
    A = np.zeros(n, dtype=bool)
    A[e] = True
    moves = 0
    applied = []
    while cap < 0 or moves < cap:
        c["decisions"] += 1
        c["active_nodes"] += int(A.sum())
        cur = SR.walk(work, seq[0], W)
        own, delta, kind, key = window_candidates(D, work, nbr, kinds, A, cur)
        if len(own) == 0:
            break
        hit = np.zeros(n, dtype=bool)
        hit[own] = True
        m = delta.min()
        kd = kind[delta == m].min()
        d = (float(m), int(kd), int(key[(delta == m) & (kind == kd)].min()))
        ends = DL.ends(work, d)
        if kd == 2:
            applied.append(relabel(cur, work, d))
        work = apply_window_move(work, d, cur, c)
        A = hit
        A[ends] = True
        moves += 1
    cur = SR.walk(work, seq[0], W)
    c1 = SR.window_cost(D, cur)
    ok = c1 < c0
    if log is not None:
        log.append({"c0": c0, "c1": c1, "accepted": ok, "seq": list(seq), "kicked": kicked, "moves": moves, "three": applied})
    c["accepted"] += int(ok)
    return (work, cur, True) if ok else (succ, seq, False)


def run(D, succ, nbr, kinds, seed, b, iterations, window=0, span=0, trials=1, max_moves=-1, order=None, log=None):
    """tsp_dev_seg_ils3 of one chain -> (succ', cost, stats without deltas_executed and the times).  order, log: as
    seg_ils_ref.run; a log record also has "three", the (r, type) of the trial's 3-opt moves in the order applied."""
    succ = np.array(succ, dtype=np.int32, copy=True)
    n = len(succ)
    c = new_counters()
    c["start_cost"] = SR.IR.cost(D, succ)
    if n < 10:
        return succ, c["start_cost"], c
    W, S = SR.resolve(n, window, span)
    c["windows"] = n // W
    for it in range(iterations):
        wins = SR.windows(succ, seed, b, it, W)
        for w in (order(it, len(wins)) if order else range(len(wins))):
            seq = wins[w]
            for t in range(trials):
                mark = len(log) if log is not None else 0
                succ, seq, _ = trial(D, succ, nbr, kinds, seq, SR.trial_draws(seed, b, it, w, trials, t), S, max_moves, c, log)
                if log is not None:
                    log[mark].update({"it": it, "w": w, "t": t})
                c["trials"] += 1
        c["iterations"] += 1
    return succ, SR.IR.cost(D, succ), c
