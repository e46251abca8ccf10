"""CPU reference of the windowed iterated local search with Lin-Kernighan chains (include/tsp_hip.h, tsp_dev_seg_ils_lk), on top
of seg_groups_ref.py / seg_ils3_ref.py / seg_ils_ref.py: a chain is a variable-depth sequence of reversals on a private copy of
the window path, kept up to its best prefix, and a fourth kind (index 3) of the window repair.  The chain is written here from the
header's text, not from csrc/seg_lk.hpp: it reverses a real list.  trial, window_groups and run are restated over it.  A helper of
the tests, not collected by pytest."""
import numpy as np

import dlb_ref as DL
import seg_groups_ref as SG
import seg_ils3_ref as S3
import seg_ils_ref as SR

NL_LK = 8
MAX_DEPTH, DEFAULT_DEPTH = 16, 16
LK_COUNTERS = ("lk_depth", "moves_lk", "lk_flips", "lk_chains", "lk_steps")
COUNTERS = SG.COUNTERS + LK_COUNTERS


def _d(D, a, b):
    return np.float64(D[min(a, b), max(a, b)])


def resolve_depth(depth):
    """D of a call's argument; None where it is a bad argument"""
    if depth <= 0:
        return DEFAULT_DEPTH
    return depth if depth <= MAX_DEPTH else None


def chain(D, nbr, seq, i, depth, slots=None):
    """Side 0 of the chain of the node at slot i of the window path seq -> None without a first edge, else a dict: steps (all
    reversals made), hstar, best, and per step h = 1 .. steps: e, y, p, j (1-based lists with a dummy at 0), G.  slots: the slot
    of every node of seq, when the caller has it."""
    W = len(seq)
    if i > W - 2:
        return None
    cur = list(seq)
    slot = dict(slots) if slots is not None else {v: k for k, v in enumerate(cur)}   # of cur, kept up with every reversal
    t1 = cur[i]
    G = np.float64(0.0)
    best = np.float64(0.0)
    hstar = 0
    used = set()
    es, ys, ps, js, Gs = [None], [None], [None], [None], [None]
    for h in range(1, depth + 1):
        e = cur[i + 1]
        x = _d(D, t1, e)
        pick = None
        for k in range(nbr.shape[1]):
            y = int(nbr[e][k])
            if y == e or y not in slot or y in used:
                continue
            j = slot[y]
            if not (i + 3 <= j <= W - 1):
                continue
            g1 = (G + x) - _d(D, e, y)
            if not g1 > best:
                continue
            p = cur[j - 1]
            g2 = g1 + _d(D, p, y)
            if pick is None or g2 > pick[0]:
                pick = (g2, k, j, y, p)
        if pick is None:
            break
        g2, _, j, y, p = pick
        cur[i + 1:j] = cur[i + 1:j][::-1]
        for k in range(i + 1, j):
            slot[cur[k]] = k
        used |= {e, y}
        es.append(e); ys.append(y); ps.append(p); js.append(j)
        G = g2 - _d(D, p, t1)
        Gs.append(G)
        if G > best:
            best, hstar = G, h
    return {"t1": t1, "steps": len(js) - 1, "hstar": hstar, "best": float(best), "e": es, "y": ys, "p": ps, "j": js, "G": Gs}


def side_chain(D, nbr, seq, v, s, depth, sides=None):
    """chain(v, s) on the window seq: side 1 is side 0 on the window read backwards -> (chain or None, the intervals (lo, hi) of
    its first hstar reversals in the slots of seq).  sides: read_both(seq), when the caller has it."""
    W = len(seq)
    path, slots = (sides or read_both(seq))[s]
    i = slots[v]
    c = chain(D, nbr, path, i, depth, slots)
    if c is None:
        return None, []
    iv = [(i + 1, c["j"][h] - 1) for h in range(1, c["hstar"] + 1)]
    if s == 1:
        iv = [(W - 1 - hi, W - 1 - lo) for lo, hi in iv]
    return c, iv


def read_both(seq):
    """the window read forwards and backwards, each with the slots of its nodes"""
    fwd, bwd = list(seq), list(seq)[::-1]
    return (fwd, {v: k for k, v in enumerate(fwd)}), (bwd, {v: k for k, v in enumerate(bwd)})


def apply_intervals(seq, iv):
    new = list(seq)
    for lo, hi in iv:
        new[lo:hi + 1] = new[lo:hi + 1][::-1]
    return new


def chain_ends(c):
    return sorted({c["t1"]} | {x for h in range(1, c["hstar"] + 1) for x in (c["e"][h], c["y"][h], c["p"][h])})


def new_counters():
    c = SG.new_counters()
    c.update({k: 0 for k in LK_COUNTERS})
    return c


def trial(D, succ, nbr, kinds, depth, seq, v, S, cap, c, log=None):
    """One trial of the window seq of the tour succ -> (succ', seq', accepted).  log: takes ("decision", |A|) per decision and
    ("chain", t1, s, hstar, intervals) per applied chain."""
    if not kinds & NL_LK:
        return S3.trial(D, succ, nbr, kinds, seq, v, S, cap, c)
    n, W = len(succ), len(seq)
    older = kinds & 7
    c0 = SR.window_cost(D, seq)
    kicked, e = SR.kick(seq, S, v)
    work = SR.set_path(succ, kicked)
    A = np.zeros(n, dtype=bool)
    A[e] = True
    moves = 0
    while cap < 0 or moves < cap:
        c["decisions"] += 1
        c["active_nodes"] += int(A.sum())
        if log is not None:
            log.append(("decision", int(A.sum())))
        cur = SR.walk(work, seq[0], W)
        hit = np.zeros(n, dtype=bool)
        best = None                      # (delta, kind, key, payload)
        if older:
            own, delta, kind, key = S3.window_candidates(D, work, nbr, older, A, cur)
            if len(own):
                hit[own] = True
                m = delta.min()
                kd = kind[delta == m].min()
                best = (float(m), int(kd), int(key[(delta == m) & (kind == kd)].min()), None)
        sides = read_both(cur)
        for node in np.flatnonzero(A):
            node = int(node)
            assert node in sides[0][1]
            for s in (0, 1):
                ch, iv = side_chain(D, nbr, cur, node, s, depth, sides)
                if ch is None:
                    continue
                c["lk_chains"] += 1
                c["lk_steps"] += ch["steps"]
                if ch["hstar"] >= 1:
                    hit[node] = True
                    cand = (-ch["best"], 3, 2 * node + s, (ch, iv, s))
                    if best is None or cand[:3] < best[:3]:
                        best = cand
        if best is None:
            break
        if best[1] == 3:
            ch, iv, s = best[3]
            ends = chain_ends(ch)
            work = SR.set_path(work, apply_intervals(cur, iv))
            c["moves"] += 1
            c["moves_lk"] += 1
            c["lk_flips"] += ch["hstar"]
            if log is not None:
                log.append(("chain", ch["t1"], s, ch["hstar"], iv))
        else:
            d = best[:3]
            ends = DL.ends(work, d)
            work = S3.apply_window_move(work, d, cur, c)
        A = hit
        A[ends] = True
        moves += 1
    cur = SR.walk(work, seq[0], W)
    c1 = SR.window_cost(D, cur)
    ok = c1 < c0
    c["accepted"] += int(ok)
    return (work, cur, True) if ok else (succ, seq, False)


def window_groups(D, succ, nbr, kinds, depth, seq, seed, b, it, w, G, T, S, cap, c, log=None):
    """seg_groups_ref.window_groups over this file's trial"""
    W = len(seq)
    c_start = np.float64(SR.window_cost(D, seq))
    offers, fins = [], {}
    for g in range(G):
        cur_succ, cur_seq, acc = succ, seq, 0
        for t in range(T):
            cur_succ, cur_seq, ok = trial(D, cur_succ, nbr, kinds, depth, cur_seq, SR.trial_draws(seed, b, it, w * G + g, T, t), S,
                                          cap, c, log)
            acc += int(ok)
            c["trials"] += 1
        if not acc:
            continue
        diff = [k for k in range(W) if cur_seq[k] != seq[k]]
        gain = float(np.float64(SR.window_cost(D, cur_seq)) - c_start)
        assert diff and 1 <= diff[0] <= diff[-1] <= W - 2 and gain < 0.0
        offers.append((gain, g, diff[0], diff[-1]))
        fins[g] = cur_seq
    return offers, fins


def run(D, succ, nbr, kinds, seed, b, iterations, depth=0, groups=1, window=0, span=0, trials=1, max_moves=-1, log=None, glog=None):
    """tsp_dev_seg_ils_lk of one chain -> (succ', cost, stats without deltas_executed and the times).  log: as trial takes it.
    glog: one record (it, w, offers, committed) per window."""
    succ = np.array(succ, dtype=np.int32, copy=True)
    n = len(succ)
    depth = resolve_depth(depth)
    assert depth is not None and 1 <= kinds <= 15
    c = new_counters()
    c["lk_depth"] = depth
    c["start_cost"] = SR.IR.cost(D, succ)
    if n < 10:
        c["groups"] = groups if groups >= 1 else 1
        return succ, c["start_cost"], c
    W, S = SR.resolve(n, window, span)
    G = groups if groups >= 1 else SG.default_groups(n, W)
    assert G <= SG.MAX_GROUPS
    c["windows"], c["groups"] = n // W, G
    for it in range(iterations):
        wins = SR.windows(succ, seed, b, it, W)
        for w, seq in enumerate(wins):
            offers, fins = window_groups(D, succ, nbr, kinds, depth, seq, seed, b, it, w, G, trials, S, max_moves, c, log)
            keep = SG.committed(offers)
            new = list(seq)
            for gain, g, lo, hi in offers:
                if g in keep:
                    assert sorted(fins[g][lo:hi + 1]) == sorted(seq[lo:hi + 1])
                    new[lo:hi + 1] = fins[g][lo:hi + 1]
            succ = SR.set_path(succ, new)
            c["offers"] += len(offers)
            c["commits"] += len(keep)
            if glog is not None:
                glog.append((it, w, list(offers), sorted(keep)))
        c["iterations"] += 1
    return succ, SR.IR.cost(D, succ), c
