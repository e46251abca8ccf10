"""CPU reference of the windowed iterated local search with groups (include/tsp_hip.h, tsp_dev_seg_ils_groups), on top of
seg_ils3_ref.trial and seg_ils_ref.windows / trial_draws / window_cost / set_path: G groups per window run their trials from the
window as the iteration found it, and the offers that lose to no other offer are written to the tour.  The rule is stated here
from the header's text, not from csrc/seg_groups.hpp.  A helper of the tests, not collected by pytest."""
import numpy as np

import seg_ils3_ref as S3
import seg_ils_ref as SR

MAX_GROUPS = 64
COUNTERS = S3.COUNTERS + ("groups", "offers", "commits")


def default_groups(n, W):
    """G of groups <= 0: a function of n and W only"""
    return max(1, min(MAX_GROUPS, 1024 // (n // W)))


def conflict(a, b):
    """offers (gain, g, lo, hi): the edges of the slots lo - 1 .. hi of the two meet"""
    return b[2] - 1 <= a[3] and a[2] - 1 <= b[3]


def committed(offers):
    """offers: a list of (gain, g, lo, hi) -> the set of g that lose to no group"""
    return {a[1] for a in offers if not any(b[1] != a[1] and conflict(a, b) and (b[0], b[1]) < (a[0], a[1]) for b in offers)}


def new_counters():
    c = S3.new_counters()
    c.update({"groups": 0, "offers": 0, "commits": 0})
    return c


def window_groups(D, succ, nbr, kinds, seq, seed, b, it, w, G, T, S, cap, c):
    """The G groups of window w (the path seq of the tour succ) -> (the offers (gain, g, lo, hi), fin by g)"""
    W = len(seq)
    c_start = np.float64(SR.window_cost(D, seq))
    offers, fins = [], {}
    for g in range(G):
        cur_succ, cur_seq, acc = succ, seq, 0
        for t in range(T):
            cur_succ, cur_seq, ok = S3.trial(D, cur_succ, nbr, kinds, cur_seq, SR.trial_draws(seed, b, it, w * G + g, T, t), S, cap, c)
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


def run(D, succ, nbr, kinds, seed, b, iterations, groups=0, window=0, span=0, trials=1, max_moves=-1, log=None):
    """tsp_dev_seg_ils_groups of one chain -> (succ', cost, stats without deltas_executed and the times).  log: a list that takes
    one record (it, w, g, offer, gain, lo, hi, committed) per group; gain, lo and hi are None without an offer."""
    succ = np.array(succ, dtype=np.int32, copy=True)
    n = len(succ)
    c = new_counters()
    c["start_cost"] = SR.IR.cost(D, succ)
    if n < 10:
        c["groups"] = groups if groups >= 1 else 1
        return succ, c["start_cost"], c
    W, S = SR.resolve(n, window, span)
    G = groups if groups >= 1 else default_groups(n, W)
    assert G <= MAX_GROUPS
    c["windows"], c["groups"] = n // W, G
    for it in range(iterations):
        wins = SR.windows(succ, seed, b, it, W)
        for w, seq in enumerate(wins):
            offers, fins = window_groups(D, succ, nbr, kinds, seq, seed, b, it, w, G, trials, S, max_moves, c)
            keep = committed(offers)
            new = list(seq)
            for gain, g, lo, hi in offers:
                if g in keep:
                    assert sorted(fins[g][lo:hi + 1]) == sorted(seq[lo:hi + 1])
                    new[lo:hi + 1] = fins[g][lo:hi + 1]
            succ = SR.set_path(succ, new)
            c["offers"] += len(offers)
            c["commits"] += len(keep)
            if log is not None:
                by_g = {o[1]: o for o in offers}
                for g in range(G):
                    o = by_g.get(g)
                    log.append((it, w, g, o is not None, o[0] if o else None, o[2] if o else None, o[3] if o else None, g in keep))
        c["iterations"] += 1
    return succ, SR.IR.cost(D, succ), c
