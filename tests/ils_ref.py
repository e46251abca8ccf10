"""CPU reference of the iterated local search of include/tsp_hip.h (tsp_dev_ils, tsp_dev_ils_kick): the counter-based random
stream, the double-bridge kick and the chain, on top of nl3_opt_ref.descent(..., sparse=True).  A helper of the tests, not
collected by pytest.  The cost is the sum over nodes in node order, added one after the other (np.sum is pairwise)."""
import numpy as np

import nl3_opt_ref as N3

M64 = (1 << 64) - 1
GOLD, MUL1, MUL2, CHAIN = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0x100000001B3
NL_COUNTERS = ("decisions", "moves", "moves_2opt", "moves_oropt", "moves_by_len", "moves_reversed", "reversed", "moves_3opt",
               "moves_by_type")


def mix(x):
    x = (x + GOLD) & M64
    z = x
    z = ((z ^ (z >> 30)) * MUL1) & M64
    z = ((z ^ (z >> 27)) * MUL2) & M64
    return z ^ (z >> 31)


def draws(seed, b, it):
    """u_0 .. u_4 of chain b at iteration it"""
    base = mix((mix((seed & M64) ^ ((b * CHAIN) & M64)) + it) & M64)
    return [mix((base + j) & M64) for j in range(5)]


def window(n, span):
    return n if span <= 0 else min(span, n)


def cuts(n, span, u):
    """-> (s, o1, o2, o3, o4) of the kick"""
    W = window(n, span)
    assert n >= 8 and W >= 8
    s = u[0] % n
    o1 = 1 + u[1] % (W - 3)
    o2 = o1 + 1 + u[2] % (W - 2 - o1)
    o3 = o2 + 1 + u[3] % (W - 1 - o2)
    o4 = o3 + 1 + u[4] % (W - o3)
    assert 1 <= o1 < o2 < o3 < o4 <= W
    return s, o1, o2, o3, o4


def kick(succ, seed, b, it, span):
    """the tour P Dk Ck Bk R of the definition, as a successor list"""
    succ = np.asarray(succ)
    n = len(succ)
    s, o1, o2, o3, o4 = cuts(n, span, draws(seed, b, it))
    seq = [s]
    for _ in range(n - 1):
        seq.append(int(succ[seq[-1]]))
    new = seq[:o1] + seq[o3:o4] + seq[o2:o3] + seq[o1:o2] + seq[o4:]
    new = np.array(new, dtype=np.int32)
    out = np.empty(n, dtype=np.int32)
    out[new] = np.roll(new, -1)
    return out


def cost(D, succ):
    c = 0.0
    for v in range(len(succ)):
        c += float(D[v, succ[v]])
    return c


def _add(total, c):
    for k in NL_COUNTERS:
        if isinstance(c[k], list):
            total[k] = [x + y for x, y in zip(total[k], c[k])]
        else:
            total[k] += c[k]


def chain(D, succ, nbr, kinds, seed, b, iterations, span=0, max_moves=-1):
    """-> (succ', cost, stats): the nl counters summed over all descents, iterations, accepted, last_improved, start_cost"""
    n = len(succ)
    total = N3.new_counters()
    inc, c = N3.descent(D, succ, nbr, kinds, max_moves=max_moves, sparse=True)
    _add(total, c)
    best = cost(D, inc)
    st = {"iterations": 0, "accepted": 0, "last_improved": -1, "start_cost": best}
    if n >= 8:
        for it in range(iterations):
            work, c = N3.descent(D, kick(inc, seed, b, it, span), nbr, kinds, max_moves=max_moves, sparse=True)
            _add(total, c)
            cw = cost(D, work)
            if cw < best:
                inc, best = work, cw
                st["accepted"] += 1
                st["last_improved"] = it
            st["iterations"] += 1
    st.update(total)
    return inc, best, st
