"""CPU reference of the Or-opt neighbourhood of include/tsp_hip.h (tsp_dev_or_opt / tsp_dev_two_opt_or_opt), numpy over the
oracle's distance matrix.  A helper of the tests, not collected by pytest.

Move (f, L, a, o): segment f = x1 -> .. -> xL = l (p = pred f, s = succ l), inserted between a and b = succ a,
a not in {p, x1..xL}; o = 0 forward (a f .. l b), o = 1 reversed (a l .. f b, L > 1).
    rem = (d(p,f) + d(l,s)) - d(p,s);  ins = (d(a,f) + d(l,b)) - d(a,b)  [reversed: (d(a,l) + d(f,b)) - d(a,b)];  delta = ins - rem
Decision: smallest delta among delta < 0, ties -> smallest key ((f*3 + L-1)*n + a)*2 + o."""
import numpy as np

from oracle import oracle as O


def n_moves(n):
    """N(n) = n(n-2) + 2n(n-3) + 2n(n-4) = n(5n - 16) moves per decision."""
    return n * (5 * n - 16) if n >= 5 else 0


def tour_order(succ):
    n = len(succ)
    order = np.empty(n, dtype=np.int64)
    v = 0
    for k in range(n):
        order[k] = v
        v = int(succ[v])
    return order


def key(f, L, a, o, n):
    return ((f * 3 + (L - 1)) * n + a) * 2 + o


def decode(k, n):
    o = k & 1
    t = k >> 1
    a = t % n
    fl = t // n
    return fl // 3, fl % 3 + 1, a, o


def apply_move(succ, f, L, a, o):
    """The move on a successor list (every right-hand side read before the move)."""
    succ = np.array(succ, dtype=np.int32, copy=True)
    x = [f]
    for _ in range(L - 1):
        x.append(int(succ[x[-1]]))
    l = x[-1]
    p = int(np.nonzero(succ == f)[0][0])
    s, b = int(succ[l]), int(succ[a])
    if o == 0:
        succ[p], succ[a], succ[l] = s, f, b
    else:
        succ[p], succ[a] = s, l
        for k in range(L - 1):
            succ[x[k + 1]] = x[k]
        succ[f] = b
    return succ


def _decision_mats(Dp, E, order, n):
    """Yields (L, o, delta matrix over (row position i, column position j) with +inf where not a move)."""
    cols = np.arange(n)
    for L in (1, 2, 3):
        i = np.arange(n)
        p, l, s = (i - 1) % n, (i + L - 1) % n, (i + L) % n
        rem = (Dp[p, i] + Dp[l, s]) - Dp[p, s]
        invalid = ((cols[None, :] - i[:, None] + 1) % n) <= L
        Dl = Dp[l]                       # rows: position of l
        Dj1 = np.roll(Dp, -1, axis=1)    # column j -> D(., j + 1)
        for o in ((0,) if L == 1 else (0, 1)):
            if o == 0:
                ins = (Dp + Dj1[l]) - E[None, :]
            else:
                ins = (Dl + Dj1) - E[None, :]
            delta = ins - rem[:, None]
            delta[invalid] = np.inf
            yield L, o, delta


def decide(D, succ):
    """One best-improvement decision -> (delta, key) or None when no move improves."""
    n = len(succ)
    order = tour_order(succ)
    Dp = D[np.ix_(order, order)]
    E = Dp[np.arange(n), (np.arange(n) + 1) % n]
    best = None
    for L, o, delta in _decision_mats(Dp, E, order, n):
        m = delta.min()
        if not m < 0.0:
            continue
        ii, jj = np.nonzero(delta == m)
        k = int((((order[ii] * 3 + (L - 1)) * n + order[jj]) * 2 + o).min())
        if best is None or m < best[0] or (m == best[0] and k < best[1]):
            best = (float(m), k)
    return best


def or_opt_descent(xy, wt, succ, integer_cost=1, max_moves=-1, D=None):
    """-> (succ', counters dict: sweeps, evals, moves, moves_by_len, moves_reversed)"""
    if D is None:
        D = O.dist_matrix(xy, wt, integer_cost)
    succ = np.array(succ, dtype=np.int32, copy=True)
    n = len(succ)
    c = {"sweeps": 0, "evals": 0, "moves": 0, "moves_by_len": [0, 0, 0], "moves_reversed": 0}
    if n < 5:
        return succ, c
    while max_moves < 0 or c["moves"] < max_moves:
        c["sweeps"] += 1
        c["evals"] += n_moves(n)
        d = decide(D, succ)
        if d is None:
            break
        f, L, a, o = decode(d[1], n)
        succ = apply_move(succ, f, L, a, o)
        c["moves"] += 1
        c["moves_by_len"][L - 1] += 1
        c["moves_reversed"] += o
    return succ, c


def two_opt_or_opt(xy, wt, succ, obj, mode=0, integer_cost=1, D=None):
    """2-opt (the oracle's two_opt_first for mode 0, two_opt_best for mode 1) and Or-opt descents in turn until an Or-opt
    descent makes no move.  -> (succ', recomputed cost, rounds)"""
    if D is None:
        D = O.dist_matrix(xy, wt, integer_cost)
    rounds = 0
    while True:
        if mode == 0:
            _, succ, obj, _, _ = O.two_opt_first(xy, wt, succ, obj, integer_cost)
        else:
            _, succ, obj, _, _, _ = O.two_opt_best(xy, wt, succ, obj, integer_cost)
        succ, c = or_opt_descent(xy, wt, succ, integer_cost, D=D)
        rounds += 1
        if c["moves"] == 0:
            break
    return succ, O.succ_cost(xy, wt, succ, integer_cost), rounds


def _euc_rows(xy, rows, cols, integer_cost):
    """calc_dist of EUC_2D (src/distutil.c:13-18) for a block of node pairs: the same IEEE operations in the same order."""
    dx = xy[rows, 0][:, None] - xy[cols, 0][None, :]
    dy = xy[rows, 1][:, None] - xy[cols, 1][None, :]
    d = np.sqrt(dx * dx + dy * dy)
    return np.floor(d + 0.5) if integer_cost else d


def _blocked_rows(xy, wt, succ, integer_cost, chunk, D):
    """Yields (row positions i, L, o, delta block over (i, every column position)) with +inf where not a move, rows in
    chunks: the same IEEE operations in the same order as _decision_mats."""
    n = len(succ)
    order = tour_order(succ)
    xy = np.asarray(xy, dtype=np.float64)
    if D is None and wt != O.EUC_2D:
        D = O.dist_matrix(xy, wt, integer_cost)

    def block(ri, cj):
        if D is not None:
            return D[np.ix_(order[ri], order[cj])]
        return _euc_rows(xy, order[ri], order[cj], integer_cost)

    allc = np.arange(n)
    E = block(allc, (allc + 1) % n)[allc, allc] if D is not None else None
    if E is None:
        a, b = order, order[(allc + 1) % n]
        dx, dy = xy[a, 0] - xy[b, 0], xy[a, 1] - xy[b, 1]
        d = np.sqrt(dx * dx + dy * dy)
        E = np.floor(d + 0.5) if integer_cost else d
    Ecol = E[None, :]
    for r0 in range(0, n, chunk):
        i = np.arange(r0, min(n, r0 + chunk))
        win = (np.arange(r0 - 1, i[-1] + 4)) % n          # positions i-1 .. i+3
        Dw = block(win, allc)                             # D(win, column)
        Dw1 = np.roll(Dw, -1, axis=1)
        row = lambda q: Dw[q - (r0 - 1)]                  # noqa: E731  D(position q, .)
        row1 = lambda q: Dw1[q - (r0 - 1)]                # noqa: E731  D(position q, . + 1)
        for L in (1, 2, 3):
            pp, ll, ss = i - 1, i + L - 1, i + L
            dpf = row(pp)[np.arange(len(i)), i % n]
            dls = row(ll)[np.arange(len(i)), ss % n]
            dps = row(pp)[np.arange(len(i)), ss % n]
            rem = (dpf + dls) - dps
            invalid = ((allc[None, :] - i[:, None] + 1) % n) <= L
            outs = [((row(i) + row1(ll)) - Ecol) - rem[:, None]]
            if L > 1:
                outs.append(((row(ll) + row1(i)) - Ecol) - rem[:, None])
            for o, dm in enumerate(outs):
                dm[invalid] = np.inf
                yield order, i, L, o, dm


def min_delta(xy, wt, succ, integer_cost=1, chunk=256, D=None):
    """Smallest delta over every Or-opt move of the tour (rows in chunks: usable up to n of about 20 000 for EUC_2D, whose
    distances are computed here block by block; other metrics take the oracle's full matrix)."""
    best = np.inf
    for _, _, _, _, dm in _blocked_rows(xy, wt, succ, integer_cost, chunk, D):
        best = min(best, float(dm.min()))
    return best


def decide_blocked(xy, wt, succ, integer_cost=1, chunk=256, D=None):
    """decide() with the rows in chunks, as min_delta walks them (no n x n matrix for EUC_2D): -> (delta, key) or None."""
    n = len(succ)
    if n < 5:
        return None
    best = None
    for order, i, L, o, dm in _blocked_rows(xy, wt, succ, integer_cost, chunk, D):
        m = dm.min()
        if not m < 0.0:
            continue
        ii, jj = np.nonzero(dm == m)
        k = int((((order[i[ii]] * 3 + (L - 1)) * n + order[jj]) * 2 + o).min())
        if best is None or m < best[0] or (m == best[0] and k < best[1]):
            best = (float(m), k)
    return best


def or_opt_prefix_blocked(xy, wt, succ, moves, integer_cost=1, D=None):
    """The first `moves` decisions of the descent through decide_blocked -> (succ', counters as or_opt_descent's,
    [(m1, m2)] of every applied move as shift_lengths gives them)."""
    succ = np.array(succ, dtype=np.int32, copy=True)
    n = len(succ)
    c = {"sweeps": 0, "evals": 0, "moves": 0, "moves_by_len": [0, 0, 0], "moves_reversed": 0}
    shifts = []
    while n >= 5 and c["moves"] < moves:
        c["sweeps"] += 1
        c["evals"] += n_moves(n)
        d = decide_blocked(xy, wt, succ, integer_cost, D=D)
        if d is None:
            break
        f, L, a, o = decode(d[1], n)
        shifts.append(shift_lengths(succ, f, L, a))
        succ = apply_move(succ, f, L, a, o)
        c["moves"] += 1
        c["moves_by_len"][L - 1] += 1
        c["moves_reversed"] += o
    return succ, c, shifts


def shift_lengths(succ, f, L, a):
    """(m1, m2) of the move as k_or_pick_apply splits the tour: m1 nodes s .. a, m2 nodes b .. p."""
    n = len(succ)
    pos = np.empty(n, dtype=np.int64)
    pos[tour_order(succ)] = np.arange(n)
    m1 = (int(pos[a]) - (int(pos[f]) + L)) % n + 1
    return m1, n - L - m1


def is_or_opt_optimal(xy, wt, succ, integer_cost=1, rel_tol=0.0, cost=None):
    """No Or-opt move improves (by more than rel_tol * cost when rel_tol > 0)."""
    m = min_delta(xy, wt, succ, integer_cost)
    if rel_tol > 0:
        return m >= -rel_tol * abs(cost)
    return not m < 0.0
