"""The reference of a run of tabu() iterations (tabusearch.c:238-309), restated around the oracle's alg_2opt_tabu.

An iteration is: alg_2opt_tabu on the stamps in place (O.two_opt_best), the incumbent's update, the kick's trials with
check_tenure's lazy clears (:262-287), reverse_path (:288-290) and the two stamps (:306-309).  `replay` makes the whole
trajectory a function of ONE ordered stream of node pairs: iteration k takes pairs from the stream, in order, until one is
accepted -- however a driver cuts the iterations into calls, chains and further trials, it must consume the same pairs in the
same order and arrive at the same tours.  Test infrastructure only (tests/, tools/stress_parity.py, the golden generator)."""
import numpy as np

from oracle import oracle as O


def upos(a, b, n):
    """utility.c:17-30: the stamp of the undirected edge {a, b}"""
    if a > b:
        a, b = b, a
    return a * n + b - (a + 1) * (a + 2) // 2


def tenure_bounds(n):
    """tabusearch.c:213-214 -> (lo, hi)"""
    lo, hi = int(np.ceil(n * 0.02)), int(np.floor(n * 0.1 + 0.5))     # C's round(): halves away from zero
    if lo == hi:
        hi += 2
    elif hi < lo:
        lo, hi = hi, lo
    return lo, hi


def policy_tenures(n, policy, count):
    """The tenures of iterations 1 .. count under step_policy (0, :33-37) or linear_policy (1, :47-59); the policy is stepped
    after an iteration's kick (:298-304).  random_policy draws from libc inside the loop and is not restated here."""
    assert policy in (0, 1)
    lo, hi = tenure_bounds(n)
    tenure, rising, out = lo, False, []
    for it in range(1, count + 1):
        out.append(tenure)
        if policy == 0:
            if it % 100 == 0:
                tenure = hi if tenure == lo else lo
        else:
            tenure = min(max(tenure, lo), hi)
            if tenure in (lo, hi):
                rising = not rising
            tenure += 1 if rising else -1
    return out


def pair_stream(n, seed, count):
    """`count` node pairs over [0, n) from a seeded numpy generator, one in ten made a == b (rejected, :271-273)"""
    rng = np.random.default_rng(seed)
    ab = rng.integers(0, n, size=(count, 2)).astype(np.int32)
    same = rng.random(count) < 0.1
    ab[same, 1] = ab[same, 0]
    return ab


def canonical_cycle(succ):
    """The cycle as a permutation from node 0 towards the smaller of its two neighbours: one form for both orientations"""
    perm = O.succ_to_perm(np.ascontiguousarray(succ, dtype=np.int32))
    if len(perm) > 2 and perm[1] > perm[-1]:
        perm = np.concatenate([perm[:1], perm[:0:-1]])
    return np.ascontiguousarray(perm, dtype=np.int32)


def sparse(stamps):
    """-> (indices, values) of the non-zero stamps"""
    idx = np.nonzero(stamps)[0]
    return idx, stamps[idx]


class Replay:
    """What `replay` returns.  Per iteration that ran its descent: obj (after the descent), improved, trials, best (the
    running incumbent cost).  accepted: the last iteration's kick was carried out (False: the stream ran out first; that
    iteration has its descent and the trials it could take).  consumed: pairs taken from the stream.  tour, stamps: the state
    after the last iteration; inc, inc_cost: the incumbent.  snaps[k] = (tour, (indices, values) of the non-zero stamps) after
    the k-th iteration of this call's count, kick included, and the incumbent at that point as a third element."""

    def __init__(self):
        self.obj, self.improved, self.trials, self.best = [], [], [], []
        self.accepted, self.consumed = True, 0
        self.tour = self.stamps = self.inc = None
        self.inc_cost = float("inf")
        self.snaps = {}


def replay(xy, wt, ic, succ0, cost0, stamps0, it0, tenures, stream, best0=float("inf"), inc0=None, snaps=()):
    """len(tenures) iterations of tabu() from the tour succ0 (cost cost0) and the stamps stamps0 (None: all zero; copied), the
    first of them numbered it0.  Iteration k descends with tenures[k], updates the incumbent (best0 / inc0 to start from),
    then takes pairs from `stream` ([P, 2]) in order until one is accepted.  Stops after the iteration in whose trials the
    stream runs out."""
    n = len(xy)
    stream = np.asarray(stream, dtype=np.int64).reshape(-1, 2)
    stamps = np.zeros(n * (n - 1) // 2, dtype=np.int32) if stamps0 is None else np.array(stamps0, dtype=np.int32, copy=True)
    cur, cost = np.array(succ0, dtype=np.int32, copy=True), float(cost0)
    r = Replay()
    r.inc_cost, r.inc = float(best0), (None if inc0 is None else np.array(inc0, dtype=np.int32, copy=True))

    def is_tabu(a, b, itn, ten):          # check_tenure, :83-92
        q = upos(a, b, n)
        v = stamps[q]
        if v == 0:
            return False
        if itn - v > ten:
            stamps[q] = 0
            return False
        return True

    p = 0
    for k, ten in enumerate(tenures):
        itn, ten = it0 + k, int(ten)
        _, cur, cost, _, _, _ = O.two_opt_best(xy, wt, cur, cost, integer_cost=ic, tabu=stamps, iter_=itn, tenure=ten)   # :238
        cur = np.array(cur, dtype=np.int32)
        better = cost < r.inc_cost                                                                          # :241-249
        if better:
            r.inc_cost, r.inc = cost, cur.copy()
        r.obj.append(cost); r.improved.append(bool(better)); r.best.append(r.inc_cost)
        used, acc = 0, False
        while p < len(stream) and not acc:                                                                  # :262-287
            a, b = int(stream[p, 0]), int(stream[p, 1])
            p += 1; used += 1
            a1, b1 = int(cur[a]), int(cur[b])
            if a == b or a1 == b or b1 == a:
                continue
            if not is_tabu(a, a1, itn, ten) and not is_tabu(b, b1, itn, ten) and not is_tabu(a, b, itn, ten) and not is_tabu(a1, b1, itn, ten):
                acc = True
                path, v = [], a1                       # a1 ... b along the tour, reversed (utility.c:708-717)
                while True:
                    path.append(v)
                    if v == b:
                        break
                    v = int(cur[v])
                cur[a] = b
                for q in range(len(path) - 1, 0, -1):
                    cur[path[q]] = path[q - 1]
                cur[a1] = b1
                stamps[upos(a, a1, n)] = itn; stamps[upos(b, b1, n)] = itn                                  # :306-309
        r.trials.append(used)
        r.accepted = acc
        if acc and (k + 1) in snaps:
            r.snaps[k + 1] = (cur.copy(), sparse(stamps), r.inc.copy())
        if not acc:
            break
    r.consumed, r.tour, r.stamps = p, cur, stamps
    return r
