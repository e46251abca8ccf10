"""CPU references of the three constructive heuristics on an n x n distance matrix, in plain Python / numpy.

greedy(D, start), grasp(D, start, urand) and extramileage(D) restate src/heuristics.c on a matrix instead of coordinates, so that
they can run on the DEVICE's own distances: for GEO, glibc and ocml differ in the last ulp of cos / acos, and a construction
compared on the device's matrix is decision-exact where one compared on the oracle's is not.  They are also a second statement of
the heuristics, written independently of oracle/tsp_oracle.c (tests/test_cpu_construct_ref.py holds the two against each other).

What they keep of the reference, bit for bit:
  - D is indexed in calc_dist's argument order: D[cur, k] (:50, :116); (D[a, c] + D[c, b]) - D[a, b] (:272-275);
  - the strict '<' of a scan in index order: the first of equal minima wins (:51, :117, :276), the first of equal maxima too (:230);
  - GRASP's runner-up is the running minimum just before the last one (:117-122), i.e. the first minimum among the unvisited nodes
    with a SMALLER index than the winner -- not the second nearest node;
  - GRASP adds the closing edge inside the loop (:135) and again after it (:152);
  - extra-mileage keeps its edges in slots: the replaced slot gets (a, c) and (c, b) is appended (:298-299), and later ties go to
    the lower slot;
  - costs are added one by one in visiting order (:70, :148, :303), never pairwise.
"""
import numpy as np

GRASP_RAND = 0.9   # src/heuristics.c:10


def _first_min(vals):
    """index of the first minimum of a 1-d array (a strict '<' scan in index order), -1 if it is empty"""
    return int(np.argmin(vals)) if len(vals) else -1


def greedy(D, start):
    """src/heuristics.c:18-78 -> (succ int32 [n], obj)"""
    n = D.shape[0]
    succ = np.zeros(n, dtype=np.int32)
    free = np.ones(n, dtype=bool)
    free[start] = False
    obj = 0.0
    cur = start
    for _ in range(n - 1):
        cand = np.flatnonzero(free)                 # ascending: the scan's order (:48-49; cur itself is visited)
        k = int(cand[_first_min(D[cur, cand])])     # :51
        succ[cur] = k
        free[k] = False
        obj += float(D[cur, k])                     # :70
        cur = k
    succ[cur] = start                               # :60-61
    obj += float(D[cur, start])                     # :74
    return succ, obj


def grasp(D, start, urand):
    """src/heuristics.c:82-156 with the n values URAND() returns, in draw order -> (succ int32 [n], obj)"""
    n = D.shape[0]
    succ = np.zeros(n, dtype=np.int32)
    free = np.ones(n, dtype=bool)
    free[start] = False
    obj = 0.0
    cur = start
    for step in range(n - 1):
        cand = np.flatnonzero(free)
        row = D[cur, cand]
        w = _first_min(row)                         # :117
        pick, d = int(cand[w]), float(row[w])
        if not (urand[step] < GRASP_RAND) and w > 0:   # :128; w == 0: no running minimum before the winner (second_minidx == -1)
            r = _first_min(row[:w])                 # :118-119 as a definition: the first minimum below the winner
            pick, d = int(cand[r]), float(row[r])
        succ[cur] = pick
        free[pick] = False
        obj += d                                    # :148
        cur = pick
    # the n-th pass of the loop finds no node (it still draws, :127): the closing edge, counted at :135 and again at :152
    succ[cur] = start
    obj += float(D[cur, start])
    obj += float(D[cur, start])
    return succ, obj


def extramileage(D):
    """src/heuristics.c:208-314 -> (succ int32 [n], obj).  O(n^3 / vector width): for n of a few hundred."""
    n = D.shape[0]
    A, B, far = 0, 1, 0.0                           # :214-215, :226
    for i in range(n - 1):
        row = D[i, i + 1:]
        j = int(np.argmax(row))                     # the first of the row's maxima; rows in order: the first (i, j) overall
        if row[j] > far:                            # :230
            A, B, far = i, i + 1 + j, float(row[j])
    succ = np.zeros(n, dtype=np.int32)
    frm = np.zeros(n, dtype=np.int64)
    to = np.zeros(n, dtype=np.int64)
    frm[0], to[0], frm[1], to[1] = A, B, B, A       # :239-243
    m = 2
    succ[A], succ[B] = B, A
    free = np.ones(n, dtype=bool)
    free[[A, B]] = False
    obj = 2 * float(D[A, B])                        # :250
    while m < n:
        nodes = np.flatnonzero(free)
        a, b = frm[:m], to[:m]
        # extra[c, j] = (D[a_j, c] + D[c, b_j]) - D[a_j, b_j], :272-275; node-major, slot-minor like the loops at :263 / :267
        extra = (D[a][:, nodes].T + D[nodes][:, b]) - D[a, b][None, :]
        flat = int(np.argmin(extra))                # first minimum in (node, slot) order, :276
        ci, j = divmod(flat, m)
        c = int(nodes[ci])
        x, y = int(frm[j]), int(to[j])
        succ[x], succ[c] = c, y                     # :296-297
        to[j] = c                                   # :298, the slot now holds (a, c)
        frm[m], to[m] = c, y                        # :299, (c, b) appended
        m += 1
        free[c] = False
        obj += float(extra[ci, j])                  # :303
    return succ, obj
