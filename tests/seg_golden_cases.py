"""The cases of tests/golden/seg_runs.json: instances, lists, start tours, parameters and the state record of the windowed iterated
local search at the shapes it works at, shared by the recorder (tests/golden/make_golden_seg.py), tests/test_cpu_seg_golden.py and
tests/test_gpu_seg_golden.py.  A helper of the tests, not collected by pytest.

S1: rand_instance(1100), one window of 1024 with span W - 1 from a random tour, through all four entry points: the active set, a
    reversal, a 3-opt relabeling and a chain's hull outgrow the 256 threads of a workgroup.
S2: rand_instance(2100, hi = 100000), the largest window (2048) from a random tour to the end, with chains.
S3: rand_instance(5000) from the oracle's greedy tour, 78 windows of 64 at once without groups, states after 1, 2, 3 iterations.
S4: the same instance and start with groups: 78 x 16 = 1248 workgroups, 4 windows of 1024 x 16 groups x 4 trials, 19 x 8 x 2,
    and 4 windows of 1024 x 4 x 4 with span W - 1, where rejected trials are restored over most of the window.
S5: kroA100 from a random tour, 640 iterations of four windows of 25: past the host's first batches of launches, and most
    trials rejected and restored.

A run is one entry point with its parameters on one instance; its states are keyed by the number of iterations, each the
reference's result of a call of that many iterations from the start."""
import contextlib
import hashlib

import numpy as np

import nl3_opt_ref as N3
import nl_opt_ref as NL
import seg_groups_ref as SG
import seg_ils3_ref as S3
import seg_ils_ref as SR
import seg_lk_ref as SL
from helpers import load_instance, rand_instance, random_tour
from oracle import oracle as O

FIXTURE = "seg_runs.json"
THREADS = 256                # of a workgroup of k_seg_ils
CHAIN_GROUPS = 16            # chains it runs side by side
RESIDENT = 1024              # workgroups of k_seg_ils the device holds at once (seg_run)
# Descent::run queues one launch, then batches of 4, 8, .. doubling up to 256: the iterations queued when it looks at the clock
BATCH_ENDS = (1, 5, 13, 29, 61, 125, 253, 509, 765)

REFS = {"seg_ils": SR, "seg_ils3": S3, "seg_ils_groups": SG, "seg_ils_lk": SL}

INSTANCES = {
    "r1100": {"n": 1100, "K": 5, "wt": "EUC_2D", "integer_cost": 1, "start": "random"},
    "r2100": {"n": 2100, "K": 5, "wt": "EUC_2D", "integer_cost": 1, "start": "random", "hi": 100000},
    "r5000": {"n": 5000, "K": 5, "wt": "EUC_2D", "integer_cost": 1, "start": "greedy"},
    "kroA100": {"n": 100, "K": 5, "wt": "EUC_2D", "integer_cost": 1, "start": "random", "tsplib": "kroA100"},
}


def _run(case, instance, entry, kinds, iterations, window, span, trials, seed, groups=1, depth=0, max_moves=-1):
    return {"case": case, "instance": instance, "entry": entry, "kinds": kinds, "iterations": list(iterations), "window": window,
            "span": span, "trials": trials, "seed": seed, "groups": groups, "depth": depth, "max_moves": max_moves}


S5_ITERATIONS = (1, 5, 6, 13, 29, 61, 125, 252, 253, 300, 509, 640)
S5_CPU = 252                 # tests/test_cpu_seg_golden.py recomputes the states up to here
S5_DRY_FROM = 100            # behind this iteration fewer than a tenth of the trials are accepted

RUNS = {
    "S1-ils": _run("S1", "r1100", "seg_ils", 3, (1,), 1024, 0, 1, 3),
    "S1-ils3": _run("S1", "r1100", "seg_ils3", 7, (1,), 1024, 0, 1, 3),
    "S1-groups": _run("S1", "r1100", "seg_ils_groups", 7, (1,), 1024, 0, 1, 3, groups=2),
    "S1-lk": _run("S1", "r1100", "seg_ils_lk", 15, (1,), 1024, 0, 1, 3, groups=1, depth=16),
    "S1-lk8": _run("S1", "r1100", "seg_ils_lk", 8, (1,), 1024, 0, 1, 3, groups=1, depth=16),
    "S2-lk": _run("S2", "r2100", "seg_ils_lk", 15, (1,), 2048, 0, 1, 6, groups=1, depth=16),
    # seed 2: under seed 3 fewer than half of the windows accept in the third iteration
    "S3-ils": _run("S3", "r5000", "seg_ils", 3, (1, 2, 3), 64, 50, 2, 2),
    "S3-ils3": _run("S3", "r5000", "seg_ils3", 7, (1, 2, 3), 64, 50, 2, 2),
    "S4-groups": _run("S4", "r5000", "seg_ils_groups", 7, (2,), 64, 50, 1, 3, groups=16),
    "S4-lk": _run("S4", "r5000", "seg_ils_lk", 15, (2,), 64, 50, 1, 3, groups=16, depth=16),
    "S4-lk-w1024": _run("S4", "r5000", "seg_ils_lk", 15, (2,), 1024, 50, 4, 3, groups=16, depth=16),
    # span W - 1: trials that are rejected with another window than they began with, restored over more than 256 slots ahead
    # of the group's next trial (under span 50 no restore is that long)
    "S4-lk-w1024-span0": _run("S4", "r5000", "seg_ils_lk", 15, (1,), 1024, 0, 4, 3, groups=4, depth=16),
    "S4-lk-w256": _run("S4", "r5000", "seg_ils_lk", 15, (3,), 256, 50, 2, 3, groups=8, depth=16),
    "S5-lk": _run("S5", "kroA100", "seg_ils_lk", 15, S5_ITERATIONS, 25, 10, 1, 3, groups=1, depth=6),
    "S5-groups": _run("S5", "kroA100", "seg_ils_groups", 7, S5_ITERATIONS, 25, 10, 1, 3, groups=3),
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def instance(name, lists=True):
    """-> (xy, wt, the distances, the lists, the start tour); lists = False: (xy, wt, the start tour)"""
    p = INSTANCES[name]
    n = p["n"]
    if "tsplib" in p:
        xy, wt = load_instance(p["tsplib"])
    else:
        xy, wt = (rand_instance(n, seed=n, hi=p["hi"]) if "hi" in p else rand_instance(n)), O.EUC_2D
    assert len(xy) == n and wt == getattr(O, p["wt"])
    if p["start"] == "random":
        start = random_tour(n, np.random.default_rng(n))
    else:
        start = np.asarray(O.greedy(xy, wt)[1], dtype=np.int32)
    if not lists:
        return xy, wt, start
    D = O.dist_matrix(xy, wt, p["integer_cost"])
    return xy, wt, D, NL.knn(D, p["K"]), start


def ref_run(r, D, start, nbr, iterations, log=None, glog=None):
    """the reference of the run r -> (succ', cost, counters)"""
    a = (D, start, nbr, r["kinds"], r["seed"], 0, iterations)
    w = (r["window"], r["span"], r["trials"])
    if r["entry"] == "seg_ils":
        return SR.run(*a, *w, max_moves=r["max_moves"], log=log)
    if r["entry"] == "seg_ils3":
        return S3.run(*a, *w, max_moves=r["max_moves"], log=log)
    if r["entry"] == "seg_ils_groups":
        return SG.run(*a, r["groups"], *w, max_moves=r["max_moves"], log=glog)
    return SL.run(*a, r["depth"], r["groups"], *w, max_moves=r["max_moves"], log=log, glog=glog)


def dev_run(inst, r, start, iterations, time_limit):
    """the entry point of the run r on the device -> (status, succ', cost, stats)"""
    w = (r["window"], r["span"], r["trials"])
    if r["entry"] == "seg_ils":
        return inst.seg_ils(start, iterations, *w, seed=r["seed"], kinds=r["kinds"], max_moves_per_trial=r["max_moves"],
                            time_limit=time_limit)
    if r["entry"] == "seg_ils3":
        return inst.seg_ils3(start, iterations, *w, seed=r["seed"], kinds=r["kinds"], max_moves_per_trial=r["max_moves"],
                             time_limit=time_limit)
    if r["entry"] == "seg_ils_groups":
        return inst.seg_ils_groups(start, iterations, r["groups"], *w, seed=r["seed"], kinds=r["kinds"],
                                   max_moves_per_trial=r["max_moves"], time_limit=time_limit)
    return inst.seg_ils_lk(start, iterations, r["kinds"], r["depth"], r["groups"], *w, seed=r["seed"], max_moves=r["max_moves"],
                           time_limit=time_limit)


def counters_of(entry):
    return REFS[entry].COUNTERS


def kept(entry, c):
    """a device stats dict or a reference's counters: the counters the entry point's reference keeps"""
    return {k: (list(c[k]) if isinstance(c[k], (list, tuple)) else int(c[k])) for k in counters_of(entry)}


def state(xy, wt, ic, entry, succ, c):
    """what the fixture keeps of a tour: no tour, its hash"""
    return {"sha": sha(succ), "cost": O.succ_cost(xy, wt, succ, ic), "counters": kept(entry, c), "start_cost": c["start_cost"]}


@contextlib.contextmanager
def probe():
    """While it is open the references tell what their decisions were made of -> a dict of lists: "active" (the active set of
    every decision that looked for list moves), "rev2" (the slots of every applied 2-opt reversal), "span3" (the slots a 3-opt
    move relabels: from behind its lowest tail to its highest), "kick" (the slots every kick permutes), and per trial, in the
    order of the trials: "accepts" (its outcome), "windows" (the window it started from and the one it ended with, kept or not),
    "touched" (the nodes whose slot its list decisions asked for: the active nodes and their list entries)."""
    seen = {"active": [], "rev2": [], "span3": [], "kick": [], "accepts": [], "windows": [], "touched": []}
    sr_cost = SR.window_cost
    costed, touched = [], set()
    sr_cand, s3_cand, sr_apply, s3_apply = SR.window_candidates, S3.window_candidates, SR.apply_window_move, S3.apply_window_move
    sr_kick, trials = SR.kick, (SR.trial, S3.trial, SL.trial)
    inside = [0]

    def kick(seq, S, v):
        new, ends = sr_kick(seq, S, v)
        diff = [k for k in range(len(seq)) if new[k] != seq[k]]
        seen["kick"].append(diff[-1] - diff[0] + 1 if diff else 0)
        return new, ends

    def trial(inner):
        def f(*a, **kw):
            inside[0] += 1                      # seg_lk_ref.trial hands a trial without chains on to seg_ils3_ref.trial
            try:
                out = inner(*a, **kw)
            finally:
                inside[0] -= 1
            if not inside[0]:
                seen["accepts"].append(bool(out[2]))
                seen["windows"].append((costed[0], costed[-1]))
                seen["touched"].append(set(touched))
                del costed[:]
                touched.clear()
            return out
        return f

    def cand(inner):
        def f(D, succ, nbr, kinds, active, seq):
            seen["active"].append(int(np.asarray(active).sum()))
            ids = np.flatnonzero(active)
            touched.update(int(v) for v in ids)
            touched.update(int(v) for v in np.asarray(nbr)[ids].ravel())
            return inner(D, succ, nbr, kinds, active, seq)
        return f

    def cost(D, seq):
        if inside[0]:
            costed.append(list(seq))
        return sr_cost(D, seq)

    def apply2(succ, d, seq, c=None):
        if d[1] == 0:
            n = len(succ)
            slot = SR._slots(n, seq)
            seen["rev2"].append(abs(int(slot[d[2] // n]) - int(slot[d[2] % n])))
        return sr_apply(succ, d, seq, c)

    def apply3(succ, d, seq, c=None):
        if d[1] == 2:
            slot = SR._slots(len(succ), seq)
            at = [int(slot[x]) for x in N3.decode(int(d[2]), len(succ))[:3]]
            seen["span3"].append(max(at) - min(at))
        return s3_apply(succ, d, seq, c)

    SR.window_candidates, S3.window_candidates = cand(sr_cand), cand(s3_cand)
    SR.apply_window_move, S3.apply_window_move = apply2, apply3
    SR.kick, SR.window_cost = kick, cost
    SR.trial, S3.trial, SL.trial = (trial(t) for t in trials)
    try:
        yield seen
    finally:
        SR.window_candidates, S3.window_candidates, SR.apply_window_move, S3.apply_window_move = sr_cand, s3_cand, sr_apply, s3_apply
        SR.kick, SR.window_cost = sr_kick, sr_cost
        SR.trial, S3.trial, SL.trial = trials


def stale_slots(seq, fin, threads=THREADS):
    """A trial that took the window seq to fin and was rejected is restored over the hull of what it permuted, which begins at
    or before the first slot lo where the two differ -> (hi - lo + 1, the nodes whose slot changed and whose own slot lies more
    than `threads` slots behind lo: the ones a restore of the first `threads` slots of the hull alone would leave with the
    rejected window's slot)."""
    diff = [k for k in range(len(seq)) if seq[k] != fin[k]]
    if not diff:
        return 0, set()
    return diff[-1] - diff[0] + 1, {int(seq[k]) for k in diff if k >= diff[0] + threads}


def lk_log_sizes(log):
    """seg_lk_ref's log -> (the active set of every decision, the slots of every applied chain's hull)"""
    active = [r[1] for r in log if r[0] == "decision"]
    hulls = [max(hi for _, hi in r[4]) - min(lo for lo, _ in r[4]) + 1 for r in log if r[0] == "chain"]
    return active, hulls


def straddles(start, seed, W, it=0):
    """a window of iteration `it` of the tour `start` lies across position n - 1 of the device's order, which starts at node 0"""
    n = len(start)
    p0 = int(np.flatnonzero(NL.R.tour_order(start) == SR.anchor(n, seed, 0, it))[0])
    return any(p0 + w * W <= n - 1 < p0 + w * W + W - 1 for w in range(n // W))


def consistent(entry, c, iterations, trials):
    """the relations between the counters of one state; c as kept() returns it"""
    kinds = c["moves_2opt"] + c["moves_oropt"] + c.get("moves_3opt", 0) + c.get("moves_lk", 0)
    assert c["moves"] == kinds, c
    assert sum(c["moves_by_len"]) == c["moves_oropt"] and sum(c.get("moves_by_type", [])) == c.get("moves_3opt", 0), c
    assert c["iterations"] == iterations
    assert c["trials"] == iterations * c["windows"] * c.get("groups", 1) * trials, c
    assert 0 <= c["accepted"] <= c["trials"] and c["moves"] <= c["decisions"] <= c["moves"] + c["trials"], c
    if "offers" in c:
        assert c["commits"] <= c["offers"] <= c["trials"], c
    if "moves_lk" in c:
        assert c["moves_lk"] <= c["lk_flips"] <= c["lk_steps"] and c["lk_flips"] <= c["moves_lk"] * c["lk_depth"], c
        assert c["lk_chains"] <= 2 * c["active_nodes"], c


# ---- the inline cases of tests/test_gpu_seg_golden.py: non-integer costs at windows whose cost tree is deeper than one pass ------------

# name: (instance, metric or None for the file's, K, W, G, T, iterations, seed).  P is the tree's width, the next power of two
# >= W - 1; its first level has P / 2 entries
INLINE = {
    "u724": ("u724", None, 5, 723, 4, 2, 3, 3),              # W = n - 1: P = 1024, W - 1 no multiple of 8
    "pr1002": ("pr1002", None, 10, 1001, 2, 2, 2, 3),        # P = 1024
    "rand600": ("rand600", None, 5, 518, 2, 2, 2, 3),        # W - 1 = 517: P = 1024, the first size of two strided passes
    "rand1100": ("rand1100", None, 5, 1025, 2, 2, 2, 3),     # W - 1 = 1024 = P: no padding
    "u724-att": ("u724", "ATT", 5, 650, 2, 2, 2, 3),
    # a lattice: many tours of the same edge lengths in another order, and moves whose gain is exactly zero
    "lattice729": ("lattice729", None, 6, 700, 2, 2, 3, 3),
    "lattice1089": ("lattice1089", None, 6, 1025, 2, 2, 2, 3),
    # one node far away: its two edges absorb the low bits of the partial sums they meet, and which partial sums those are is
    # the order of the sum.  For the kick alone (max_moves = 0), where no gain of a move is formed
    "far600": ("far600", None, 5, 518, 2, 2, 2, 3),
    "far1100": ("far1100", None, 5, 1025, 2, 2, 2, 3),
}
DESCENTS = [name for name in INLINE if not name.startswith("far")]
KICKS = ["u724", "rand600", "rand1100", "lattice729", "far600", "far1100"]
FAR = (1e22, 0.37e22)


def lattice(n, step=1000.0):
    side = int(round(n ** 0.5))
    assert side * side == n
    i = np.arange(n)
    return np.stack([(i % side) * step, (i // side) * step], axis=1).astype(np.float64)


def inline_instance(name):
    """-> (xy, wt, the oracle's greedy tour under non-integer costs)"""
    src, metric = INLINE[name][:2]
    if src.startswith("lattice"):
        xy, wt = lattice(int(src[7:])), O.EUC_2D
    elif src.startswith("far"):
        xy, wt = rand_instance(int(src[3:])), O.EUC_2D
        xy[0] = FAR
    else:
        xy, wt = load_instance(src)
    wt = getattr(O, metric) if metric else wt
    return xy, wt, np.asarray(O.greedy(xy, wt, integer_cost=0)[1], dtype=np.int32)



def window_cost_pairs(D, seq):
    """seg_ils_ref.window_cost with every level folded over the pairs (2 k, 2 k + 1): the same sum in an order the definition
    does not allow.  tests/test_cpu_seg_golden.py holds the far instances to telling the two apart."""
    W = len(seq)
    P = 1
    while P < W - 1:
        P *= 2
    a, c = np.asarray(seq[:-1]), np.asarray(seq[1:])
    x = np.zeros(P, dtype=np.float64)
    x[:W - 1] = D[np.minimum(a, c), np.maximum(a, c)]
    while len(x) > 1:
        x = x[0::2] + x[1::2]
    return float(x[0])


def kick_runs(D, nbr, start, W, seeds=20):
    """the kick-alone calls of tests/test_gpu_seg_golden.py by the reference -> [(succ, cost, counters)] per seed"""
    return [S3.run(D, start, nbr, 7, seed, 0, 3, W, 0, 2, max_moves=0) for seed in range(seeds)]
