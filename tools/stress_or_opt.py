"""Randomised Or-opt parity sweep: random sizes around the wave / row-group / chunk boundaries of csrc/or_opt.hip, the five
planar metrics, coordinates that select the *_ICOORD and the general kernel instances, both cost modes, random / greedy /
2-opt-optimal start tours and move caps -- tsp_dev_or_opt against tests/or_opt_ref.py bit for bit (tour, cost, every
counter), full sweeps against the incremental path, the *_ICOORD instance against the general one, batches against single
calls, and tsp_dev_two_opt_or_opt against the reference's alternation.  `run(seed, cases)` returns the number of
mismatching cases (it stops at the first); tests/test_gpu_or_opt_stress.py runs a seeded slice of it under `-m gpu`, and
as a script SEED=<n> CASES=<n> select a longer run."""
import os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if R not in sys.path: sys.path.insert(0, R)
if os.path.join(R, 'tests') not in sys.path: sys.path.insert(0, os.path.join(R, 'tests'))
import numpy as np
SIZES = [5, 6, 7, 8, 9, 12, 13, 31, 61, 62, 63, 64, 65, 124, 125, 126, 127, 186, 187, 255, 256, 257, 511, 512, 513]
SWITCHES = ("TSP_OROPT_FULL", "TSP_NO_ICOORD")
TIME_LIMIT = 120.0          # every device call: a descent that does not end comes back as status 2, a mismatch
COUNTERS = ("sweeps", "evals", "moves", "moves_by_len", "moves_reversed")


def run(seed, cases, ctx=None, verbose=True, max_n=600):
    prev = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES: os.environ.pop(k, None)
    try:
        return _run(seed, cases, ctx, verbose, max_n)
    finally:
        for k, v in prev.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


FAILED_AT = []


def _chk(ok, what, cond):
    if ok and not cond:
        FAILED_AT.append(what)      # the first check of the case that failed
    return bool(ok and cond)


def _same_run(a, b, with_deltas=True):
    """Two device results (rc, succ, obj, stats) are identical."""
    keys = COUNTERS + (("deltas_executed",) if with_deltas else ())
    return a[0] == b[0] == 0 and (a[1] == b[1]).all() and a[2] == b[2] and all(a[3][k] == b[3][k] for k in keys)


def _run(seed, cases, ctx, verbose, max_n):
    from tsp_optimization_amd import engine as E
    from helpers import random_tour
    from oracle import oracle as O
    import or_opt_ref as RF
    own = ctx is None
    if own: ctx = E.Context(0)
    rng = np.random.default_rng(seed)
    bad = 0
    for c in range(cases):
        t_case = time.perf_counter()
        n = int(rng.choice(SIZES)) if rng.random() < 0.6 else int(rng.integers(5, 601))
        n = min(n, max_n)
        wt = int(rng.choice([O.EUC_2D, O.ATT, O.CEIL_2D, O.MAN_2D, O.MAX_2D]))
        kind = str(rng.choice(["i20", "i1k", "i1m", "i3m", "float"]))
        hi = {"i20": 20, "i1k": 1000, "i1m": 1_000_000, "i3m": 3_000_000}.get(kind)
        xy = rng.integers(0, hi, size=(n, 2)).astype(np.float64) if hi else rng.uniform(-5000, 5000, size=(n, 2))
        ic = int(rng.random() < 0.6)
        # float costs with exactly tied distances (integer coordinates on EUC_2D / ATT) and float coordinates on MAN_2D /
        # MAX_2D (dy = |y2 - y2|) can make a best-improvement descent cycle on rounding noise: integer costs there.
        # CEIL_2D, and MAN_2D / MAX_2D on integer coordinates, have integer-valued distances in both cost modes.
        if (hi and wt in (O.EUC_2D, O.ATT)) or (not hi and wt in (O.MAN_2D, O.MAX_2D)): ic = 1
        exact = ic or wt in (O.CEIL_2D, O.MAN_2D, O.MAX_2D)   # integer-valued distances: no descent cycles on noise
        span = float(np.hypot(*(xy.max(0) - xy.min(0))))
        icoord = bool(hi) and span < 2097151.0 and (wt == O.CEIL_2D or (ic and wt in (O.EUC_2D, O.ATT)))
        D = O.dist_matrix(xy, wt, ic)
        # start tour
        sk = rng.random()
        _, es, eo = O.greedy(xy, wt, int(rng.integers(0, n)), ic)
        if sk < 0.4: start, tour = "random", random_tour(n, rng)
        elif sk < 0.7: start, tour = "greedy", es
        else:
            start = "2opt"
            _, tour, _, _, _ = O.two_opt_first(xy, wt, es, eo, ic)
        tour = np.array(tour, dtype=np.int32)
        # move cap: -1 / 0 / random; random starts beyond n = 300 and --fcost always carry one
        r = rng.random()
        cap = -1 if r < 0.5 else (0 if r < 0.6 else int(rng.integers(1, 80)))
        if cap < 0 and (not ic or (start == "random" and n > 300)): cap = int(rng.integers(40, 200))
        ok = True
        ref, rc_ = RF.or_opt_descent(xy, wt, tour, ic, max_moves=cap, D=D)
        inst = E.Instance(ctx, xy, wt, ic)
        d = inst.or_opt(tour, max_moves=cap, time_limit=TIME_LIMIT)
        rc, s, o, st = d
        cost = O.succ_cost(xy, wt, s, ic)
        ok = _chk(ok, "device vs reference", rc == 0 and (s == ref).all() and all(st[k] == rc_[k] for k in COUNTERS)
                  and (o == cost if ic else abs(o - cost) <= 1e-9 * abs(cost)))
        # full sweeps: the same decisions
        os.environ["TSP_OROPT_FULL"] = "1"
        inst.reload_switches()
        f = inst.or_opt(tour, max_moves=cap, time_limit=TIME_LIMIT)
        os.environ.pop("TSP_OROPT_FULL")
        inst.reload_switches()
        ok = _chk(ok, "full vs incremental", _same_run(d, f, with_deltas=False))
        if icoord:   # the general instance of the same metric
            os.environ["TSP_NO_ICOORD"] = "1"
            ig = E.Instance(ctx, xy, wt, ic)
            os.environ.pop("TSP_NO_ICOORD")
            g = ig.or_opt(tour, max_moves=cap, time_limit=TIME_LIMIT)
            ig.close()
            ok = _chk(ok, "ICOORD vs general", _same_run(d, g))
        nb = 0
        if rng.random() < 0.35:
            # a batch: this tour, an Or-opt-optimal one and random ones; large n keeps the batch short and capped
            nb = int(rng.choice([2, 3, 5, 8] if n <= 128 else [2, 3]))
            bcap = cap if n <= 256 else (0 if cap == 0 else int(rng.integers(1, 40)))
            opt, _ = RF.or_opt_descent(xy, wt, es, ic, D=D) if (n <= 256 and exact) else (ref, None)
            tours = [tour, np.array(opt, dtype=np.int32)] + [random_tour(n, rng) for _ in range(nb - 2)]
            order = rng.permutation(nb)
            tours = np.stack([tours[q] for q in order])
            rb, sb, ob, stb = inst.or_opt(tours, max_moves=bcap, time_limit=TIME_LIMIT)
            ok = _chk(ok, "batch status", rb == 0)
            for b in range(nb):
                if not ok: break
                one = inst.or_opt(tours[b], max_moves=bcap, time_limit=TIME_LIMIT)
                ok = _chk(ok, "batch vs single call", _same_run(one, (rb, sb[b], ob[b], stb[b])))
                rr, rcb = RF.or_opt_descent(xy, wt, tours[b], ic, max_moves=bcap, D=D)
                ok = _chk(ok, "batch vs reference", (sb[b] == rr).all() and all(stb[b][k] == rcb[k] for k in COUNTERS))
        if n <= 300 and exact:
            # the composite from greedy, both 2-opt rules, against the reference's alternation
            for mode in (E.FIRST, E.BEST):
                rc2, s2, o2, _, so2 = inst.two_opt_or_opt(es, eo, mode=mode, time_limit=TIME_LIMIT)
                rs, ro, rounds = RF.two_opt_or_opt(xy, wt, es, eo, mode=mode, integer_cost=ic, D=D)
                ok = _chk(ok, "composite mode %d" % mode, rc2 == 0 and (s2 == rs).all() and o2 == ro and so2["rounds"] == rounds)
        inst.close()
        if verbose:
            print("case %d n %d wt %d ic %d %s %s cap %d batch %d moves %d %s  %.2f s" % (
                c, n, wt, ic, kind, start, cap, nb, st["moves"], "ok" if ok else "MISMATCH", time.perf_counter() - t_case),
                flush=True)
        if not ok:
            bad += 1
            print("MISMATCH case %d: n %d wt %d ic %d coords %s start %s cap %d batch %d, first failing check: %s" % (
                c, n, wt, ic, kind, start, cap, nb, FAILED_AT[-1:]))
            break
    if own: ctx.close()
    return bad


if __name__ == "__main__":
    n_cases = int(os.environ.get("CASES", "60"))
    n_bad = run(int(os.environ.get("SEED", "1")), n_cases)
    print("cases %d, mismatches %d" % (n_cases, n_bad))
    sys.exit(1 if n_bad else 0)
