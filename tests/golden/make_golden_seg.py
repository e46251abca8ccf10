"""Records tests/golden/seg_runs.json: results of the CPU references of the windowed iterated local search (tests/seg_ils_ref.py,
seg_ils3_ref.py, seg_groups_ref.py, seg_lk_ref.py through their run(); never the device) at the shapes the search works at, which
are beyond the inline references of tests/test_gpu_seg_*.py.  The cases are those of tests/seg_golden_cases.py.  Every state is kept
as the SHA-256 of the tour's int32 little-endian bytes, its cost (oracle.succ_cost), the counters of the entry point's reference
(COUNTERS of its module) and start_cost; every run also keeps "worth", the quantities that make it worth its name, which this
recorder asserts.

S1  rand_instance(1100), one window of 1024, span W - 1, one trial from a random tour, to the end, through tsp_dev_seg_ils (kinds
    3), _seg_ils3 (7), _seg_ils_groups (7, two groups), _seg_ils_lk (15 and 8 alone, one group, D = 16): four instantiations of
    k_seg_ils.  The active set of a decision grows past the 256 threads of a workgroup (971 nodes under kinds 15), and so do an
    applied reversal, a 3-opt relabeling and a chain's hull; the trial is accepted.
S2  rand_instance(2100, hi = 100000), W = 2048, kinds 15, D = 16, the start and seed of test_the_largest_window in
    tests/test_gpu_seg_lk.py, not cut: active sets and permuted intervals of more than 1024.
S3  rand_instance(5000) from the oracle's greedy tour, W = 64 (78 windows, one of them across position n - 1), span 50, two
    trials, kinds 3 and 7 without groups: the states after 1, 2 and 3 iterations, each a call of its own.  In every iteration
    more than half of the windows accept and write order / pos while the others read pos.
S4  the same instance and start with groups: W = 64, G = 16 (1248 workgroups, more than are resident), one trial, two
    iterations, kinds 7 and 15; W = 1024 (4 windows), G = 16, four trials, two iterations, kinds 15; W = 256 (19 windows), G = 8,
    two trials, three iterations, kinds 15, all with span 50.  Fewer commits than offers, a committed record of a window and a
    group behind the first, and (W = 64 and 256; at W = 1024 nearly every offer spans the window and one commits) windows that
    commit two offers or more.  S4-lk-w1024-span0 is W = 1024, G = 4, four trials, one iteration with span W - 1: six trials
    are rejected with another window than they began with, differing over more than 256 slots, and the next trial of their
    group asks for the slot of nodes beyond the first 256 slots of that hull: the restore branch at full length.
S5  kroA100, W = 25, span 10, one trial, from a random tour, kinds 15 with D = 6 and one group, and kinds 7 with three groups:
    the states after 1, 5, 6, 13, 29, 61, 125, 252, 253, 300, 509 and 640 iterations.  Descent::run (csrc/descent.hpp) queues one
    launch and then batches of 4, 8, 16, 32, 64, 128, 256, 256: 640 iterations are nine rounds of queueing, the last one cut at
    131 of its 256 launches; 1, 5, 13, 29, 61, 125, 253 and 509 are the counts at which a time limit can end the call.  Behind
    iteration 100 fewer than a tenth of the trials are accepted: reject and restore.

Times of the references on the recording machine, one core each with seven others busy, the longest state of every run:
S1-ils 134 s, S1-ils3 111 s, S1-groups 204 s, S1-lk 46 s, S1-lk8 9 s, S2-lk 222 s, S3-ils 9 s, S3-ils3 11 s, S4-groups 60 s,
S4-lk 63 s, S4-lk-w1024 26 s, S4-lk-w1024-span0 6 s, S4-lk-w256 28 s, S5-lk 19 s, S5-groups 58 s (alone on the machine about
a quarter less).  The whole recording, its 44 jobs eight side by side, takes 223 s.

The recorder is deterministic: it reproduces the committed file byte for byte.  Run from the repository root, on the CPU:
    python tests/golden/make_golden_seg.py [jobs side by side, default 8]"""
import json
import multiprocessing
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def worth(G, r, c, seen, log, glog, start):
    """the quantities that make the run worth its name, asserted"""
    n_win = c["windows"]
    out = {}
    if r["entry"] == "seg_ils_lk" and r["kinds"] & 8:
        active, hulls = G.lk_log_sizes(log)
        out["max_hull_lk"] = max(hulls) if hulls else 0
    else:
        active = seen["active"]
    out["max_active"] = max(active)
    out["max_rev2"] = max(seen["rev2"]) if seen["rev2"] else 0
    out["max_span3"] = max(seen["span3"]) if seen["span3"] else 0
    out["max_kick"] = max(seen["kick"])
    acc = seen["accepts"]
    assert len(acc) == c["trials"] and sum(acc) == c["accepted"]
    case = r["case"]
    if case in ("S1", "S2"):
        big = G.THREADS if case == "S1" else 1024
        assert out["max_active"] > big, out
        if r["kinds"] & 1:
            assert out["max_rev2"] > big, out
        if r["kinds"] & 4 and case == "S1":
            assert out["max_span3"] > big, out
        if r["kinds"] & 8:
            assert out["max_hull_lk"] > big, out
            assert max(2 * a for a in active) > 4 * G.CHAIN_GROUPS and any(2 * a % G.CHAIN_GROUPS for a in active if 2 * a > G.CHAIN_GROUPS)
            out["partial_chain_pass"] = True
        assert max(out["max_rev2"], out["max_span3"], out.get("max_hull_lk", 0)) > big
        assert acc[0], "the first trial is not accepted"
    if case == "S3":
        per_it = []
        for it in range(max(r["iterations"])):
            per_it.append(len({rec["w"] for rec in log if rec["it"] == it and rec["accepted"]}))
        assert n_win == 78 and all(2 * a > n_win for a in per_it), per_it
        assert G.straddles(start, r["seed"], r["window"])
        out["accepting_windows"] = per_it
        out["straddles"] = True
    if case == "S4" and r["span"] == 0:
        # rejected trials with a trial behind them in their group; of these, the restores whose hull is more than a workgroup's
        # threads and where the next trial asks for the slot of nodes that lie beyond the hull's first 256 slots and sat elsewhere
        # in the rejected window: a restore that stopped after 256 slots would hand it the wrong slots
        T = r["trials"]
        late = [q for q in range(len(acc)) if not acc[q] and q % T < T - 1]
        long = []
        for q in late:
            hull, stale = G.stale_slots(*seen["windows"][q])
            if hull > G.THREADS and stale & seen["touched"][q + 1]:
                long.append((hull, len(stale & seen["touched"][q + 1])))
        assert len(long) >= 2, (len(late), long)
        out["restored_ahead_of_a_trial"] = len(late)
        out["long_restores_read_by_the_next_trial"] = len(long)
        out["longest_restore_hull"] = max(h for h, _ in long)
        out["restored_slots_read_by_the_next_trial"] = sum(k for _, k in long)
    if case == "S4":
        if r["entry"] == "seg_ils_groups":
            per, later = {}, 0
            for it, w, g, offer, gain, lo, hi, kept in glog:
                per[(it, w)] = per.get((it, w), 0) + int(kept)
                later += int(kept and w >= 1 and g >= 1)
            most = max(per.values())
        else:
            most = max(len(keep) for _, _, _, keep in glog)
            later = sum(1 for _, w, _, keep in glog for g in keep if w >= 1 and g >= 1)
        # a committed record of a window >= 1 and a group >= 1: k_seg_ils and k_seg_commit must agree on where it lies
        assert later >= 1
        out["commits_behind_the_first_window_and_group"] = later
        # at W = 1024 nearly every offer spans the window: one commit per window and iteration
        assert c["commits"] < c["offers"] and (most >= 2 or r["window"] == 1024), (c["commits"], c["offers"], most)
        out["workgroups"] = n_win * r["groups"]
        out["most_commits_of_a_window"] = most
        if r["window"] == 64:
            assert out["workgroups"] > G.RESIDENT
    if case == "S5":
        per = n_win * r["groups"] * r["trials"]
        tail = acc[G.S5_DRY_FROM * per:]
        assert len(tail) == (max(r["iterations"]) - G.S5_DRY_FROM) * per and 10 * sum(tail) < len(tail), (sum(tail), len(tail))
        out["accepted_behind_%d" % G.S5_DRY_FROM] = sum(tail)
        assert max(r["iterations"]) > G.BATCH_ENDS[7] and set(G.BATCH_ENDS[:8]) <= set(r["iterations"])
    return out


def job(arg):
    import seg_golden_cases as G
    name, iterations = arg
    r = G.RUNS[name]
    xy, wt, D, nbr, start = G.instance(r["instance"])
    last = iterations == max(r["iterations"])
    log, glog = [], []
    t0 = time.time()
    with G.probe() as seen:
        succ, cost, c = G.ref_run(r, D, start, nbr, iterations, log=log, glog=glog)
    seconds = time.time() - t0
    st = G.state(xy, wt, G.INSTANCES[r["instance"]]["integer_cost"], r["entry"], succ, c)
    assert st["cost"] == cost
    G.consistent(r["entry"], st["counters"], iterations, r["trials"])
    out = {"state": st, "lists_sha": G.sha(nbr), "start_sha": G.sha(start), "seconds": seconds}
    if last:
        try:
            out["worth"] = worth(G, r, st["counters"], seen, log, glog, start)
        except AssertionError as e:          # told at the end, with those of the other runs
            out["failed"] = "%s: %r" % (name, e)
    return name, iterations, out


def main():
    import seg_golden_cases as G
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    jobs = [(name, it) for name, r in G.RUNS.items() for it in r["iterations"]]
    # the long ones first
    jobs.sort(key=lambda j: (-{"S2": 9, "S1": 8, "S4": 7}.get(G.RUNS[j[0]]["case"], 0), -j[1], j[0]))
    t0 = time.time()
    with multiprocessing.Pool(procs) as pool:
        done = {(name, it): out for name, it, out in pool.imap_unordered(job, jobs)}
    failed = [out["failed"] for out in done.values() if "failed" in out]
    assert not failed, "a run does not meet the conditions of its case (choose another seed): " + "; ".join(failed)
    inst, runs = {}, {}
    for name, r in G.RUNS.items():
        states = {}
        for it in r["iterations"]:
            out = done[(name, it)]
            i = inst.setdefault(r["instance"], dict(G.INSTANCES[r["instance"]], lists_sha=out["lists_sha"], start_sha=out["start_sha"]))
            assert (i["lists_sha"], i["start_sha"]) == (out["lists_sha"], out["start_sha"])
            states[str(it)] = out["state"]
        top = done[(name, max(r["iterations"]))]
        runs[name] = dict(r, states=states, worth=top["worth"])
    times = {name: round(done[(name, max(r["iterations"]))]["seconds"]) for name, r in G.RUNS.items()}
    with open(os.path.join(HERE, G.FIXTURE), "w") as f:
        json.dump({"instances": inst, "runs": runs}, f, separators=(",", ":"), sort_keys=True)
    print("recorded in %.0f s; seconds of every run's longest state: %s" % (time.time() - t0, json.dumps(times, sort_keys=True)))
    for name in runs:
        print(name, json.dumps(runs[name]["worth"], sort_keys=True))


if __name__ == "__main__":
    main()
