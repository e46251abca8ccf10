"""GPU: runs of tabu() iterations (tabusearch.c:238-309) on the device against the oracle's trajectories, iteration by iteration.

The expected trajectories (tests/golden/tabu_chains.json, tests/golden/make_golden_tabu.py) come from the oracle's
alg_2opt_tabu and tests/tabu_ref.replay alone; they are a function of one ordered stream of node pairs, whatever way the
iterations are cut into calls.  The driver below follows tsp_host_tabu's protocol -- a call gets the next P pairs of the stream,
the position advances by the trials the device reports, a rejected last kick is finished with tsp_dev_tours_tabu_kick one pair at
a time -- and compares EVERY iteration, exactly (all costs are integers): cost after the descent, improved flag, trials, the
running best; at the checkpoints that fall on a call boundary the tour and the non-zero stamps; at the end the incumbent.

What varies: the path (iterations inside one launch; launches queued back to back; one by one; the GRID engine), the cut into
calls, the number of workgroups of the CLUSTER engine (by default 34 at pr1002, 12 at att532, 256 at n = 3000; forced 8, 64, 256
-- at 256 most workgroups of a small instance have no group pair and still take part in the exchange) and the time limit (with
one, as tsp_host_tabu always has, launches end after 128 sweeps and a chain resumes in the middle of an iteration).  On the two
chain paths a call that completes no iteration is a failure: every case meets the conditions of tsp_grid_tabu_iterations."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from helpers import golden, HostInstance, Instance
import tabu_cases as TC
import tabu_ref as T

pytestmark = pytest.mark.gpu

G = golden("tabu_chains.json")
SPLIT_ORDER = ["steps", "eights", "exact", "host"]


@pytest.fixture(scope="module")
def eng():
    from tsp_optimization_amd import engine as E
    assert E.device_count() >= 1, "no HIP device visible: the product path has no CPU fallback"
    return E


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.Context(0)
    yield c
    c.close()


def _params():
    """(case, path, split, TSP_CLUSTER_BLOCKS or None, time limit, iterations or None).  Not the full cross product: the in-kernel
    path ("ex") with every (case, cluster size, time limit); every path, split, cluster size and time limit with every case."""
    out = []
    for case in TC.CASES:
        blocks = [None, 8, 64, 256] if case in ("pr1002", "att532", "d493") else [None]
        combos = [(b, tl) for b in blocks for tl in (-1.0, 600.0)]
        if len(combos) == 8:
            for i, (b, tl) in enumerate(combos):
                out.append((case, "ex", SPLIT_ORDER[(i + i // 2) % 4], b, tl, None))
            out += [(case, "queued", "host", None, 600.0, None), (case, "queued", "eights", 64, -1.0, None),
                    (case, "single", "steps", None, -1.0, None), (case, "single", "steps", 256, 600.0, None)]
        else:
            out += [(case, "ex", "steps", None, -1.0, None), (case, "ex", "exact", None, 600.0, None),
                    (case, "queued", "host", None, 600.0, None), (case, "single", "eights", None, -1.0, None)]
    # the GRID engine forced, one by one: the first 64 iterations of two cases (it takes two waits per iteration)
    out += [("pr1002", "grid", "steps", None, -1.0, 64), ("att532", "grid", "steps", None, -1.0, 64)]
    return out


PARAMS = _params()


def _id(p):
    case, path, split, blocks, tl, iters = p
    return "%s-%s-%s-C%s-tl%d%s" % (case, path, split, "nat" if blocks is None else blocks, tl, "" if iters is None else "-%dit" % iters)


def run_case(eng, ctx, monkeypatch, case, path, split, blocks, tl, iterations):
    rec = G["cases"][case]
    if blocks is not None:
        monkeypatch.setenv("TSP_CLUSTER_BLOCKS", str(blocks))     # (switches are read when the instance handle is made)
    if path == "queued":
        monkeypatch.setenv("TSP_TABU_INKERNEL", "0")
    if path == "grid":
        monkeypatch.setenv("TSP_ENGINE", "1")
    xy, wt, ic = TC.instance_of(case)
    n = len(xy)
    total = rec["iterations"] if iterations is None else iterations
    assert n == rec["n"] and wt == rec["wtype"] and ic == rec["integer_cost"] and total <= rec["iterations"]
    want_obj, want_imp, want_tri, tenures = rec["obj"], rec["improved"], rec["trials"], rec["tenures"]
    running = np.minimum.accumulate(np.array(want_obj))
    cps = {c["iteration"]: c for c in rec["checkpoints"]}
    pairs = np.array(rec["pairs"], dtype=np.int32)
    inst = eng.Instance(ctx, xy, wt, ic)
    tours, tabu = eng.Tours(inst, 1), eng.Tabu(inst)
    tours.upload(np.array(rec["start"], dtype=np.int32), rec["start_cost"])
    p, it, best, seen = 0, 1, float("inf"), []
    for K in TC.split_calls(split, total):
        end = it + K - 1
        while it <= end:                                  # (a chain that stops early: the rest of the call is asked for again)
            left = end - it + 1
            tens = tenures[it - 1:it - 1 + left]
            where = "%s %s: call from iteration %d (%d asked, stream position %d)" % (case, path, it, left, p)
            if path == "ex":
                P = TC.pairs_of_call(split, left)
                assert p + P <= len(pairs)
                rc, done, acc, best, objs, imps, tris = tours.tabu_iterations_ex(tabu, it, tens, pairs[p:p + P], best, tl)
            elif path == "queued":
                rc, done, acc, best, objs, imps = tours.tabu_iterations(tabu, it, tens, pairs[p:p + left], best, tl)
                tris = [1] * done
            else:
                rc, obj, best, imp, acc = tours.tabu_iteration(tabu, it, tens[0], int(pairs[p, 0]), int(pairs[p, 1]), best, tl)
                done, objs, imps, tris = 1, [obj], [int(imp)], [1]
            assert rc == 0, where
            assert done >= 1, where + ": the chain completed no iteration"
            tris = [int(t) for t in tris]
            p += sum(tris)
            last = it + done - 1
            while not acc:                                # :262-287, the trials after a rejected one, one launch each
                acc = tours.tabu_kick(tabu, int(pairs[p, 0]), int(pairs[p, 1]), last, tenures[last - 1])
                p += 1
                tris[-1] += 1
            for k in range(done):
                g = it - 1 + k
                got = (objs[k], int(imps[k]), tris[k])
                assert got == (want_obj[g], want_imp[g], want_tri[g]), "%s: iteration %d (obj, improved, trials) %s, oracle %s" % (
                    where, g + 1, got, (want_obj[g], want_imp[g], want_tri[g]))
            assert best == running[last - 1], "%s: best %s after iteration %d, oracle %s" % (where, best, last, running[last - 1])
            it = last + 1
        if end in cps:
            sd, od, _ = tours.download()
            assert O.fnv1a(sd[0]) == cps[end]["tour_hash"], "%s %s: tour after iteration %d" % (case, path, end)
            if end == rec["iterations"]:
                assert (sd[0] == np.array(rec["tour"], dtype=np.int32)).all()
            st = tabu.download()
            idx, val = T.sparse(st)
            assert (idx.tolist(), val.tolist()) == (cps[end]["stamps"][0], cps[end]["stamps"][1]), "%s %s: stamps after iteration %d" % (case, path, end)
            seen.append(end)
    assert it == total + 1 and (total < rec["iterations"] or p == rec["consumed"])
    assert len(seen) >= (1 if split == "host" else 3) and seen[-1] == total
    # the incumbent kept on the device: the same cycle (either orientation) and its cost
    tours.restore()
    sd, od, _ = tours.download()
    inc = T.canonical_cycle(sd[0])
    assert od[0] == best == cps[total]["best"] and O.succ_cost(xy, wt, sd[0], integer_cost=ic) == best
    assert O.fnv1a(inc) == cps[total]["incumbent_hash"]
    if total == rec["iterations"]:
        assert best == rec["incumbent_cost"] and (inc == T.canonical_cycle(np.array(rec["incumbent"], dtype=np.int32))).all()
    tabu.close(); tours.close(); inst.close()


@pytest.mark.parametrize("param", PARAMS, ids=[_id(p) for p in PARAMS])
def test_tabu_iterations_follow_the_oracles_trajectory(eng, ctx, monkeypatch, param):
    run_case(eng, ctx, monkeypatch, *param)


# ---- host level: tsp_host_tabu against O.tabu's committed runs ---------------------------------------------------------------
@pytest.fixture(scope="module")
def host(eng):
    from tsp_optimization_amd.build import lib_path
    L = C.CDLL(lib_path("libtsp_host.so"))
    L.tsp_host_tabu.argtypes = [C.POINTER(Instance), C.c_int, C.c_longlong]
    L.tsp_host_random_lookahead.restype = C.c_int
    yield L
    L.tsp_host_shutdown()


def _host_run(name, policy):
    return next(r for r in G["host_runs"] if r["instance"] == name and r["policy"] == policy)


HOST_PARAMS = [("pr1002", 0, {}), ("pr1002", 1, {}), ("pr1002", 2, {}),
               ("pr1002", 0, {"TSP_TABU_CHAIN": "1"}), ("pr1002", 0, {"TSP_TABU_CHAIN": "32"}), ("pr1002", 0, {"TSP_TABU_INKERNEL": "0"}),
               ("att532", 0, {})]


@pytest.mark.parametrize("name,policy,env", HOST_PARAMS,
                         ids=["%s-policy%d-%s" % (nm, pol, "-".join("%s=%s" % kv for kv in env.items()) or "default") for nm, pol, env in HOST_PARAMS])
def test_host_tabu_gives_the_oracles_run(host, monkeypatch, name, policy, env):
    """tsp_host_tabu for 300 iterations of the libc stream seeded with 123, with a time limit (as the CLI always has): chains of
    128 iterations that resume in the middle of iterations, 34 or 12 workgroups.  The incumbent tour, its cost and the next value
    of libc's random() after the run equal the committed run of O.tabu; nothing is held back in the library."""
    monkeypatch.delenv("TSP_TABU_CHAIN", raising=False)
    monkeypatch.delenv("TSP_TABU_INKERNEL", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = _host_run(name, policy)
    libc = C.CDLL(None)
    libc.random.restype = C.c_long
    h = HostInstance(name)
    h.c.params.time_limit = 600
    O.srandom(want["seed"])
    rc = host.tsp_host_tabu(C.byref(h.c), policy, want["iterations"])
    assert host.tsp_host_random_lookahead() == 0
    nxt = libc.random()
    assert rc == 0 and h.obj == want["cost"] and (h.succ == np.array(want["incumbent"], dtype=np.int32)).all()
    assert nxt == want["next_random"]
