"""Or-opt descent on rand10000 (greedy -> alg_2opt -> Or-opt, tsp_dev_or_opt): microseconds per move, delta expressions executed
per second and deltas_executed / evals, for the incremental path (default) and a full sweep per decision (TSP_OROPT_FULL=1).
usage: oropt_time.py [incr|full ...]"""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, 'tests'))
import numpy as np
from tsp_optimization_amd import engine as E
from helpers import load_instance

ctx = E.Context(0)
xy, wt = load_instance("rand10000")
inst = E.Instance(ctx, xy, wt, 1)
succ, obj, _ = inst.construct(E.GREEDY, np.array([0], dtype=np.int32))
_, s2, o2, _ = inst.two_opt(succ[0], obj[0], mode=E.FIRST)
print("rand10000 greedy %d -> alg_2opt %d" % (obj[0], o2), flush=True)
for c in sys.argv[1:] or ["incr", "full"]:
    if c == "full":
        os.environ["TSP_OROPT_FULL"] = "1"
    else:
        os.environ.pop("TSP_OROPT_FULL", None)
    inst.reload_switches()
    inst.or_opt(s2, o2)                            # warm-up (buffers, code objects)
    runs = [inst.or_opt(s2, o2) for _ in range(3)]
    rc, s, o, st = min(runs, key=lambda r: r[3]["device_ms"])
    ms = st["device_ms"]
    print("%-4s -> %d: %d moves (by length %s, %d reversed), %d decisions, device %.2f ms (wall %.2f ms): %.1f us per move, "
          "%.3g delta/s executed, deltas_executed / evals = %.5f"
          % (c, o, st["moves"], st["moves_by_len"], st["moves_reversed"], st["sweeps"], ms, 1e3 * st["seconds"],
             1e3 * ms / max(1, st["moves"]), st["deltas_executed"] / (1e-3 * ms), st["deltas_executed"] / st["evals"]), flush=True)
inst.close()
ctx.close()
