"""The wall time per exhaustive sweep (k_move_pos + k_exh, two_opt_exh.hpp) of rand10000 when 1 000 sweeps are queued without a
poll: how long the host takes to queue them, and when the last one is done.  TSP_LIB_DIR: another build, for a before / after.
usage: exh_host_rate.py [label] [repeats]"""
import os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, 'tests'))
import numpy as np
os.environ["TSP_NO_FILTER"] = "1"
from tsp_optimization_amd import engine as E
from helpers import load_instance

label = sys.argv[1] if len(sys.argv) > 1 else "build"
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
N = 1000
ctx = E.Context(0)
xy, wt = load_instance('rand10000')
inst = E.Instance(ctx, xy, wt, 1)
succ, obj, _ = inst.construct(E.GREEDY, np.array([0], dtype=np.int32))
t = E.Tours(inst, 1)
assert "k_exh" in t.describe(E.BEST)
t.upload(succ[0], obj[0])
t.run(E.BEST, max_steps=20)   # warm-up
for _ in range(repeats):
    t.upload(succ[0], obj[0])   # (the descent from the greedy tour has 1 428 sweeps)
    t.download()
    t0 = time.perf_counter()
    t.run(E.BEST, max_steps=N, sync=False)
    t1 = time.perf_counter()
    _, _, st = t.download()   # waits for the stream
    t2 = time.perf_counter()
    assert st[0]["sweeps"] == N, st[0]
    print("%s: queued %d sweeps in %.2f us each; all done after %.2f us each" % (label, N, (t1 - t0) / N * 1e6, (t2 - t0) / N * 1e6), flush=True)
