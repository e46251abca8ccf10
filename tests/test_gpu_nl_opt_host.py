"""GPU: the neighbour-list descent through the C host mirror (libtsp_host.so: alg_nl_opt, HEU_nl_greedy / _grasp /
_extramileage, tsp_host_set_knn, tsp_host_last_nl_stats) on the reference's `instance` struct, against the device API and the
CPU reference (tests/nl_opt_ref.py).  The `tsp` command line has no NL_* rows (tests/test_cpu_or_opt.py pins its method table);
what is checked of it here is that every existing method string still resolves to its own row."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import nl_opt_ref as NL
from helpers import Instance, HostInstance
from oracle import oracle as O

pytestmark = pytest.mark.gpu
COUNTERS = ("decisions", "moves", "moves_2opt", "moves_oropt", "moves_by_len", "moves_reversed", "reversed")


@pytest.fixture(scope="module")
def eng():
    from tsp_optimization_amd import engine as E
    assert E.device_count() >= 1
    return E


@pytest.fixture(scope="module")
def host(eng):
    from tsp_optimization_amd.build import lib_path
    L = C.CDLL(lib_path("libtsp_host.so"))
    for f in ["alg_nl_opt", "HEU_nl_greedy", "HEU_nl_grasp", "HEU_nl_extramileage", "HEU_greedy", "HEU_Grasp", "HEU_extramileage"]:
        getattr(L, f).argtypes = [C.POINTER(Instance)]
    L.tsp_host_set_knn.argtypes = [C.c_int]
    L.tsp_host_last_nl_stats.argtypes = [C.POINTER(eng.NlOptStats)]
    yield L
    L.tsp_host_set_knn(eng.NL_DEFAULT_K)
    L.tsp_host_shutdown()


def nl_stats(eng, L):
    st = eng.NlOptStats()
    L.tsp_host_last_nl_stats(C.byref(st))
    return st.as_dict()


def device_path(eng, xy, wt, succ, K):
    ctx = eng.Context(0)
    inst = eng.Instance(ctx, xy, wt, 1)
    inst.knn_build(K)
    out = inst.nl_opt(succ, time_limit=300.0)
    inst.close()
    ctx.close()
    return out


@pytest.mark.parametrize("name", ["pr299", "att532", "pr1002"])
def test_alg_nl_opt_on_the_instance_struct_equals_the_device_api(eng, host, name):
    assert host.tsp_host_set_knn(10) == 0
    h = HostInstance(name)
    assert host.HEU_greedy(C.byref(h.c)) == 0
    start = h.succ
    assert host.alg_nl_opt(C.byref(h.c)) == 0
    rc, s, o, st = device_path(eng, h.xy, h.wt, start, 10)
    assert rc == 0 and (h.succ == s).all() and h.obj == o == O.succ_cost(h.xy, h.wt, s)
    hs = nl_stats(eng, host)
    for k in COUNTERS:
        assert hs[k] == st[k], k
    assert hs["moves"] > 0


@pytest.mark.parametrize("method,construct", [("HEU_nl_greedy", "HEU_greedy"), ("HEU_nl_grasp", "HEU_Grasp"),
                                              ("HEU_nl_extramileage", "HEU_extramileage")])
def test_constructions_then_alg_nl_opt_equal_the_python_path(eng, host, method, construct):
    """seed 123, as `tsp -seed 123` sets it: the cost is the recomputed cost of the tour that the Python path gives for the
    same construction."""
    assert host.tsp_host_set_knn(10) == 0
    h0 = HostInstance("att532")
    O.srandom(123)
    getattr(host, construct)(C.byref(h0.c))
    h = HostInstance("att532")
    O.srandom(123)
    assert getattr(host, method)(C.byref(h.c)) == 0
    rc, s, o, st = device_path(eng, h.xy, h.wt, h0.succ, 10)
    assert rc == 0 and (h.succ == s).all() and h.obj == o == O.succ_cost(h.xy, h.wt, s)
    D = O.dist_matrix(h.xy, h.wt, 1)
    ref, c = NL.descent(D, h0.succ, NL.knn(D, 10), 3)
    assert (h.succ == ref).all()
    hs = nl_stats(eng, host)
    for k in COUNTERS:
        assert hs[k] == c[k], k


def test_set_knn_changes_the_lists(eng, host):
    h = HostInstance("pr299")
    D = O.dist_matrix(h.xy, h.wt, 1)
    _, es, _ = O.greedy(h.xy, h.wt)
    got = {}
    for K in (5, 10, 5):
        assert host.tsp_host_set_knn(K) == 0
        assert host.HEU_nl_greedy(C.byref(h.c)) == 0
        ref, c = NL.descent(D, es, NL.knn(D, K), 3)
        assert (h.succ == ref).all() and h.obj == O.succ_cost(h.xy, h.wt, ref), K
        assert nl_stats(eng, host)["moves"] == c["moves"]
        got[K] = h.succ
    assert not (got[5] == got[10]).all()
    for K in (0, 17, -1):
        assert host.tsp_host_set_knn(K) == -3
    assert host.HEU_nl_greedy(C.byref(h.c)) == 0 and (h.succ == got[5]).all()   # a refused K leaves the last one in place
    # fewer nodes than K + 1: the lists are the n - 1 other nodes
    host.tsp_host_set_knn(16)
    small = HostInstance("burma14")
    assert host.HEU_nl_greedy(C.byref(small.c)) == 0
    rc, s13, o13, _ = device_path(eng, small.xy, small.wt, O.greedy(small.xy, small.wt)[1], 13)
    assert rc == 0 and (small.succ == s13).all() and small.obj == o13
    assert O.is_tour(small.succ)


def test_every_existing_method_string_still_resolves_to_its_row():
    from tsp_optimization_amd.build import lib_path
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tsp_optimization_amd", "host", "tsp_host.c")) as f:
        table = re.findall(r'\{"(\w+)", (\d+), (SOLVE_\w+), "', f.read())
    r = subprocess.run([lib_path("tsp"), "--methods"], capture_output=True, text=True)
    rows = [ln.split()[0] for ln in r.stdout.splitlines() if ln.strip()]
    assert r.returncode == 0 and rows == [t[0] for t in table] and len(rows) == 20

    def resolve(m):
        got = None
        for prefix, ln, sid in table:
            if len(m) >= int(ln) and m[:int(ln)] == prefix[:int(ln)]:
                got = sid
        return got

    for prefix, _, sid in table:
        assert resolve(prefix) == sid, prefix
    assert not any(t[0].startswith("NL_") for t in table)
