"""CPU: the CLUSTER engine's group-pair table (csrc/cluster_deal.hpp) as the very source text tsp_cluster_run builds it with,
compiled with the host compiler (tests/cluster_deal_check.cpp) and compared with a reimplementation of the rule:

  * the pairs r <= c of rank-order groups, sorted by (squared distance of their boxes, id = r << 16 | c);
  * ntests = ceil(npairs / C) slots per workgroup;
  * by cost (one tour on several workgroups, and the tour a permutation of in-range ids): with len(u, v) = scale * |uv| + 1,
    ds[v] = len(v, succ v), inc[v] = max(ds[v], len(v, pred v)), gmx[g] = max inc over the group's nodes, a pair is heavy when
    scale^2 * box distance^2 < (gmx[r] + gmx[c] + 2)^2 and then costs 8 + the rows v of r with
    scale^2 * (distance^2 of v to c's box) < (ds[v] + gmx[c] + 2)^2; the heavy ones go by cost descending (stable) each to the
    workgroup with room that minimises (load, index), the light ones in turn, skipping full rows;
  * else in turn: pair k to workgroup k mod C.

Both sides work on doubles with a correctly rounded sqrt and no fused operation (-ffp-contract=off), so the tables are equal
element for element."""
import math
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsp_optimization_amd", "csrc")

NGS = (1, 2, 3, 7, 12)
CS = (1, 2, 3, 8, 64, 256)
ATT = 1.0 / math.sqrt(10.0)


def _box_d2(rb, cb):
    gx = max(0.0, max(rb[0] - cb[1], cb[0] - rb[1]))
    gy = max(0.0, max(rb[2] - cb[3], cb[2] - rb[3]))
    return gx * gx + gy * gy


def _reference(case):
    n, ng, C, by_cost, scale = case["n"], case["ng"], case["C"], case["by_cost"], case["scale"]
    gbox, sperm, xy, order = case["gbox"], case["sperm"], case["xy"], case["order"]
    pairs = sorted((_box_d2(gbox[r], gbox[c]), (r << 16) | c) for r in range(ng) for c in range(r, ng))
    ntests = -(-len(pairs) // C)
    rows = [[] for _ in range(C)]
    if by_cost and order is not None and all(0 <= v < n for v in order):
        def length(u, v):
            dx, dy = xy[u][0] - xy[v][0], xy[u][1] - xy[v][1]
            return scale * math.sqrt(dx * dx + dy * dy) + 1.0
        ds, inc = [0.0] * n, [0.0] * n
        for q, v in enumerate(order):
            ds[v] = length(v, order[(q + 1) % n])
            inc[v] = max(ds[v], length(v, order[q - 1]))
        gmx = [max([0.0] + [inc[v] for v in sperm[64 * g:64 * g + 64] if v >= 0]) for g in range(ng)]
        heavy, light = [], []
        for d2, e in pairs:
            r, c = e >> 16, e & 0xffff
            T = gmx[r] + gmx[c] + 2.0
            if scale * scale * d2 < T * T:
                live = 0
                for v in sperm[64 * r:64 * r + 64]:
                    if v < 0:
                        continue
                    x, y = xy[v]
                    gx = max(0.0, max(gbox[c][0] - x, x - gbox[c][1]))
                    gy = max(0.0, max(gbox[c][2] - y, y - gbox[c][3]))
                    Tr = ds[v] + gmx[c] + 2.0
                    live += scale * scale * (gx * gx + gy * gy) < Tr * Tr
                heavy.append((8.0 + live, e))
            else:
                light.append(e)
        heavy.sort(key=lambda it: -it[0])   # stable
        load = [0.0] * C
        for cost, e in heavy:
            w = min((load[k], k) for k in range(C) if len(rows[k]) < ntests)[1]
            rows[w].append(e)
            load[w] += cost
        w = 0
        for e in light:
            while len(rows[w]) >= ntests:
                w = (w + 1) % C
            rows[w].append(e)
            w = (w + 1) % C
        case["heavy"], case["light"] = len(heavy), len(light)
    else:
        for k, (_, e) in enumerate(pairs):
            rows[k % C].append(e)
        case["heavy"] = case["light"] = None
    return ntests, [e for row in rows for e in row + [-1] * (ntests - len(row))]


def _points(kind, n, rng):
    if kind == "uniform":
        return [(rng.random() * 1000.0, rng.random() * 1000.0) for _ in range(n)]
    if kind == "lattice":   # many equal lengths, boxes and costs
        return [(float(rng.randrange(8)), float(rng.randrange(8))) for _ in range(n)]
    return [(3.25, -7.5)] * n   # coincident


def _case(kind, ng, C, rng, tour="near", by_cost=True, scale=1.0):
    n = (ng - 1) * 64 + 17   # the last group is partly padding
    xy = _points(kind, n, rng)
    # strips walked up and down in turn: groups with boxes of their own, and no long step between two ranks
    ranked = sorted(range(n), key=lambda v: (xy[v][0] // 125.0, xy[v][1] if xy[v][0] // 125.0 % 2 == 0 else -xy[v][1], v))
    sperm = ranked + [-1] * (ng * 64 - n)
    gbox = []
    for g in range(ng):
        mem = [xy[v] for v in sperm[64 * g:64 * g + 64] if v >= 0]
        gbox.append((min(p[0] for p in mem), max(p[0] for p in mem), min(p[1] for p in mem), max(p[1] for p in mem)))
    if tour == "near":        # short edges: distant group pairs are light
        order = list(ranked)
    elif tour == "random":    # long edges: (almost) every pair is heavy
        order = list(range(n))
        rng.shuffle(order)
    elif tour == "bad":       # one id out of range
        order = list(ranked)
        order[rng.randrange(n)] = n if rng.random() < 0.5 else -1
    else:
        order = None
    return dict(n=n, ng=ng, C=C, by_cost=by_cost, scale=scale, gbox=gbox, sperm=sperm, xy=xy, order=order,
                name="%s ng=%d C=%d tour=%s by_cost=%d scale=%.3f" % (kind, ng, C, tour, by_cost, scale))


def _text(case):
    w = ["%d %d %d %d %d %s" % (case["n"], case["ng"], case["C"], case["by_cost"], case["order"] is not None, case["scale"].hex())]
    w += [v.hex() for box in case["gbox"] for v in box]
    w += [str(v) for v in case["sperm"]]
    w += [v.hex() for p in case["xy"] for v in p]
    w += [str(v) for v in case["order"] or []]
    return " ".join(w)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("cluster_deal") / "cluster_deal_check")
    # plain C++17, nothing of HIP; -ffp-contract=off as in csrc/Makefile
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cluster_deal_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def cases(driver):
    """Every case with the driver's table (`got`) and the rule's (`want`): one run of the driver for all of them."""
    rng = random.Random(20261018)
    out = []
    for ng in NGS:
        for C in CS:
            for kind in ("uniform", "lattice", "coincident"):
                out.append(_case(kind, ng, C, rng))
            out.append(_case("uniform", ng, C, rng, tour="random"))
            out.append(_case("uniform", ng, C, rng, tour="bad"))
            out.append(_case("uniform", ng, C, rng, by_cost=False))
            out.append(_case("uniform", ng, C, rng, tour="none"))
            out.append(_case("uniform", ng, C, rng, scale=ATT))
            out.append(_case("lattice", ng, C, rng, tour="random", scale=ATT))
    res = subprocess.run([driver], input="\n".join(_text(c) for c in out) + "\n", check=True, capture_output=True, text=True, timeout=60)
    lines = res.stdout.strip().splitlines()
    assert len(lines) == len(out)
    for c, line in zip(out, lines):
        v = [int(x) for x in line.split()]
        c["got"] = (v[0], v[1:])
        c["want"] = _reference(c)
    return out


def test_table_equals_the_rule_element_for_element(cases):
    for c in cases:
        npairs = c["ng"] * (c["ng"] + 1) // 2
        assert c["got"][0] == -(-npairs // c["C"]), c["name"]
        assert c["got"] == c["want"], c["name"]


def test_every_pair_once_rows_within_ntests_padding_at_the_tail(cases):
    """Independently of the reference."""
    for c in cases:
        ntests, tab = c["got"]
        assert len(tab) == c["C"] * ntests, c["name"]
        ids = sorted(e for e in tab if e != -1)
        assert ids == sorted((r << 16) | q for r in range(c["ng"]) for q in range(r, c["ng"])), c["name"]
        for w in range(c["C"]):
            row = tab[w * ntests:(w + 1) * ntests]
            used = sum(e != -1 for e in row)
            assert used <= ntests and all(e >= 0 for e in row[:used]) and all(e == -1 for e in row[used:]), (c["name"], w)


def test_in_turn_without_a_usable_tour_or_the_flag(cases):
    """A tour with an id out of range, no tour, or the by-cost flag off: pair k of the sorted list sits in row k mod C, slot k div C."""
    seen = 0
    for c in cases:
        if c["by_cost"] and " tour=near " in c["name"] or " tour=random " in c["name"]:
            continue
        seen += 1
        pairs = sorted((_box_d2(c["gbox"][r], c["gbox"][q]), (r << 16) | q) for r in range(c["ng"]) for q in range(r, c["ng"]))
        ntests, tab = c["got"]
        for k, (_, e) in enumerate(pairs):
            assert tab[(k % c["C"]) * ntests + k // c["C"]] == e, c["name"]
    assert seen == 3 * len(NGS) * len(CS)


def test_the_cases_reach_both_classes_and_equal_costs(cases):
    """What the comparison rests on: heavy and light pairs both occur, C exceeds the number of pairs in several cases, and the
    lattice and the coincident points give many equal costs (the (load, index) tie-break decides)."""
    dealt = [c for c in cases if c["heavy"] is not None]
    assert any(c["heavy"] > 0 and c["light"] > 0 for c in dealt)
    assert any(c["light"] == 0 and c["heavy"] > c["C"] > 1 for c in dealt)
    assert sum(c["C"] > c["ng"] * (c["ng"] + 1) // 2 for c in cases) >= 10
    assert any("coincident" in c["name"] and c["heavy"] > 1 for c in dealt)
