"""CPU: the dealing of the exhaustive sweep's row units to the waves of k_exh (csrc/exh_arith.hpp: exh_deal), as the very source
text tsp_dev_tours_create fills the kernel's table of descriptors with, compiled with the host compiler
(tests/exh_deal_check.cpp) and compared with a restatement of the rule k_exh used to evaluate itself, per wave, at every launch:

  * strips = ceil(n / weff) strips of pair-columns, strip s with q0 = s weff - (strips weff - n) and min(q0 + weff - 1, n - 1)
    row units; total = their sum; the units of all strips laid end to end, strip 0 first;
  * equal shares: per = ceil(total / waves), wave gw owns the units [per gw, per gw + per);
  * shares (share[0] > 0 and gens > 0): wq = waves div gens, part g = min(gens - 1, gw div wq), idx = gw - g wq, the wave owns
    share[g] units from sum(share[q] wq, q < g) + share[g] idx;
  * both ends clamped to total; the wave then visits, strip after strip, the rows [pa, pb) of every strip its range meets.

A descriptor says (strip, row, count); the kernel's walk from it -- `count` units from row `row` of strip `strip`, on into the
following strips from their row 0 -- must visit the same (strip, pa, pb), segment for segment."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsp_optimization_amd", "csrc")

WEFF = 64 * 4 - 1   # k_exh: W - 1 with W = 64 lanes x kExhRJ columns
NS = (5, 8, 254, 255, 256, 257, 509, 510, 511, 766, 1000, 10000, 20011, 40009)
WAVES = (4, 16, 1024, 4096, 8192)
SHARES = (("equal", None, 0), ("48/29/15/8", (48, 29, 15, 8), 4), ("50/30/20", (50, 30, 20, 0), 3), ("60/40", (60, 40, 0, 0), 2))


def _strips(n, weff):
    ns = (n + weff - 1) // weff
    out = []
    for s in range(ns):
        q0 = s * weff - (ns * weff - n)
        out.append((max(q0, 0), min(q0 + weff - 1, n - 1)))
    return out


def _host_shares(total, waves, pc, gens):
    """tsp_dev_tours_create's figures: rows per wave of each part of the grid, from per-cent figures."""
    if pc is None:
        return (0, 0, 0, 0)
    wq, tot = waves // gens, sum(pc)
    return tuple(max(1, -(-(total * c) // (tot * wq))) if q < gens else 0 for q, c in enumerate(pc))


def _range_of(gw, total, waves, share, gens):
    """[u_lo, u_hi) of wave gw: the arithmetic at the head of the kernel, before the change."""
    per = (total + waves - 1) // waves
    u_lo = per * gw
    if share[0] > 0 and gens > 0:
        wq = waves // gens
        g = min(gens - 1, gw // wq)
        idx = gw - g * wq
        u_lo = sum(share[q] * wq for q in range(g))
        per = share[g]
        u_lo += per * idx
    u_hi = min(total, u_lo + per)
    return min(u_lo, total), u_hi


def _parent_segments(gw, rows, total, waves, share, gens):
    """The loop of the kernel before the change, literally: the segments (strip, pa, pb) wave gw visits."""
    u_lo, u_hi = _range_of(gw, total, waves, share, gens)
    seg, cum, s = [], 0, 0
    while s < len(rows) and u_lo < u_hi:
        rows_s = rows[s]
        if u_lo >= cum + rows_s:
            cum += rows_s
            s += 1
            continue
        pa, pb = u_lo - cum, min(rows_s, u_hi - cum)
        u_lo = cum + pb
        cum += rows_s
        seg.append((s, pa, pb))
        s += 1
    return seg


def _walk(desc, rows):
    """The kernel's walk from a descriptor."""
    strip, row, count = desc
    seg, s, pa, rem = [], strip, row, count
    while rem > 0 and s < len(rows):
        pb = min(rows[s], pa + rem)
        rem -= pb - pa
        seg.append((s, pa, pb))
        pa = 0
        s += 1
    return seg


@pytest.fixture(scope="module")
def sources():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # plain C++17, nothing of HIP: exh_arith.hpp as the kernel and the host include it; -ffp-contract=off as in csrc/Makefile
    return [cxx, "-std=c++17", "-ffp-contract=off", "-I", CSRC], os.path.join(ROOT, "tests", "exh_deal_check.cpp")


@pytest.fixture(scope="module")
def case_list():
    out = []
    for n in NS:
        rows = [r for _, r in _strips(n, WEFF)]
        total = sum(rows)
        for waves in WAVES:
            for name, pc, gens in SHARES:
                out.append(dict(n=n, waves=waves, gens=gens, share=_host_shares(total, waves, pc, gens),
                                name="n=%d waves=%d shares=%s" % (n, waves, name)))
    return out


def _text(cases):
    return "".join("%d %d %d %d %d %d %d %d\n" % ((c["n"], WEFF, c["waves"]) + c["share"] + (c["gens"],)) for c in cases)


def _parse(cases, stdout):
    lines = stdout.strip().splitlines()
    assert len(lines) == len(cases)
    for c, line in zip(cases, lines):
        v = np.array(line.split(), dtype=np.int64)
        ns = int(v[0])
        c["strips"], c["total"] = ns, int(v[1])
        c["geom"] = v[2:2 + 2 * ns].reshape(ns, 2)
        c["desc"] = v[2 + 2 * ns:].reshape(c["waves"], 3)


@pytest.fixture(scope="module")
def cases(sources, case_list, tmp_path_factory):
    """Every case with the driver's descriptors: one run of the driver for all of them."""
    cmd, src = sources
    exe = str(tmp_path_factory.mktemp("exh_deal") / "exh_deal_check")
    subprocess.check_call(cmd + ["-O2", "-o", exe, src])
    res = subprocess.run([exe], input=_text(case_list), check=True, capture_output=True, text=True, timeout=120)
    case_list[0]["stdout"] = res.stdout
    _parse(case_list, res.stdout)
    return case_list


def test_strips_are_the_closed_form(cases):
    for c in cases:
        want = _strips(c["n"], WEFF)
        assert c["strips"] == len(want) and c["total"] == sum(r for _, r in want), c["name"]
        assert [tuple(int(x) for x in g) for g in c["geom"]] == want, c["name"]


def test_every_row_unit_is_owned_by_exactly_one_wave_in_contiguous_ranges_in_wave_order(cases):
    for c in cases:
        rows = c["geom"][:, 1]
        start_of = np.concatenate(([0], np.cumsum(rows)))
        strip, row, count = c["desc"][:, 0], c["desc"][:, 1], c["desc"][:, 2]
        live = count > 0
        assert (count >= 0).all() and (strip[~live] == 0).all() and (row[~live] == 0).all(), c["name"]
        assert ((strip[live] >= 0) & (strip[live] < c["strips"])).all(), c["name"]
        assert ((row[live] >= 0) & (row[live] < rows[strip[live]])).all(), c["name"]   # a start inside a strip that has rows
        lo = start_of[strip[live]] + row[live]
        hi = lo + count[live]
        # the waves that have units: the first starts at unit 0, each next one where the one before ended, the last ends at total
        assert lo[0] == 0 and hi[-1] == c["total"] and (lo[1:] == hi[:-1]).all(), c["name"]


def test_segment_for_segment_what_the_loop_in_the_kernel_visited(cases):
    """All waves of a case at once, strip by strip: at strip s (units [cum, cum + rows)) the old loop visits
    [max(u_lo, cum) - cum, min(u_hi, cum + rows) - cum) when that is not empty; the walk from the descriptor visits
    [row if s == strip else 0, min(rows, pa + rem)) while rem > 0."""
    for c in cases:
        rows = c["geom"][:, 1]
        waves, share, gens, total = c["waves"], c["share"], c["gens"], c["total"]
        rng = np.array([_range_of(gw, total, waves, share, gens) for gw in range(waves)], dtype=np.int64)
        u_lo, u_hi = rng[:, 0], rng[:, 1]
        strip, row, rem = c["desc"][:, 0], c["desc"][:, 1], c["desc"][:, 2].copy()
        cum = 0
        for s in range(c["strips"]):
            r = int(rows[s])
            pa_old, pb_old = np.maximum(u_lo, cum) - cum, np.minimum(u_hi, cum + r) - cum
            on_old = pa_old < pb_old
            on_new = (s >= strip) & (rem > 0)
            pa_new = np.where(s == strip, row, 0)
            pb_new = np.minimum(r, pa_new + rem)
            assert (on_old == on_new).all(), (c["name"], s)
            assert (pa_old[on_old] == pa_new[on_old]).all() and (pb_old[on_old] == pb_new[on_old]).all(), (c["name"], s)
            rem = np.where(on_new, rem - (pb_new - pa_new), rem)
            cum += r
        assert (rem == 0).all(), c["name"]


def test_the_literal_loops_agree_wave_by_wave(cases):
    """The same comparison with both loops written out per wave (every wave of the small grids, 64 waves of the large ones)."""
    for c in cases:
        rows = [int(r) for r in c["geom"][:, 1]]
        waves = c["waves"]
        pick = range(waves) if waves <= 16 else sorted(set(range(0, waves, waves // 61)) | {1, waves // 4 - 1, waves // 4, waves - 1})
        for gw in pick:
            want = _parent_segments(gw, rows, c["total"], waves, c["share"], c["gens"])
            got = _walk(tuple(int(x) for x in c["desc"][gw]), rows)
            assert got == want, (c["name"], gw)
            assert all(pa < pb for _, pa, pb in got), (c["name"], gw)


def test_the_cases_reach_empty_waves_many_strips_per_wave_and_a_strip_without_rows(cases):
    by = {c["name"]: c for c in cases}
    spans = lambda c: [len(_walk(tuple(int(x) for x in d), [int(r) for r in c["geom"][:, 1]])) for d in c["desc"]]
    assert max(spans(by["n=40009 waves=1024 shares=equal"])) >= 3   # a wave over three strips and more
    assert max(spans(by["n=40009 waves=1024 shares=48/29/15/8"])) >= 3
    assert any((c["desc"][:, 2] == 0).any() and (c["desc"][:, 2] > 0).any() for c in cases if c["n"] >= 10000)   # waves without units
    assert (by["n=5 waves=8192 shares=equal"]["desc"][:, 2] > 0).sum() <= 4    # nearly every wave empty
    assert int(by["n=256 waves=4 shares=equal"]["geom"][0, 1]) == 0            # strip 0 has no rows: passed over
    assert by["n=255 waves=4 shares=equal"]["strips"] == 1 and by["n=256 waves=4 shares=equal"]["strips"] == 2
    assert tuple(by["n=257 waves=4 shares=equal"]["geom"][0]) == (0, 1)         # strip 0 clamped to column 0, over strip 1
    parts = {c["gens"] for c in cases}
    assert parts == {0, 2, 3, 4}


def test_the_driver_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(sources, cases, tmp_path):
    """A program of its own, built with the sanitizers and run once on every case: the same answers, no report."""
    cmd, src = sources
    exe = str(tmp_path / "exh_deal_check_san")
    subprocess.check_call(cmd + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    res = subprocess.run([exe], input=_text(cases), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    assert res.stdout == cases[0]["stdout"]
