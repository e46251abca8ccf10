"""The LDS engine's carve-up of a workgroup's dynamic LDS: csrc/lds_layout.hpp as the very source text k_lds_two_opt and
lds_bytes_needed compile, built with the host compiler (tests/lds_layout_check.cpp) and checked there for every n from 3 to 8 200
with and without the edge cache; here the printed sample against the layout written out by hand, the largest sizes that fit the
160 KiB of a gfx950 CU, and the new name of the C ABI.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsp_optimization_amd", "csrc")
N_LO, N_HI = 3, 8200
LDS_GFX950 = 160 * 1024


def up16(x):
    return (x + 15) // 16 * 16


def layout_by_hand(n, cache):
    """rows | coord | order | pos | pad | (dsp | pad) | scratch | rowsf -> (offsets in that order, total)"""
    rows, coord = 0, 48 * 32
    order = coord + 16 * n
    pos = order + 2 * n
    dsp = up16(pos + 2 * n)
    scratch = up16(dsp + 4 * n) if cache else dsp
    rowsf = scratch + 1024
    return [rows, coord, order, pos, dsp, scratch, rowsf], rowsf + 16 * 32


@pytest.fixture(scope="module")
def sources():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return [cxx, "-std=c++17", "-I", CSRC], os.path.join(ROOT, "tests", "lds_layout_check.cpp")


@pytest.fixture(scope="module")
def program(sources, tmp_path_factory):
    cmd, src = sources
    exe = str(tmp_path_factory.mktemp("lds_layout") / "lds_layout_check")
    subprocess.check_call(cmd + ["-O2", "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def results(program):
    return subprocess.run([program, str(N_LO), str(N_HI)], capture_output=True, text=True, timeout=300)


def test_regions_are_aligned_disjoint_and_inside_the_total_for_every_size(results):
    assert results.returncode == 0 and "MISMATCH" not in results.stdout, results.stdout[-2000:]
    lines = results.stdout.split("\n")[:-1]
    assert lines[-1] == "cases %d" % (2 * (N_HI - N_LO + 1))
    seen, residues = set(), set()
    for line in lines[:-1]:
        f = [int(x) for x in line.split()]
        n, cache = f[0], f[1]
        offs, total = layout_by_hand(n, cache)
        assert f[2:9] == offs and f[9] == total, line
        # every pad computed: what the two round-ups add is 0 .. 15 bytes each, and the old "+ 16 once, with the cache" is not it
        assert 0 <= total - (3072 + 20 * n + (4 * n if cache else 0)) <= (30 if cache else 15), line
        seen.add((n, cache))
        residues.add(n % 4)
    assert {(N_LO, 0), (N_LO, 1), (N_HI, 0), (N_HI, 1), (2500, 1), (8000, 0)} <= seen and residues == {0, 3}


def test_the_pads_by_hand_for_every_residue_mod_4():
    """pos ends at 1536 + 20 n: 4 (n mod 4) bytes past a multiple of 16; with the cache dsp ends 4 (n mod 4) past one again"""
    for n in range(3, 8201):
        r = n % 4
        pad = (16 - 4 * r) % 16
        assert layout_by_hand(n, 0)[1] == 3072 + 20 * n + pad
        assert layout_by_hand(n, 1)[1] == 3072 + 24 * n + 2 * pad
    # the float rows of the fp32 tier end exactly at the total: nothing behind the size a launch asks for
    offs, total = layout_by_hand(2501, 1)
    assert offs[6] + 512 == total == 63120 and 3088 + 24 * 2501 == 63112


def test_the_largest_sizes_that_fit_160_kib_are_8038_and_6698(program):
    res = subprocess.run([program, "max", str(LDS_GFX950)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout == "max 8038 6698\n", res.stdout
    assert layout_by_hand(8038, 0)[1] == LDS_GFX950 == layout_by_hand(6698, 1)[1]        # both fill the CU's LDS to the byte
    assert layout_by_hand(8039, 0)[1] > LDS_GFX950 and layout_by_hand(6699, 1)[1] > LDS_GFX950
    res = subprocess.run([program, "max", str(64 * 1024)], capture_output=True, text=True, timeout=60)
    want = tuple(max(n for n in range(3, 4000) if layout_by_hand(n, c)[1] <= 64 * 1024) for c in (0, 1))
    assert res.returncode == 0 and res.stdout == "max %d %d\n" % want, res.stdout


def test_the_header_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(sources, results, tmp_path):
    """A program of its own, built with the sanitizers and run once on every size: the same answers, no report."""
    cmd, src = sources
    exe = str(tmp_path / "lds_layout_check_san")
    subprocess.check_call(cmd + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    res = subprocess.run([exe, str(N_LO), str(N_HI)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    assert res.stdout == results.stdout


def test_host_and_kernel_take_the_layout_from_the_header():
    """one carve-up: the kernel's pointers and the launch's size both come from lds_layout(); no arithmetic of their own is left"""
    src = open(os.path.join(CSRC, "two_opt_lds.hip")).read()
    assert '#include "lds_layout.hpp"' in src
    assert re.search(r"lds_bytes_needed\(int n, bool edge_cache = false\) \{ return lds_layout\(n, edge_cache\)\.total; \}", src)
    assert "const LdsLayout lay = lds_layout(n, CACHE);" in src
    for name in ("rows", "coord", "order", "pos", "dsp", "scratch", "rowsf"):
        assert "smem + lay.%s" % name in src, name
    assert "& 15" not in src                                # the pads the kernel used to compute from its pointers
    # one predicate for the choice of the body: launch_lds and the entry point both call lds_variant()
    assert src.count("LDS_F32_MIN_N") == 2 and src.count("LDS_EDGE_CACHE") == 2       # each once in code, once in the comment above it
    assert len(re.findall(r"= lds_variant\((?:t->)?inst\)", src)) == 2
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "lds_layout.hpp" in mk


def test_the_entry_point_is_exported_and_bound():
    from tsp_optimization_amd import engine as E
    assert "tsp_dev_inst_lds_variant" in E.EXPORTED and hasattr(E.lib(), "tsp_dev_inst_lds_variant")
    assert hasattr(E.Instance, "lds_variant")
    hip = open(os.path.join(ROOT, "include", "tsp_hip.h")).read()
    assert re.search(r"int tsp_dev_tours_describe\(tsp_dev_tours \*t, int mode, char \*buf, int cap\);\n/\*.*?\*/\n"
                     r"int tsp_dev_inst_lds_variant\(tsp_dev_inst \*inst, int mode, char \*buf, int cap\);", hip, re.S)
    assert E.lib().tsp_dev_inst_lds_variant(None, E.FIRST, None, 0) == E.E_ARG
