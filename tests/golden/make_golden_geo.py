"""Records tests/golden/geo_truth.json: the GEO distance of tests/geo_ref.py (the kernel's formula from its three double cosine
arguments on, evaluated by mpmath at 50 digits) with the derived per-pair tolerance, for tests/test_cpu_geo_ref.py (which
checks the oracle against it, and regenerates the stored pairs where mpmath is installed) and tests/test_gpu_geo.py (which
checks the device against it without mpmath).  Nothing here comes from the reference: the numbers are mpmath's.

Per instance -- burma14, ulysses22, gr431, ali535, gr666 by name, and the two point sets geo_edges and geo_cluster, whose
coordinates are stored -- the file holds
  pairs        [i, j, d_true, tol] with the two doubles as float.hex(): every pair of the three small sets, a seeded choice of
               400 from each of the others, and always the 16 pairs with the smallest 1 - |x| and the 16 nearest to a k + 1/2;
  undecidable  every pair i < j of ALL the instance's pairs whose d_true is within tol of a k + 1/2 (geo_ref's docstring).
The generator fails if an undecidable list is longer than 1e-4 of the instance's pairs: a test may not hide more than that.
All pairs of the seven instances are about two minutes of mpmath, spread over a pool of processes.  Run from the repository root:
python tests/golden/make_golden_geo.py"""
import json
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import geo_ref as G  # noqa: E402

SEED = 20260
SAMPLED = 400                    # seeded pairs of an instance that is not taken whole
EXTREMES = 16                    # of each kind
WHOLE = ("burma14", "ulysses22", "geo_cluster")
NAMES = G.TSPLIB_GEO + ("geo_edges", "geo_cluster")
UNDECIDABLE_CAP = 1e-4
MAX_BYTES = 238683               # the largest fixture of tests/golden/ before this one (nl_descents.json)


def geo_points(n):
    """the random degrees.minutes points of tests/test_gpu_construct_paths.py"""
    rng = np.random.default_rng(4242 + n)
    deg = rng.integers(-60, 61, size=(n, 2))
    minutes = rng.integers(0, 60, size=(n, 2))
    return deg + np.sign(deg + 0.5) * minutes / 100.0


def edges_points():
    """(lat, lon) in TSPLIB's degrees.minutes: where the conversion or the formula could go wrong"""
    p = [(90.00, 0.00), (-90.00, 0.00), (90.00, 123.30), (-90.00, -45.15),                     # both poles, twice each
         (0.00, 0.00), (0.00, 180.00), (0.00, -180.00), (0.00, 179.59), (0.00, -179.59),         # equator, 0 / +-180 / +-179.59
         (45.30, 180.00), (45.30, -180.00), (45.30, 179.59), (45.30, -179.59), (45.30, 0.00),
         (-45.30, 180.00), (-45.30, -180.00), (-45.30, 179.59), (-45.30, -179.59), (-45.30, 0.00),
         (0.00, 10.00), (0.00, -10.00), (0.00, 90.00), (0.00, -90.00),                           # the equator
         (0.00, 10.00), (45.30, 179.59), (-90.00, 0.00), (-10.30, -20.30),                       # coincident with others
         (10.30, 20.30), (10.31, 20.30), (10.29, 20.30), (10.30, 20.31), (10.30, 20.29),         # one minute apart, each way
         (-10.30, -20.30), (-10.31, -20.30), (-10.29, -20.30), (-10.30, -20.31), (-10.30, -20.29),
         (-0.30, 5.00), (5.00, -0.30), (-0.30, -0.30), (0.30, 0.30), (-0.01, -0.01), (0.01, 0.01),  # the degree part truncates to -0
         (89.59, 0.00), (-89.59, 100.00), (89.59, -179.59), (-89.59, 179.59),                    # a minute from the poles
         (-10.59, 30.00), (-11.00, 30.00), (-10.01, 30.00), (-10.00, 30.00), (-9.59, 30.00),     # minutes on both sides of negative degrees
         (30.00, -10.59), (30.00, -11.00), (30.00, -10.01), (30.00, -10.00), (30.00, -9.59),
         (30.00, 40.00), (-30.00, -140.00), (-30.00, -139.59), (60.15, -120.45), (-60.15, 59.15)]   # antipodes
    return np.concatenate([np.array(p, dtype=np.float64), geo_points(24)])


def cluster_points():
    """6 x 6 points one minute apart, across a degree boundary on both axes (and a negative one in longitude)"""
    lat = [47.57, 47.58, 47.59, 48.00, 48.01, 48.02]
    lon = [-122.02, -122.01, -122.00, -121.59, -121.58, -121.57]
    return np.array([(a, b) for a in lat for b in lon], dtype=np.float64)


def points(name):
    if name == "geo_edges":
        return edges_points()
    if name == "geo_cluster":
        return cluster_points()
    from helpers import load_instance
    xy, wt = load_instance(name)
    assert wt == 4, name
    return xy


def all_pairs(n):
    i, j = np.triu_indices(n, 1)
    return i.astype(np.int64), j.astype(np.int64)


def seeded_pairs(name, n):
    """the pairs chosen without looking at the distances -> indices into all_pairs(n)"""
    m = n * (n - 1) // 2
    if name in WHOLE:
        return np.arange(m)
    rng = np.random.default_rng(SEED + NAMES.index(name))
    return np.sort(rng.choice(m, size=SAMPLED, replace=False))


def scan_chunk(a):
    """every pair of a chunk -> per pair (undecidable, 1 - |x|, distance to the nearest half-integer), as doubles"""
    und, edge, off = [], [], []
    for k in range(len(a[0])):
        _, _, e, dec, o = G.truth(a[0][k], a[1][k], a[2][k])
        und.append(not dec)
        edge.append(float(e))
        off.append(float(o))
    return und, edge, off


def main():
    out = {}
    with mp.Pool(min(16, os.cpu_count() or 1)) as pool:
        for name in NAMES:
            xy = points(name)
            n = len(xy)
            i, j = all_pairs(n)
            a1, a2, a3 = G.cos_args(xy, i, j)
            cuts = np.array_split(np.arange(len(i)), max(1, len(i) // 2000))
            res = pool.map(scan_chunk, [(a1[c], a2[c], a3[c]) for c in cuts], chunksize=1)
            und = np.concatenate([r[0] for r in res]).astype(bool)
            edge = np.concatenate([r[1] for r in res])
            off = np.concatenate([r[2] for r in res])
            if und.sum() > UNDECIDABLE_CAP * len(i):
                raise SystemExit("%s: %d of %d pairs undecidable, over the cap" % (name, und.sum(), len(i)))
            sel = np.union1d(seeded_pairs(name, n), np.union1d(np.argsort(edge, kind="stable")[:EXTREMES],
                                                               np.argsort(off, kind="stable")[:EXTREMES]))
            t = G.truth_pairs(xy, i[sel], j[sel])
            rec = {"n": n, "pairs": [[int(i[s]), int(j[s]), d.hex(), tol.hex()] for s, (d, tol, _) in zip(sel, t)],
                   "undecidable": [[int(i[k]), int(j[k])] for k in np.flatnonzero(und)]}
            if name.startswith("geo_"):
                rec["xy"] = [[float(v[0]), float(v[1])] for v in xy]
            out[name] = rec
            print("%-11s n %3d  pairs %6d  stored %4d  undecidable %d  smallest 1-|x| %.3g  nearest half-integer %.3g  largest tol %.3g"
                  % (name, n, len(i), len(sel), und.sum(), edge.min(), off.min(), max(v[1] for v in t)))
    path = os.path.join(HERE, "geo_truth.json")
    with open(path, "w") as f:
        json.dump({"_source": "make_golden_geo.py: mpmath %d digits, E = 20u, tol = w + 8u d (tests/geo_ref.py); not taken from the reference"
                   % G.DIGITS, "instances": out}, f, separators=(",", ":"), sort_keys=True)
    size = os.path.getsize(path)
    print("geo_truth.json: %d bytes" % size)
    if size > MAX_BYTES:
        raise SystemExit("geo_truth.json is larger than the largest fixture before it (%d bytes)" % MAX_BYTES)


if __name__ == "__main__":
    main()
