"""The GEO distance (dist_xy<WT_GEO, INT> of csrc/tsp_dist.hpp, src/distutil.c:51-71) restated for a high-precision "truth",
with a per-pair error bound for any implementation that evaluates the same formula in IEEE double.  Host only.

What is reproducible to the bit, and so formed here in IEEE double exactly as the kernel and the oracle form it:
    geo_radians(v) = PI * (trunc(v) + 5 * (v - trunc(v)) / 3) / 180          (degrees.minutes -> radians)
    a1 = lon_i - lon_j,   a2 = lat_i - lat_j,   a3 = lat_i + lat_j             (dist_xy takes (lat, lon): q1 is the LONGITUDE term)
These three doubles are the inputs of the kernel's cosines.  Everything after them is evaluated with mpmath at 50 digits:
    q_k = cos(a_k),   x = ((1 + q1) q2 - (1 - q1) q3) / 2  clipped to [-1, 1],   d = R acos(x) + 1,   R = 6378.388 (the double).

The tolerance, derived and not tuned.  u = 2^-53.
  * ROCm's installed documentation states no ULP bound for ocml's fp64 cos and acos, so the OpenCL full-profile bound of 4 ulp is
    taken for both (OpenCL C specification, "Relative error as ULPs"); glibc's are below 1 ulp.
  * |q_k| <= 1, and the spacing of doubles up to 1 is at most u, so 4 ulp of a cosine is at most 4u absolute.
  * dx/dq1 = (q2 + q3) / 2, dx/dq2 = (1 + q1) / 2, dx/dq3 = -(1 - q1) / 2: each at most 1 in magnitude, so the three cosines move
    x by at most 12u.
  * The five roundings of the expression (1 + q1, 1 - q1, two products, the difference; the halving is exact) are each at most
    u relative on a value of magnitude at most 2 and reach x with a factor of 1/2: under 6u together.
  * E = 20u bounds |x_computed - x| with room to spare.
  * acos is ill-conditioned at x = +-1 (coincident and antipodal points), so the bound is not linearised:
        w   = R * max(acos(x - E) - acos(x), acos(x) - acos(x + E)),   arguments clipped to [-1, 1]
        tol = w + 8u * d            (acos's own 4 ulp, the product with R, the sum with 1, and the rounding of d_true to double)
A pair is DECIDABLE for integer costs when d is farther than tol from every k + 1/2; its integer distance is then
floor(d + 1/2) for every implementation within the bound.  mpmath is needed only by truth(); the fixture
tests/golden/geo_truth.json carries its results to where mpmath is not installed."""
import math
import os

import numpy as np

PI = 3.14159265358979323846264      # include/distutil.h:6-7, as the compiler rounds them
RADIUS = 6378.388
U = 2.0 ** -53
E_X = 20 * U
DIGITS = 50

HERE = os.path.dirname(os.path.abspath(__file__))
TSPLIB_GEO = ("burma14", "ulysses22", "gr431", "ali535", "gr666")


def geo_radians(v):
    v = np.asarray(v, dtype=np.float64)
    deg = np.trunc(v)
    frac = v - deg
    return PI * (deg + 5.0 * frac / 3.0) / 180.0


def cos_args(xy, i, j):
    """-> (lon_i - lon_j, lat_i - lat_j, lat_i + lat_j) in IEEE double, for index arrays i, j"""
    xy = np.asarray(xy, dtype=np.float64)
    lat, lon = geo_radians(xy[:, 0]), geo_radians(xy[:, 1])
    return lon[i] - lon[j], lat[i] - lat[j], lat[i] + lat[j]


def dist_double(xy, i, j, integer_cost=0, swap=False, plus_one=True, cos_dtype=np.float64, rad=geo_radians):
    """The formula in numpy doubles, with the mutations of tests/test_cpu_geo_ref.py as switches.  Not the reference: a
    double-precision implementation like the oracle's and the kernel's, here to show that `tol` tells right from wrong."""
    xy = np.asarray(xy, dtype=np.float64)
    lat, lon = rad(xy[:, 1 if swap else 0]), rad(xy[:, 0 if swap else 1])

    def cos(a):
        return np.cos(a.astype(cos_dtype)).astype(np.float64)
    q1, q2, q3 = cos(lon[i] - lon[j]), cos(lat[i] - lat[j]), cos(lat[i] + lat[j])
    d = RADIUS * np.arccos(0.5 * ((1.0 + q1) * q2 - (1.0 - q1) * q3)) + (1.0 if plus_one else 0.0)
    return np.trunc(d + 0.5) if integer_cost else d


def truth(a1, a2, a3):
    """One pair, from the three double arguments -> (d_true as mpf, tol as mpf, 1 - |x| as mpf, decidable)"""
    import mpmath as mp
    mp.mp.dps = DIGITS
    q1, q2, q3 = (mp.cos(mp.mpf(float(a))) for a in (a1, a2, a3))
    x = ((1 + q1) * q2 - (1 - q1) * q3) / 2
    x = min(mp.mpf(1), max(mp.mpf(-1), x))
    R, E = mp.mpf(RADIUS), mp.mpf(E_X)
    ac = mp.acos(x)
    d = R * ac + 1
    lo, hi = max(mp.mpf(-1), x - E), min(mp.mpf(1), x + E)
    w = R * max(mp.acos(lo) - ac, ac - mp.acos(hi))
    tol = w + 8 * mp.mpf(U) * d
    off = abs(d - mp.floor(d) - mp.mpf(0.5))          # distance to the nearest k + 1/2
    return d, tol, 1 - abs(x), bool(off > tol), off


def truth_pairs(xy, i, j):
    """-> list of (d_true double, tol double rounded up, decidable) for index arrays i, j"""
    a1, a2, a3 = cos_args(xy, np.asarray(i), np.asarray(j))
    out = []
    for k in range(len(a1)):
        d, tol, _, dec, _ = truth(a1[k], a2[k], a3[k])
        out.append((float(d), math.nextafter(float(tol), math.inf), dec))
    return out


def true_int(d_true):
    """The integer distance of a decidable pair: floor(d + 1/2)"""
    return np.floor(np.asarray(d_true, dtype=np.float64) + 0.5)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def load_fixture():
    """tests/golden/geo_truth.json -> {name: {"xy", "i", "j", "d", "tol", "decidable", "undecidable"}} with numpy arrays"""
    import json
    from helpers import load_instance
    with open(os.path.join(HERE, "golden", "geo_truth.json")) as f:
        raw = json.load(f)
    out = {}
    for name, r in raw["instances"].items():
        xy = np.array(r["xy"], dtype=np.float64) if "xy" in r else load_instance(name)[0]
        assert len(xy) == r["n"]
        p = r["pairs"]
        und = np.array(r["undecidable"], dtype=np.int64).reshape(-1, 2)
        i, j = np.array([q[0] for q in p]), np.array([q[1] for q in p])
        und_set = {(int(a), int(b)) for a, b in und}
        out[name] = {"xy": xy, "i": i, "j": j,
                     "d": np.array([float.fromhex(q[2]) for q in p]), "tol": np.array([float.fromhex(q[3]) for q in p]),
                     "decidable": np.array([(int(a), int(b)) not in und_set for a, b in zip(i, j)]),
                     "undecidable": und}
    return out
