"""The GEO truth of tests/golden/geo_truth.json (tests/geo_ref.py: mpmath from the three double cosine arguments on, with a
derived per-pair tolerance) on the host: the fixture is what its generator produces, the CPU oracle agrees with it -- which is
what makes "equal to the oracle" in tests/test_gpu_geo.py mean "equal to the truth" --, and the tolerance tells a right
implementation from a wrong one: the same formula with latitude and longitude swapped, without the + 1, with single-precision
cosines or with floor for trunc in geo_radians falls outside it."""
import os
import sys

import numpy as np
import pytest

import geo_ref as G
from helpers import GOLDEN
from oracle import oracle as O

sys.path.insert(0, GOLDEN)
import make_golden_geo as MG  # noqa: E402

FX = G.load_fixture()
NAMES = list(MG.NAMES)


def test_fixture_holds_what_the_issue_names():
    assert sorted(FX) == sorted(NAMES)
    assert os.path.getsize(os.path.join(GOLDEN, "geo_truth.json")) <= MG.MAX_BYTES
    for name in NAMES:
        f = FX[name]
        n = len(f["xy"])
        assert (f["i"] < f["j"]).all() and (f["j"] < n).all() and (f["i"] >= 0).all()
        assert len(f["undecidable"]) <= MG.UNDECIDABLE_CAP * n * (n - 1) // 2
        if name.startswith("geo_"):
            assert (f["xy"] == MG.points(name)).all()            # the committed point sets are the generator's
        i, j = MG.all_pairs(n)
        s = MG.seeded_pairs(name, n)                              # the seeded choice is among the stored pairs
        stored = set(zip(f["i"].tolist(), f["j"].tolist()))
        assert all((a, b) in stored for a, b in zip(i[s].tolist(), j[s].tolist()))
        assert np.isfinite(f["d"]).all() and (f["d"] >= 1.0).all() and (f["tol"] > 0).all()
    assert 70 <= len(FX["geo_edges"]["xy"]) <= 90 and len(FX["geo_cluster"]["xy"]) == 36


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_current(name):
    """Regenerating the stored pairs reproduces the fixture bit for bit (needs mpmath)."""
    pytest.importorskip("mpmath")
    f = FX[name]
    t = G.truth_pairs(f["xy"], f["i"], f["j"])
    assert [v[0].hex() for v in t] == [v.hex() for v in f["d"].tolist()]
    assert [v[1].hex() for v in t] == [v.hex() for v in f["tol"].tolist()]
    assert [v[2] for v in t] == f["decidable"].tolist()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_is_within_tol_and_integer_exact(name):
    f = FX[name]
    xy, i, j = f["xy"], f["i"], f["j"]
    for a, b in ((i, j), (j, i)):
        got = np.array([O.dist(xy, int(p), int(q), O.GEO, 0) for p, q in zip(a, b)])
        err = np.abs(got - f["d"])
        assert (err <= f["tol"]).all(), (name, float((err / f["tol"]).max()))
    D = O.dist_matrix(xy, O.GEO, 1)
    dec = f["decidable"]
    exp = G.true_int(f["d"])
    assert (D[i, j][dec] == exp[dec]).all() and (D[j, i][dec] == exp[dec]).all()
    assert (np.abs(D[i, j] - exp) <= 1).all()
    print("%s: oracle worst err / tol %.3g" % (name, float((err / f["tol"]).max())))


def floor_radians(v):
    v = np.asarray(v, dtype=np.float64)
    deg = np.floor(v)
    return G.PI * (deg + 5.0 * (v - deg) / 3.0) / 180.0


MUTATIONS = {"lat and lon swapped": dict(swap=True), "+ 1.0 dropped": dict(plus_one=False),
             "float32 cosines": dict(cos_dtype=np.float32), "floor for trunc in geo_radians": dict(rad=floor_radians)}


def applies(mutation, xy):
    """Does the mutation change any input of this instance?  floor differs from trunc only on a negative value with minutes."""
    if mutation == "floor for trunc in geo_radians":
        return bool(((xy < 0) & (xy != np.trunc(xy))).any())
    return True


@pytest.mark.parametrize("name", NAMES)
def test_plain_doubles_are_within_tol(name):
    """the control of the mutation test: numpy's doubles, unmutated, pass on every stored pair"""
    f = FX[name]
    err = np.abs(G.dist_double(f["xy"], f["i"], f["j"]) - f["d"])
    assert (err <= f["tol"]).all()
    dec = f["decidable"]
    assert (G.dist_double(f["xy"], f["i"], f["j"], 1)[dec] == G.true_int(f["d"])[dec]).all()
    print("%s: numpy worst err / tol %.3g" % (name, float((err / f["tol"]).max())))


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
@pytest.mark.parametrize("name", NAMES)
def test_the_bound_can_fail(name, mutation):
    """Each wrong formula is outside tol on stored pairs of every instance whose inputs it touches, and wrong
    in integer costs too (test_mutations_reach_the_integer_criterion): the tolerance is not vacuous."""
    f = FX[name]
    if not applies(mutation, f["xy"]):
        assert (G.dist_double(f["xy"], f["i"], f["j"], **MUTATIONS[mutation]) == G.dist_double(f["xy"], f["i"], f["j"])).all()
        return
    with np.errstate(invalid="ignore"):
        got = G.dist_double(f["xy"], f["i"], f["j"], **MUTATIONS[mutation])
    bad = ~(np.abs(got - f["d"]) <= f["tol"])
    print("%s, %s: %d of %d stored pairs outside tol" % (name, mutation, bad.sum(), len(bad)))
    assert bad.any()


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_mutations_reach_the_integer_criterion(mutation):
    bad = total = wrong_int = 0
    for name in NAMES:
        f = FX[name]
        with np.errstate(invalid="ignore"):
            got = G.dist_double(f["xy"], f["i"], f["j"], **MUTATIONS[mutation])
            gi = G.dist_double(f["xy"], f["i"], f["j"], 1, **MUTATIONS[mutation])
        bad += int((~(np.abs(got - f["d"]) <= f["tol"])).sum())
        wrong_int += int((gi != G.true_int(f["d"]))[f["decidable"]].sum())
        total += len(got)
    print("%s: %d of %d stored pairs outside tol, %d integer distances wrong" % (mutation, bad, total, wrong_int))
    assert wrong_int > 0                      # the integer criterion of test_gpu_geo.py sees each of them too
    if mutation == "+ 1.0 dropped":
        assert bad == total                   # every tol is far below 1


def test_coincident_points_give_exactly_one():
    f = FX["geo_edges"]
    xy = f["xy"]
    same = [(a, b) for a in range(len(xy)) for b in range(a + 1, len(xy)) if (xy[a] == xy[b]).all()]
    assert len(same) >= 4
    D = O.dist_matrix(xy, O.GEO, 1)
    stored = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(f["i"], f["j"]))}
    for a, b in same:
        assert O.dist(xy, a, b, O.GEO, 0) == 1.0 and O.dist(xy, b, a, O.GEO, 0) == 1.0
        assert D[a, b] == 1.0 and D[b, a] == 1.0
        assert f["d"][stored[(a, b)]] == 1.0      # always stored: 1 - |x| is zero
    for name in ("burma14", "geo_cluster"):
        for v in range(len(FX[name]["xy"])):
            assert O.dist(FX[name]["xy"], v, v, O.GEO, 0) == 1.0 and O.dist(FX[name]["xy"], v, v, O.GEO, 1) == 1.0
