"""csrc/gnc.h as a program of its own, tests/native/gnc_main.cpp, built by g++ under ASan + UBSan: the run is clean and its
output is bitwise what the library's host entry point, pgo_gnc_weight_eval, returns (the same statement), over a grid of
(cbar, mu, s) that sits on both thresholds, one ulp to either side of each, at s = 0, inf and NaN, for mu from 1e-9 to 1e9.
The properties of the weight -- its range, its monotonicity in s, its continuity at the thresholds -- are checked in numpy on
the same grid."""
import os

import numpy as np
import pytest

import _gnc_restatement as GR
import _native_san as NS

EPS = np.finfo(np.float64).eps
CBARS = (0.5, 1.0, 0.03, 7.25)
MUS = np.concatenate([10.0 ** np.arange(-9, 10), [1.4e-4, 0.37, 2.6, 977.0]])


def thresholds(cbar, mu):
    c2 = cbar * cbar
    return mu / (mu + 1.0) * c2, (mu + 1.0) / mu * c2   # (gnc.h's order of operations)


def grid():
    rows = []
    for cbar in CBARS:
        for mu in MUS:
            lo, hi = thresholds(cbar, mu)
            s = [0.0, np.inf, np.nan, -np.inf, lo, hi, np.nextafter(lo, 0.0), np.nextafter(lo, np.inf), np.nextafter(hi, 0.0),
                 np.nextafter(hi, np.inf), 0.5 * lo, 2.0 * hi, np.finfo(np.float64).tiny, 1e300]
            s += list(np.geomspace(lo, hi, 17)[1:-1])
            rows += [(cbar, mu, v) for v in s]
    return np.array(rows)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("gnc_native"), "gnc_main")


def test_sanitized_program_is_bitwise_the_library(pgo, exe, tmp_path):
    G = grid()
    src, dst = os.path.join(str(tmp_path), "in.txt"), os.path.join(str(tmp_path), "out.txt")
    with open(src, "w") as f:
        f.write("%d\n" % len(G))
        for cbar, mu, s in G:
            f.write("%.17g %.17g %.17g\n" % (cbar, mu, s))
    assert "gnc ok: %d weights" % len(G) in NS.run([exe, src, dst])
    got = np.array([[float(v) for v in line.split()] for line in open(dst).read().split("\n") if line])
    assert got.shape == (len(G), 2)
    for cbar in CBARS:
        for mu in MUS:
            m = (G[:, 0] == cbar) & (G[:, 1] == mu)
            ref = pgo.gnc_weight_eval(cbar, mu, G[m, 2])
            assert got[m, 0].tobytes() == ref.tobytes(), (cbar, mu)
            # ... and the numpy restatement the GPU tests lean on says the same
            assert GR.tls_weight(cbar * cbar, mu, G[m, 2]).tobytes() == ref.tobytes(), (cbar, mu)
    # gnc_mu0 where it is defined (2 rmax2 > c2), against the same three operations in numpy
    c2, r2 = G[:, 0] ** 2, G[:, 2]
    ok = np.isfinite(r2) & (2.0 * r2 > c2)
    assert ok.sum() > 100 and got[ok, 1].tobytes() == (c2[ok] / (2.0 * r2[ok] - c2[ok])).tobytes()
    assert np.all(got[ok, 1] > 0.0)


def test_weight_properties(pgo):
    """w in [0, 1]; non-increasing in s; exactly 1 / 0 at and beyond the thresholds; continuous there.

    Continuity bound: between the thresholds w = sqrt(c2 mu (mu + 1) / s) - mu has the slope -(mu + 1) / (2 s) at the lower and
    -mu / (2 s) at the upper threshold, so over ONE ulp of s the exact function itself moves by up to (mu + 1) eps / 2, and the
    three roundings under the square root and the subtraction add less than 3 (mu + 1) eps: |w(one ulp inside) - w(threshold)|
    <= 4 (mu + 1) eps.  That is below the 1e-12 asked for up to mu = 1e3, where 1e-12 is asserted as it stands; for larger mu
    (ulp(mu) alone is 1.2e-7 at 1e9) the bound is 4 (mu + 1) eps."""
    for cbar in CBARS:
        for mu in MUS:
            lo, hi = thresholds(cbar, mu)
            s = np.sort(np.concatenate([[0.0, lo, hi, np.nextafter(lo, 0.0), np.nextafter(lo, np.inf), np.nextafter(hi, 0.0),
                                         np.nextafter(hi, np.inf), 1e300, np.inf], np.geomspace(lo, hi, 401), np.geomspace(1e-3 * lo, 1e3 * hi, 101)]))
            w = pgo.gnc_weight_eval(cbar, mu, s)
            what = (cbar, mu)
            fin = np.isfinite(s)
            assert np.all((w >= 0.0) & (w <= 1.0)), what
            assert np.all(np.diff(w[fin]) <= 0.0), what
            assert np.all(w[s <= lo] == 1.0) and np.all(w[s >= hi] == 0.0), what
            bound = 1e-12 if mu <= 1e3 else 4.0 * (mu + 1.0) * EPS
            assert 4.0 * (min(mu, 1e3) + 1.0) * EPS <= 1e-12
            w_in = pgo.gnc_weight_eval(cbar, mu, np.array([np.nextafter(lo, np.inf), np.nextafter(hi, 0.0)]))
            assert abs(w_in[0] - 1.0) <= bound and abs(w_in[1] - 0.0) <= bound, (what, w_in)
    assert np.array_equal(pgo.gnc_weight_eval(0.5, 0.1, np.array([np.nan, np.inf, -np.inf])), np.zeros(3))
    for bad in ((0.0, 1.0), (-1.0, 1.0), (np.inf, 1.0), (np.nan, 1.0), (0.5, 0.0), (0.5, -1.0), (0.5, np.nan), (0.5, np.inf)):
        with pytest.raises(pgo.PgoError) as ei:
            pgo.gnc_weight_eval(bad[0], bad[1], np.ones(2))
        assert ei.value.status == -1
