"""csrc/prior.h as a program of its own, tests/native/prior_main.cpp, built by g++ under ASan + UBSan: the run is clean, the
heading wraps by the IEEE remainder, position-only informations are accepted and indefinite ones refused, and the values are
those of the numpy closed form (tests/_prior_restatement.py) and of the library's host entry point pgo_prior_eval, for every
loss type on both sides of its bend."""
import math
import os

import numpy as np
import pytest

import _loss_restatement as LR
import _native_san as NS
import _prior_restatement as PR

EPS = np.finfo(np.float64).eps
# (loss, scale): with the informations below chi2 falls on both sides of a^2 (Huber, Tukey) and of the knee of the others
LOSSES = [("trivial", 0.0), ("huber", 0.5), ("softlone", 0.5), ("cauchy", 0.5), ("arctan", 0.5), ("tukey", 0.5)]
WRAPS = [math.pi, -math.pi, math.pi + 1e-9, -(math.pi + 1e-9), 6.2, -6.2]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("prior_native"), "prior_main")


def _run(exe, tmp_path, cases):
    src, dst = os.path.join(str(tmp_path), "in.txt"), os.path.join(str(tmp_path), "out.txt")
    with open(src, "w") as f:
        f.write("%d\n" % len(cases))
        for p, z, w, loss in cases:
            f.write(" ".join("%.17g" % v for v in (*p, *z, *w)) + " %d %.17g\n" % (LR.TYPES[loss[0]], loss[1]))
    assert "prior ok: %d cases" % len(cases) in NS.run([exe, src, dst])
    out = np.loadtxt(dst, ndmin=2)
    assert out.shape == (len(cases), 8)
    return out


def _value_cases():
    rng = np.random.default_rng(5)
    cases = []
    for loss in LOSSES:
        for scale in (1e-3, 0.05, 0.3, 2.0, 40.0):   # chi2 from ~1e-6 a^2 to ~1e4 a^2
            B = rng.normal(size=(3, 3))
            for M in (B @ B.T + 0.1 * np.eye(3), np.diag([3.0, 3.0, 0.0]), np.outer(B[0], B[0]), np.zeros((3, 3))):
                z = rng.normal(size=3) * np.array([10.0, 10.0, 1.0])
                cases.append((z + scale * rng.normal(size=3), z, PR.info6(M[None])[0], loss))
    return cases


def test_values_against_numpy_and_the_library(pgo, exe, tmp_path):
    cases = _value_cases()
    out = _run(exe, tmp_path, cases)
    sides = set()
    for (p, z, w, loss), row in zip(cases, out):
        assert row[0] >= 0, (w, "a positive semi-definite information was refused")
        d, chi2, mag, rho = PR.closed(p, z, w, loss)
        np.testing.assert_array_equal(row[1:4], d)   # two subtractions and one remainder: exact operations
        assert abs(row[4] - chi2) <= 4 * EPS * mag, (w, row[4], chi2)
        # the loss at the PROGRAM's chi2: 4 eps relative, every member of the family on both sides of its bend
        ref = [float(v) for v in LR.rho(loss[0], loss[1], np.array(row[4]))]
        for got, exp in zip(row[5:8], ref):
            assert abs(got - exp) <= 4 * EPS * abs(exp), (loss, row[4], got, exp)
        if loss[0] != "trivial":
            sides.add((loss[0], bool(row[4] > loss[1] ** 2)))
        # the library's host entry point runs the same statement: bitwise
        ld, lc, lr = pgo.prior_eval(p, z, w, pgo.Loss(*loss))
        assert np.concatenate([ld, [lc], lr]).tobytes() == np.ascontiguousarray(row[1:8]).tobytes()
    assert sides == {(n, s) for n, _ in LOSSES[1:] for s in (True, False)}


def test_heading_wraps_by_the_ieee_remainder(pgo, exe, tmp_path):
    cases = [((0.0, 0.0, 1.0 + dt), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 0.0, 0.0, 2.0), ("trivial", 0.0)) for dt in WRAPS]
    out = _run(exe, tmp_path, cases)
    for (p, z, w, _), row in zip(cases, out):
        ref = math.remainder(p[2] - z[2], 2.0 * math.pi)
        assert row[3] == ref and abs(row[3]) <= math.pi
        assert row[4] == 2.0 * ref * ref
    # +-pi stay at the ends of [-pi, pi] (up to the rounding of 1 + pi - 1); a hair beyond comes back from the other side; +-6.2 is -+0.083
    assert abs(abs(out[0, 3]) - math.pi) < 1e-15 and abs(abs(out[1, 3]) - math.pi) < 1e-15
    assert out[2, 3] < -3.14 and out[3, 3] > 3.14
    assert out[4, 3] == pytest.approx(6.2 - 2.0 * math.pi, abs=1e-15) and out[5, 3] == pytest.approx(2.0 * math.pi - 6.2, abs=1e-15)


def test_information_classes(pgo, exe, tmp_path):
    rng = np.random.default_rng(9)
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    rot = lambda ev: PR.info6((Q @ np.diag(ev) @ Q.T)[None])[0]
    mats = [(np.array([4.0, 0, 0, 4.0, 0, 0]), 0),            # diag(a, a, 0): position only
            (rot([2.0, 3.0, 0.0]), 0),                         # the same, rotated: zero up to rounding
            (np.zeros(6), 0),
            (np.array([1e-300, 0, 0, 1e-300, 0, 1e-300]), 1), (np.array([1e300, 0, 0, 1e300, 0, 1e300]), 1),
            (rot([2.0, 3.0, 1e-6]), 1),
            (rot([2.0, 3.0, -1e-6]), -1), (np.array([1.0, 2.0, 0, 1.0, 0, 1.0]), -1), (np.array([-1.0, 0, 0, 1.0, 0, 1.0]), -1),
            (np.array([0.0, 0, 0, 0, 0, -1e-300]), -1),
            (np.array([np.nan, 0, 0, 1.0, 0, 1.0]), -2), (np.array([1.0, 0, np.inf, 1.0, 0, 1.0]), -2)]
    cases = [((0.1, 0.2, 0.3), (0.0, 0.0, 0.0), w, ("trivial", 0.0)) for w, _ in mats]
    out = _run(exe, tmp_path, cases)
    for (w, cls), row in zip(mats, out):
        assert int(row[0]) == cls, (w, row[0])
        if cls < 0:   # ... and pgo_prior_eval refuses what pgo_set_priors would
            with pytest.raises(pgo.PgoError) as e:
                pgo.prior_eval((0.1, 0.2, 0.3), (0.0, 0.0, 0.0), w)
            assert e.value.status == -1
        else:
            d, chi2, rho = pgo.prior_eval((0.1, 0.2, 0.3), (0.0, 0.0, 0.0), w)
            assert chi2 == row[4] and chi2 >= 0.0


def test_symbols_and_null_arguments(pgo):
    import ctypes
    hdr = open(os.path.join(os.path.dirname(NS.CSRC), "..", "include", "pgo.h")).read()
    for sym in ("pgo_set_priors", "pgo_num_priors", "pgo_get_prior_residuals", "pgo_prior_eval"):
        assert sym in pgo.EXPORTS and sym + "(" in hdr
        assert getattr(pgo.lib(), sym) is not None
    L = pgo.lib()
    assert L.pgo_set_priors(None, 0, None, None, None, None) == -1
    assert L.pgo_num_priors(None) == 0
    assert L.pgo_get_prior_residuals(None, None, None, None) == -1
    v = np.zeros(6)
    dp = v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.pgo_prior_eval(None, dp, dp, None, dp, dp, dp) == -1
    assert L.pgo_prior_eval(dp, dp, dp, None, None, None, None) == 0   # every output is optional
    with pytest.raises(pgo.PgoError):
        pgo.prior_eval((0, 0, 0), (0, 0, 0), np.eye(3), pgo.Loss("cauchy", -1.0))
