"""CPU: the robust loss family (pgo_loss_evaluate) against Ceres' closed forms and central differences, the numpy
restatement of tests/_loss_restatement.py against the golden fixtures (Huber(0.01) must reproduce the oracle's
direct-solve trajectories: that validates the reference the GPU loss tests use), and the host side of the C-ABI."""
import ctypes
import json
import os

import numpy as np
import pytest

import _loss_restatement as LR
from conftest import DATA, GOLDEN, ROOT

SCALES = {"trivial": 0.0, "huber": 0.01, "softlone": 0.3, "cauchy": 0.3, "arctan": 0.7, "tukey": 0.5}


@pytest.mark.parametrize("name", list(LR.TYPES))
def test_loss_evaluate_matches_closed_forms(pgo, name):
    a = SCALES[name]
    L = pgo.Loss(name, a)
    for s in (0.0, 1e-6, 1e-4, 0.09, 0.2499, 0.25, 0.2501, 0.49, 1.0, 3.7, 1e3, 1e8):
        got = L.evaluate(s)
        exp = np.array([v[0] for v in LR.rho(name, a, np.array([s]))])
        np.testing.assert_allclose(got, exp, rtol=1e-14, atol=1e-300)
    np.testing.assert_array_equal(L.evaluate(0.0)[:2], [0.0, 1.0])   # rho(0) = 0, rho'(0) = 1


@pytest.mark.parametrize("name", list(LR.TYPES))
def test_loss_derivatives_are_central_differences(pgo, name):
    a = SCALES[name]
    L = pgo.Loss(name, a)
    for s in (0.003, 0.05, 0.2, 0.7, 2.5, 40.0):
        if name == "tukey" and abs(s - a * a) < 0.05:
            continue
        h = 1e-6 * max(1.0, s)
        d1 = (L.evaluate(s + h)[0] - L.evaluate(s - h)[0]) / (2 * h)
        d2 = (L.evaluate(s + h)[1] - L.evaluate(s - h)[1]) / (2 * h)
        rho = L.evaluate(s)
        assert d1 == pytest.approx(rho[1], rel=1e-6, abs=1e-9)
        assert d2 == pytest.approx(rho[2], rel=1e-5, abs=1e-8)
        assert rho[2] <= 0.0   # every loss of the family: the corrector is a plain sqrt(rho') scaling


def test_loss_floor_and_tukey_sides(pgo):
    # rho' never underflows to 0 for the non-Tukey losses (Ceres' max(DBL_MIN, .))
    for name in ("huber", "softlone", "cauchy", "arctan"):
        assert pgo.Loss(name, 1e-3).evaluate(1e300)[1] >= LR.DBL_MIN
    assert pgo.Loss("huber", 1e-3).evaluate(1e300)[1] == pytest.approx(1e-3 / 1e150)
    assert pgo.Loss("arctan", 1.0).evaluate(1e300)[1] == LR.DBL_MIN
    T = pgo.Loss("tukey", 0.5)
    inside, at, beyond = T.evaluate(0.2), T.evaluate(0.25), T.evaluate(0.3)
    v = 1.0 - 0.2 / 0.25
    np.testing.assert_allclose(inside, [0.25 / 3.0 * (1 - v ** 3), v * v, -2.0 * v / 0.25], rtol=1e-14)
    np.testing.assert_allclose(at, [0.25 / 3.0, 0.0, 0.0], atol=1e-17)
    np.testing.assert_array_equal(beyond, [0.25 / 3.0, 0.0, 0.0])   # constant cost, zero rows
    # Huber's branch point: s <= b is the quadratic side
    np.testing.assert_array_equal(pgo.Loss("huber", 0.5).evaluate(0.25), [0.25, 1.0, 0.0])


def test_loss_argument_errors(pgo):
    for name, a in (("cauchy", 0.0), ("tukey", -1.0), ("huber", float("nan")), ("softlone", float("inf"))):
        with pytest.raises(pgo.PgoError) as e:
            pgo.Loss(name, a).evaluate(1.0)
        assert e.value.status == -1
    assert pgo.Loss("trivial", float("nan")).evaluate(2.0)[0] == 2.0   # Trivial ignores its scale
    bad = pgo.Loss("cauchy", 1.0)
    bad.type = 6
    with pytest.raises(pgo.PgoError):
        bad.evaluate(1.0)
    with pytest.raises(ValueError):
        pgo.Loss("welsch", 1.0)
    L = pgo.lib()
    rho = np.zeros(3)
    assert L.pgo_loss_evaluate(None, 1.0, rho.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    assert L.pgo_loss_evaluate(ctypes.byref(pgo.Loss("cauchy", 1.0)), 1.0, None) == -1


def test_set_losses_symbols_and_null_handles(pgo):
    hdr = open(os.path.join(ROOT, "include", "pgo.h")).read()
    for sym in ("pgo_loss_evaluate", "pgo_set_losses", "pgo_batch_set_losses"):
        assert sym in pgo.EXPORTS and sym + "(" in hdr
        assert getattr(pgo.lib(), sym) is not None
    arr = (pgo.Loss * 1)(pgo.Loss("cauchy", 0.1))
    assert pgo.lib().pgo_set_losses(None, 1, arr, None) == -1
    assert pgo.lib().pgo_batch_set_losses(None, 1, arr, None) == -1


def _graph(O, name, n_out):
    g = O.read_g2o(os.path.join(DATA, name + ".g2o"))
    return O.add_random_C(g, n_out, 1) if n_out else g


@pytest.mark.parametrize("name,n_out,method", [("INTEL", 50, 0), ("INTEL", 50, 1), ("MIT", 0, 1), ("M3500", 0, 1),
                                               ("INTEL", 50, 2)])
def test_restatement_with_huber_reproduces_golden(oracle, name, n_out, method):
    """the restated corrector + LM loop with one Huber(0.01) class follows the oracle's golden trajectories to the
    bounds of test_lm_solve_matches_golden"""
    og = _graph(oracle, name, n_out)
    tag = "%s_out%d_m%d" % (name, n_out, method)
    fx = json.load(open(os.path.join(GOLDEN, "lm_%s.json" % tag)))
    ref = np.load(os.path.join(GOLDEN, "lm_%s_poses.npy" % tag))
    cls = LR.classes(og.kind, 1)
    res = LR.lm(oracle, og, [("huber", 0.01)], cls, method=method)
    assert res.termination == fx["termination"] and res.iterations == fx["iterations"]
    assert res.initial_cost == pytest.approx(fx["initial_cost"], rel=1e-12)
    assert res.final_cost == pytest.approx(fx["final_cost"], rel=1e-7)
    assert len(res.records) == len(fx["records"])
    for a, b in zip(res.records, fx["records"]):
        assert a["step_ok"] == b["step_ok"]
        assert a["cost"] == pytest.approx(b["cost"], rel=1e-6)
    assert np.abs(res.poses[:, :2] - ref[:, :2]).max() < 5e-6
    if method == 2:
        sw = np.load(os.path.join(GOLDEN, "lm_%s_switches.npy" % tag))
        assert np.abs(res.switches - sw).max() < 1e-6


def test_restatement_corrector_matches_oracle_huber(oracle):
    """the restated corrector with Huber(0.01) equals the oracle's own Huber corrector, METHOD 0 / 1 / 2 and weighted"""
    og = _graph(oracle, "INTEL", 50)
    cls = LR.classes(og.kind, 1)
    for method in (0, 1):
        for iw in (False, True):
            if iw and method == 0:
                g2 = og.copy()
                g2.info = np.tile(np.array([2.0, 0.1, 0.0, 3.0, 0.0, 5.0]), (og.n_edges, 1))
            else:
                g2 = og
            c, r, J = LR.evaluate(oracle, g2, [("huber", 0.01)], cls, method=method, info_weighting=iw and method == 0)
            oc, orr, oJ = oracle.evaluate(g2, method=method, info_weighting=iw and method == 0)
            assert c == pytest.approx(oc, rel=1e-13)
            np.testing.assert_allclose(r, orr, rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(J, oJ, rtol=1e-13, atol=1e-15)
    sw = np.ones(og.n_edges)
    sw[og.kind != 0] = np.linspace(0.2, 1.0, int((og.kind != 0).sum()))
    c, r, J, Js, q = LR.evaluate_sc(oracle, og, [("huber", 0.01)], cls, switches=sw)
    oc, orr, oJ, oJs, oq = oracle.evaluate_sc(og, switches=sw)
    assert c == pytest.approx(oc, rel=1e-13)
    for x, y in ((r, orr), (J, oJ), (Js, oJs), (q, oq)):
        np.testing.assert_allclose(x, y, rtol=1e-13, atol=1e-15)
