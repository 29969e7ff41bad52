"""CPU: the SE(2) edge model (csrc/edge_model.h, the one statement behind k_edge_eval, k_edge_chi2, k_gate_eval and
k_window_solve) through tests/native/edge_model_main.cpp under ASan + UBSan, against the oracle's Jet restatement
(oracle/pgo_oracle.c).  Bound: 1e-11 absolute on residuals and Jacobians, the one test_edge_kernel_parity holds the kernel to
against the same oracle."""
import os

import numpy as np
import pytest

import _native_san as NS
from conftest import DATA

TOL = 1e-11
PHI = 0.5


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("edge_model"), "edge_model_main")


@pytest.mark.parametrize("name,n_out", [("INTEL", 50), ("M3500", 0)])
def test_every_edge_matches_oracle(oracle, exe, tmp_path, name, n_out):
    g = oracle.read_g2o(os.path.join(DATA, name + ".g2o"))
    if n_out:
        g = oracle.add_random_C(g, n_out, 1)
    r0, J0, r1, J1 = NS.edge_model(exe, tmp_path, g.poses[g.ia], g.poses[g.ib], g.meas, (g.kind != 0).astype(int), PHI)
    for method, r, J in ((0, r0, J0), (1, r1, J1)):
        _, orr, oJ = oracle.evaluate(g, method=method, phi=PHI, apply_loss=False)
        dr, dJ = np.abs(r - orr).max(), np.abs(J - oJ).max()
        print("%s method %d: %d edges, max |dr| %.3g, max |dJ| %.3g" % (name, method, g.n_edges, dr, dJ))
        assert dr < TOL and dJ < TOL
    dcs = g.kind != 0
    assert np.array_equal(r0[~dcs], r1[~dcs]) and np.array_equal(J0[~dcs], J1[~dcs])   # DCS only where the flag says so
    assert (np.abs(r1[dcs]) < np.abs(r0[dcs])).any()                                    # and it does bite on some edge


def hand_cases():
    """(P1, P2, meas, what) at every branch of the model; |sin delta| = 1 is left out: the Jacobian is not defined there"""
    z = [0.0, 0.0, 0.0]
    return [
        (z, [0.70710678, 0, 0], z, "DCS, ex^2 just below phi: psi just above 1, not applied"),
        (z, [0.70710679, 0, 0], z, "DCS, ex^2 just above phi: psi just below 1"),
        (z, [0.0, 0.0, 2.5], z, "the asin fold: delta = 2.5"),
        (z, [0.3, -0.2, float(np.arcsin(0.999))], z, "sin delta = +0.999"),
        (z, [0.3, -0.2, -float(np.arcsin(0.999))], z, "sin delta = -0.999"),
        ([1.0, 2.0, 0.3], [1.0, 2.0, 0.3], z, "identical poses"),
        ([1.0, 2.0, 0.3], [2.5, 1.0, 1.1], [1.2, -0.7, 0.6], "a general edge"),
        (z, [100.0, -50.0, 3.0], z, "far apart"),
    ]


def test_hand_made_cases_match_oracle(oracle, exe, tmp_path):
    cases = hand_cases()
    P1, P2, M = (np.array([c[k] for c in cases]) for k in range(3))
    r0, J0, r1, J1 = NS.edge_model(exe, tmp_path, P1, P2, M, np.ones(len(cases), int), PHI)
    for k, (a, b, m, what) in enumerate(cases):
        for dcs, r, J in ((False, r0[k], J0[k]), (True, r1[k], J1[k])):
            oe, oJ = oracle.edge(a, b, m, dcs, PHI)
            assert np.abs(r - oe).max() < TOL and np.abs(J - oJ.ravel()).max() < TOL, (what, dcs)
    # the branches were taken
    assert np.array_equal(r0[0], r1[0]) and np.array_equal(J0[0], J1[0])          # psi >= 1: untouched
    assert 0.0 < r1[1][0] < r0[1][0] and r1[1][0] == pytest.approx(r0[1][0], rel=1e-8)   # psi just below 1
    assert r0[2][2] == pytest.approx(np.pi - 2.5, abs=1e-15) and J0[2][17] == pytest.approx(-1.0, abs=1e-14)
    assert np.sin(r0[3][2]) == pytest.approx(0.999, abs=1e-15) and np.sin(r0[4][2]) == pytest.approx(-0.999, abs=1e-15)
    assert J0[3][17] == pytest.approx(1.0, abs=1e-12) and J0[4][14] == pytest.approx(-1.0, abs=1e-12)
    assert np.abs(r0[5]).max() < 1e-16
    assert np.isfinite(J0).all() and np.isfinite(J1).all()
