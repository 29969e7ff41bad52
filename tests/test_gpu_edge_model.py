"""GPU: the four kernels that evaluate csrc/edge_model.h -- K1 (k_edge_eval, with and without Jacobian, the default and
the per-class-loss instantiations), k_edge_chi2, k_gate_eval and k_window_solve -- on ONE small graph that sits on every
branch of the model, against the same header compiled for the host (tests/native/edge_model_main.cpp, built plain here;
tests/test_edge_model_host.py runs it under ASan + UBSan on the CPU).

Bounds: residuals and Jacobians 1e-11 absolute and costs 1e-12 relative, the ones test_edge_kernel_parity holds K1 to against
the oracle; chi2 against |r|^2 of the host residual: 2 sqrt(3) |r| 1e-11 (r is held to 1e-11 per entry) + 16 eps |r|^2 (a
nine-term quadratic form in double precision).  Different kernels are not compared bitwise: they share the source, the
compiler contracts each on its own."""
import numpy as np
import pytest

import _native_san as NS

pytestmark = pytest.mark.gpu

TOL = 1e-11
EPS = np.finfo(np.float64).eps
PHI = 0.5
DELTA = 0.5          # Huber: |e|^2 > 0.25 is the linear side
INACTIVE = 9


def rot(t):
    return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])


def measurement(Pa, Pb, e_xy, sin_delta):
    """the measurement that leaves the residual (e_xy, asin(sin_delta)) on the edge Pa -> Pb"""
    dth = (Pb[2] - Pa[2]) - np.arcsin(sin_delta)
    m = rot(Pa[2]).T @ (Pb[:2] - Pa[:2]) - rot(dth) @ np.asarray(e_xy, float)
    return [m[0], m[1], dth]


def graph():
    """8 poses, 10 edges: 0-6 odometry (3 beyond the Huber threshold, 5 at sin delta = 0.999), 7 / 8 DCS with psi just above /
    just below 1, 9 a DCS edge that the active set leaves out"""
    poses = np.array([[0, 0, 0], [1, 0, 0.1], [2, 0.1, 0.2], [3, 0.1, 0.1], [4, 0, 0], [5, 0, -0.1], [6, 0.2, 0], [7, 0, 0.1]], float)
    ia = np.array([0, 1, 2, 3, 4, 5, 6, 0, 1, 2], np.int32)
    ib = np.array([1, 2, 3, 4, 5, 6, 7, 4, 6, 7], np.int32)
    kind = np.array([0] * 7 + [1] * 3, np.uint8)
    resid = [([0.01, -0.02], 0.01), ([-0.03, 0.01], -0.02), ([0.02, 0.02], 0.005), ([0.8, 0.0], 0.01), ([0.0, 0.04], -0.03),
             ([0.05, -0.05], 0.999), ([-0.01, 0.03], 0.02), ([0.70710678, 0.0], 0.0), ([0.70710679, 0.0], 0.0), ([0.9, -0.4], 0.3)]
    meas = np.array([measurement(poses[a], poses[b], e, sd) for a, b, (e, sd) in zip(ia, ib, resid)])
    return poses, ia, ib, meas, kind


def huber(s):
    """(rho, sqrt(rho')) of Huber(DELTA) at s = |e|^2"""
    lin = s > DELTA * DELTA
    rs = np.sqrt(np.where(lin, s, 1.0))
    return np.where(lin, 2.0 * DELTA * rs - DELTA * DELTA, s), np.where(lin, np.sqrt(DELTA / rs), 1.0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host program's records of the graph: plain (r0, J0) and under METHOD 1 (r1, J1), no loss"""
    tmp = tmp_path_factory.mktemp("edge_model_gpu")
    poses, ia, ib, meas, kind = graph()
    exe = NS.build(tmp, "edge_model_main", sanitize=False)
    return NS.edge_model(exe, tmp, poses[ia], poses[ib], meas, (kind != 0).astype(int), PHI)


def test_graph_sits_on_every_branch(host):
    r0, J0, r1, J1 = host
    s = (r1 ** 2).sum(axis=1)
    assert np.array_equal(r0[7], r1[7]) and 0.0 < r1[8][0] < r0[8][0]             # psi just above / just below 1
    assert (r0[7, :2] ** 2).sum() < PHI < (r0[8, :2] ** 2).sum()
    assert s[3] > DELTA ** 2 and (s[[0, 1, 2, 4, 6]] < DELTA ** 2).all()           # both sides of the Huber threshold
    assert np.sin(r0[5][2]) == pytest.approx(0.999, abs=1e-14)
    assert np.isfinite(J1).all()


def test_kernels_against_the_host_statement(pgo, host):
    r0, J0, r1, J1 = host
    poses, ia, ib, meas, kind = graph()
    E = len(ia)
    ident = np.tile([1.0, 0, 0, 1.0, 0, 1.0], (E, 1))
    g = pgo.Graph.from_arrays(poses, ia, ib, meas, kind, info=ident)
    s = pgo.Solver(g, pgo.Options(method=1, phi=PHI, huber_delta=DELTA))
    sq = (r1 ** 2).sum(axis=1)
    rho, sc = huber(sq)

    def check_k1(active):
        for apply_loss in (False, True):
            f = (sc if apply_loss else np.ones(E)) * active
            c, r, J = s.evaluate(apply_loss=apply_loss)                         # with the Jacobian
            dr, dJ = np.abs(r - f[:, None] * r1).max(), np.abs(J - f[:, None] * J1).max()
            print("K1 active %d apply_loss %d: max |dr| %.3g  max |dJ| %.3g" % (active.sum(), apply_loss, dr, dJ))
            assert dr < TOL and dJ < TOL
            assert c == pytest.approx(0.5 * (rho * active).sum(), rel=1e-12)
            c2, _, _ = s.evaluate(apply_loss=apply_loss, want_r=False, want_J=False)   # without
            assert c2 == pytest.approx(0.5 * (rho * active).sum(), rel=1e-12)
        return c

    # K1, the default instantiations (one Huber for every edge)
    check_k1(np.ones(E))
    # chi2 with identity information: |r|^2 of the plain residual
    chi2 = s.edge_chi2()
    n2 = (r0 ** 2).sum(axis=1)
    assert (np.abs(chi2 - n2) <= 2.0 * np.sqrt(3.0) * np.sqrt(n2) * TOL + 16.0 * EPS * n2).all(), (chi2, n2)
    # the gate: the same edges as candidates; r and J of the plain model, unscaled
    out, _ = s.gate(ia, ib, meas)
    assert (out["status"] == 0).all()
    dr, dJ = np.abs(out["r"] - r0).max(), np.abs(out["J"].reshape(E, 18) - J0).max()
    print("gate: max |dr| %.3g  max |dJ| %.3g" % (dr, dJ))
    assert dr < TOL and dJ < TOL
    # K1, the per-class-loss instantiations: an edge mask puts the handle on them; the inactive edge's record is all zero
    active = np.ones(E)
    active[INACTIVE] = 0.0
    s.set_active(active.astype(np.uint8))
    k1_cost = check_k1(active)
    _, r, J = s.evaluate()
    assert not r[INACTIVE].any() and not J[INACTIVE].any()
    # the window kernel on a window holding all of the problem: its initial cost is the sum of K1's costs.  (The ABI takes
    # max_iters >= 1; initial_cost is the cost before the first step whatever the iteration limit.)
    _, res = s.window_solve([(np.arange(len(poses)), np.nonzero(active)[0], 0)], max_iters=1)
    print("window initial cost %r, K1 %r" % (res[0].initial_cost, k1_cost))
    assert res[0].initial_cost == pytest.approx(k1_cost, rel=1e-12)
    assert res[0].initial_cost == pytest.approx(0.5 * (rho * active).sum(), rel=1e-12)
    s.close()
