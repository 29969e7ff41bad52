"""pgo_gate_evaluate (host): the 3x3 algebra of the loop-edge gate (csrc/gate.h, what k_gate_reduce runs on the device)
against numpy.  chi2 = r' Omega r, chi2_marginal = r' (P + Omega^-1)^-1 r, info_gain = 1/2 logdet(I + Omega P)."""
import numpy as np
import pytest

EPS = np.finfo(np.float64).eps


def full(info):
    a, b, c, d, e, f = info
    return np.array([[a, b, c], [b, d, e], [c, e, f]])


def spd(rng, lo, hi):
    """random SPD 3x3 with eigenvalues log-uniform in [lo, hi]"""
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    w = np.exp(rng.uniform(np.log(lo), np.log(hi), 3))
    m = (q * w) @ q.T
    return 0.5 * (m + m.T)


def info6(W):
    return np.array([W[0, 0], W[0, 1], W[0, 2], W[1, 1], W[1, 2], W[2, 2]])


def draws(n=200, seed=20261018):
    """(r, P, Omega, M) with cond(M) <= 1e6, M = I + L' P L"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        P = spd(rng, 1e-6, 1e2)
        W = spd(rng, 1e-2, 1e3)
        L = np.linalg.cholesky(W)
        M = np.eye(3) + L.T @ P @ L
        if np.linalg.cond(M) > 1e6:
            continue
        out.append((rng.standard_normal(3) * np.exp(rng.uniform(-6, 3)), P, W, M))
    return out


def test_random_inputs_match_numpy(pgo):
    """tolerance 64 eps cond(M) per draw: relative on chi2_marginal, absolute on info_gain -- the backward-stable 3x3
    Cholesky bound (a solve with M carries a relative error of O(eps cond(M)); so does each log of a pivot)"""
    conds = []
    for r, P, W, M in draws():
        chi2, cm, ig = pgo.gate_evaluate(r, P, info6(W))
        L = np.linalg.cholesky(W)
        v = L.T @ r
        cm_ref = v @ np.linalg.solve(M, v)
        ig_ref = 0.5 * np.linalg.slogdet(M)[1]
        tol = 64 * EPS * np.linalg.cond(M)
        assert abs(cm - cm_ref) <= tol * cm_ref, (cm, cm_ref, tol)
        assert abs(ig - ig_ref) <= tol, (ig, ig_ref, tol)
        assert abs(chi2 - r @ W @ r) <= 16 * EPS * np.linalg.norm(W) * (r @ r)
        # the two forms of the innovation gate agree (P + Omega^-1 is as well conditioned as these draws make it)
        assert cm == pytest.approx(r @ np.linalg.solve(P + np.linalg.inv(W), r), rel=1e-6)
        conds.append(np.linalg.cond(M))
    assert max(conds) > 1e4   # the draws do reach ill-conditioned M


def test_zero_P(pgo):
    rng = np.random.default_rng(3)
    for k in range(20):
        r = rng.standard_normal(3) * 10.0 ** rng.integers(-5, 3)
        chi2, cm, ig = pgo.gate_evaluate(r, np.zeros((3, 3)))
        assert cm == chi2 and ig == 0.0 and chi2 > 0
        W = spd(rng, 1e-2, 1e3)
        chi2, cm, ig = pgo.gate_evaluate(r, np.zeros((3, 3)), info6(W))
        assert ig == 0.0
        assert abs(cm - chi2) <= 16 * EPS * np.linalg.norm(W) * (r @ r)   # (L'r)'(L'r) against r' Omega r: rounding alone


def test_proxy_is_the_identity_P_case(pgo):
    """the reference's compute_info_gain_edge, 1/2 logdet(I + Omega), on the information of an injected loop"""
    w = np.array([2.0, 0, 0, 300.0, 0, 300.0])
    chi2, cm, ig = pgo.gate_evaluate([0.1, -0.2, 0.05], np.eye(3), w)
    assert ig == pytest.approx(0.5 * (np.log(3.0) + 2 * np.log(301.0)), rel=4 * EPS)
    r = np.array([0.1, -0.2, 0.05])
    assert cm == pytest.approx(r @ np.linalg.solve(np.eye(3) + np.diag([0.5, 1 / 300, 1 / 300]), r), rel=1e-14)


def test_identity_information_is_the_default(pgo):
    rng = np.random.default_rng(5)
    for k in range(10):
        r, P = rng.standard_normal(3), spd(rng, 1e-4, 10.0)
        assert pgo.gate_evaluate(r, P) == pgo.gate_evaluate(r, P, [1.0, 0, 0, 1.0, 0, 1.0])


def test_errors(pgo):
    r, P = np.ones(3), np.eye(3)
    for w in ([1.0, 2.0, 0, 1.0, 0, 1.0], [0.0, 0, 0, 1.0, 0, 1.0], [1.0, 0, 0, 1.0, 0, -1.0], [np.nan, 0, 0, 1.0, 0, 1.0],
              [np.inf, 0, 0, 1.0, 0, 1.0]):
        with pytest.raises(pgo.PgoError) as e:
            pgo.gate_evaluate(r, P, w)
        assert e.value.status == -1, w
    with pytest.raises(pgo.PgoError) as e:   # an indefinite P: M = I + P has a negative pivot
        pgo.gate_evaluate(r, np.diag([1.0, -3.0, 1.0]))
    assert e.value.status == -7
    with pytest.raises(pgo.PgoError) as e:
        pgo.gate_evaluate(r, np.full((3, 3), np.nan))
    assert e.value.status == -7
