"""The host side of pgo_posterior_sample: pgo_sample_noise_eval against the numpy restatement of the stream
(tests/_sample_restatement.py), the moments of the stream's normals, the defaults and refusals of the host entry points, and
the estimator condition on the restatement ALONE -- for the cases, seeds and sample counts the GPU test uses, the second
moment of exact draws stays inside the Wishart cap, so that the GPU test cannot hide a failure behind statistics."""
import ctypes

import numpy as np
import pytest

import _sample_restatement as SR


def test_noise_eval_equals_the_restatement(pgo):
    rng = np.random.default_rng(17)
    for seed in (0, 1, 2 ** 63 + 12345, 2 ** 64 - 1):
        for stream in (0, 1):
            idx = np.concatenate([[0, 1, 2 ** 32 - 1], rng.integers(0, 2 ** 32, 200)])
            smp = np.concatenate([[0, 2 ** 31 - 1, 5], rng.integers(0, 2 ** 31, 200)])
            ref = SR.triples(seed, stream, idx, smp)
            got = np.stack([pgo.sample_noise_eval(seed, stream, int(i), int(s)) for i, s in zip(idx, smp)])
            assert np.abs(got - ref).max() <= 1e-14


def test_noise_eval_refusals_and_defaults(pgo):
    for bad in ((0, 2, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 2 ** 32, 0), (0, 0, 0, -1)):
        with pytest.raises(pgo.PgoError) as e:
            pgo.sample_noise_eval(*bad)
        assert e.value.status == -1
    assert pgo.lib().pgo_sample_noise_eval(0, 0, 0, 0, None) == -1
    o = pgo.SampleOptions()
    assert (o.rtol, o.max_iters, o.samples_per_pass, o.solver, o.first_sample, o.seed) == (1e-10, 20000, 24, 0, 0, 0)
    assert ctypes.sizeof(o) == 32
    assert pgo.lib().pgo_posterior_sample(None, 1, None, None, None, None) == -1
    assert pgo.lib().pgo_debug_sample_rhs(None, 0, 0, None, None) == -1
    hdr = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "pgo.h")).read()
    for sym in ("pgo_sample_options_default", "pgo_sample_noise_eval", "pgo_posterior_sample", "pgo_debug_sample_rhs"):
        assert sym in pgo.EXPORTS and sym + "(" in hdr and getattr(pgo.lib(), sym) is not None


def test_moments_of_a_million_variates():
    """mean, variance and fourth moment within 5 standard errors of 0, 1 and 3 (their standard errors over n variates:
    sqrt(1 / n), sqrt(2 / n), sqrt(96 / n))"""
    n = 10 ** 6
    z = SR.triples(20260410, 0, np.arange(n // 3 + 1), 3).reshape(-1)[:n]
    assert abs(z.mean()) <= 5 * np.sqrt(1.0 / n)
    assert abs((z * z).mean() - 1.0) <= 5 * np.sqrt(2.0 / n)
    assert abs((z ** 4).mean() - 3.0) <= 5 * np.sqrt(96.0 / n)
    # the three members of a triple, and the two streams, are uncorrelated at the same level
    t = z[:3 * (n // 3)].reshape(-1, 3)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert abs((t[:, a] * t[:, b]).mean()) <= 5 * np.sqrt(3.0 / n)
    w = SR.triples(20260410, 1, np.arange(n // 3 + 1), 3).reshape(-1)[:n]
    assert abs((z * w).mean()) <= 5 * np.sqrt(1.0 / n)


def test_draws_have_the_posterior_covariance_on_a_tiny_problem(pgo, oracle):
    """cov(H^-1 J' eps) = H^-1: on the five-pose walk 20000 restated draws reproduce every marginal block to sampling error"""
    import _solo_cases as SC
    from conftest import oracle_graph
    og = oracle_graph(oracle, SC.pgo_graph(pgo, "five"))
    _, _, J = oracle.evaluate(og, og.poses, method=0)
    P = SR.Problem(og.n_poses, og.ia, og.ib, J)
    S = 20000
    err = SR.whitened_errors(SR.second_moment(P.deltas(5, 0, S))[1:], P.exact_blocks()[1:])
    assert err.max() <= SR.wishart_cap(S)


@pytest.mark.parametrize("name", sorted(SR.ESTIMATOR_CASES))
def test_estimator_condition_on_the_restatement(pgo, oracle, name):
    """|| L^-1 C_i L^-T - I ||_F <= 3 sqrt(12 / S) for every non-constant pose, C from the restatement's own draws"""
    seed, S = SR.ESTIMATOR_CASES[name]
    P = SR.case_problem(pgo, oracle, name)
    C = SR.second_moment(P.deltas(seed, 0, S))
    assert np.array_equal(C[0], np.zeros((3, 3)))
    err = SR.whitened_errors(C[1:], P.exact_blocks()[1:])
    print("%s: seed %d, S = %d: worst whitened error %.4f = %.3f sqrt(12 / S) (cap 3)" % (name, seed, S, err.max(), err.max() / np.sqrt(12.0 / S)))
    assert err.max() <= SR.wishart_cap(S)
