"""pgo_coarsen_info_plan (include/pgo.h, "hierarchical initialisation", "with information"; host only): the closed form of
the straight unit chain bitwise, the numpy restatement of tests/_coarsen_info_cases.py to the bounds derived there, the
first-order statement itself against a Monte Carlo run, the symmetry under storing an edge the other way round, and the
refusals."""
import numpy as np
import pytest

import _coarsen_cases as CC
import _coarsen_info_cases as CI

INVALID_ARG, NUMERIC = -1, -7


def chain_graph(n, extra=()):
    """a straight chain of unit steps plus the edges of `extra` = (a, b, kind), measurements the exact relatives"""
    P = np.stack([np.arange(n, dtype=float), np.zeros(n), np.zeros(n)], -1)
    ia = np.concatenate([np.arange(n - 1), [e[0] for e in extra]]).astype(np.int32)
    ib = np.concatenate([np.arange(1, n), [e[1] for e in extra]]).astype(np.int32)
    kind = np.concatenate([np.zeros(n - 1), [e[2] for e in extra]]).astype(np.uint8)
    return P, ia, ib, CC.relative(P[ia], P[ib]), kind


def graph_with_info(pgo, name):
    """(n, ia, ib, meas, kind, info): random SPD information on the generated graphs, the datasets' own on the others"""
    if name == "exact130":
        P, ia, ib, meas, kind = CC.exact_graph(130, 12, 5)
        return 130, ia, ib, meas, kind, CI.random_spd_info(len(ia), 1)
    g = getattr(CC, name)(pgo) if name in ("synth600", "intel50") else CC.dataset(pgo, name)
    n, ia, ib, meas, kind = CC.arrays(g)
    return n, ia, ib, meas, kind, (CI.random_spd_info(len(ia), 2) if name == "synth600" else np.array(g.info))


# ------------------------------------------------------------------------------------------------ 1. known answer, exact
@pytest.mark.parametrize("S", CC.STRIDES)
def test_straight_chain_is_the_closed_form_bitwise(pgo, S):
    """unit steps, unit information: every entry is an integer below 2^53, so C's and Cend's covariances are the closed form
    bitwise; a loop between two key poses has identity pairs on both sides and keeps Omega^-1 bitwise (here powers of two)"""
    n = 2 * S + 3
    P, ia, ib, meas, kind = chain_graph(n, [(0, 2 * S, 1), (2 * S, S, 2), (1, S + 1, 1)])
    info = CI.unit_info(len(ia))
    info[n - 1] = [4.0, 0, 0, 16.0, 0, 0.25]
    info[n] = [0.25, 0, 0, 4.0, 0, 64.0]
    got = pgo.coarsen_info_plan(n, ia, ib, meas, kind, S, info)
    j, K = np.arange(n) % S, got["n_poses"]
    assert got["Ccov"].tobytes() == CI.straight_chain_cov(j).tobytes()
    assert got["Cendcov"].tobytes() == CI.straight_chain_cov(np.full(K - 1, S)).tobytes()
    assert got["cov"][:K - 1].tobytes() == got["Cendcov"].tobytes()
    assert list(got["origin"]) == [-1] * (K - 1) + [n - 1, n, n + 1]
    assert got["cov"][K - 1].tobytes() == np.array([0.25, 0, 0, 0.0625, 0, 4.0]).tobytes()
    assert got["cov"][K].tobytes() == np.array([4.0, 0, 0, 0.25, 0, 0.015625]).tobytes()
    assert got["info"][K - 1].tobytes() == info[n - 1].tobytes() and got["info"][K].tobytes() == info[n].tobytes()
    # the closed form against the restatement; the third loop runs one step into both segments, (1, 0, 0) o (S, 0, 0) o
    # (1, 0, 0)^-1: integers again
    want = CI.restate_coarsen_info(n, ia, ib, meas, kind, info, S)
    assert np.array_equal(want["Ccov"], got["Ccov"]) and np.array_equal(want["Cendcov"], got["Cendcov"])
    assert np.array_equal(got["cov"][K + 1], want["cov"][K + 1]) and np.array_equal(got["meas"], want["meas"])


def test_composing_with_the_identity_pair_changes_no_bit(pgo):
    """a loop between key poses with a full information matrix and a turning measurement: covariance = the plan's own Omega^-1
    (what it gives for the same matrix on a chain edge at the start of a segment), bitwise"""
    S, n = 4, 9
    P, ia, ib, meas, kind = chain_graph(n, [(0, 8, 1)])
    info = CI.random_spd_info(len(ia), 3)
    info[0] = info[n - 1]
    meas[n - 1] = [3.7, -1.2, 2.5]
    got = pgo.coarsen_info_plan(n, ia, ib, meas, kind, S, info)
    assert got["cov"][2].tobytes() == got["Ccov"][1].tobytes()
    CI.assert_close_cov(got["cov"][2], CI.vec6(np.linalg.inv(CI.mat(info[0]))), 64 * CI.EPS * np.linalg.cond(CI.mat(info[0])), "Omega^-1")


# ------------------------------------------------------------------------------------------------ 2. plan against restatement
@pytest.mark.parametrize("name", ["exact130", "synth600", "intel50", "MIT"])
def test_plan_is_the_restatement(pgo, name):
    n, ia, ib, meas, kind, info = graph_with_info(pgo, name)
    for S in CC.STRIDES:
        if n <= S:
            continue
        got = pgo.coarsen_info_plan(n, ia, ib, meas, kind, S, info)
        plain = pgo.coarsen_plan(n, ia, ib, meas, kind, S)
        want = CI.restate_coarsen_info(n, ia, ib, meas, kind, info, S)
        CC.assert_same_structure(got, want)
        for k in ("meas", "C", "Cend"):                                  # the means are pgo_coarsen_plan's, bitwise
            assert got[k].tobytes() == plain[k].tobytes(), k
        tol_xy, tol_th = CC.bounds(n, ia, ib, meas, S)
        CC.assert_close_poses(got["meas"], want["meas"], tol_xy, tol_th, "%s S=%d coarse measurements" % (name, S))
        rel_cov, rel_info = CI.bounds(n, ia, ib, meas, info, S, want)
        CI.assert_close_cov(got["cov"], want["cov"], rel_cov, "%s S=%d cov" % (name, S))
        CI.assert_close_cov(got["info"], want["info"], rel_info, "%s S=%d info" % (name, S))
        K = got["n_poses"]
        assert got["cov"][:K - 1].tobytes() == got["Cendcov"].tobytes() and not got["Ccov"][::S].any()
        rest = np.arange(n) % S != 0
        CI.assert_close_cov(got["Ccov"][rest], want["Ccov"][rest], CI.bounds_C(n, ia, ib, meas, info, S, want), "%s S=%d Ccov" % (name, S))


def test_null_information_is_unit_information(pgo):
    g = CC.synth600(pgo)
    n, ia, ib, meas, kind = CC.arrays(g)
    a = pgo.coarsen_info_plan(n, ia, ib, meas, kind, 16, None)
    b = pgo.coarsen_info_plan(n, ia, ib, meas, kind, 16, CI.unit_info(len(ia)))
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


# ------------------------------------------------------------------------------------------------ 3. first-order validity
def monte_carlo(factors, n_draws, seed):
    """factors: (motion, Sigma 3x3, inverted) in order; the sample covariance of the product of the perturbed factors minus
    the unperturbed product, angle difference wrapped"""
    rng = np.random.default_rng(seed)
    R = R0 = None
    for m, Sg, inv in factors:
        d = rng.multivariate_normal(np.zeros(3), Sg, n_draws)
        Z, Z0 = m + d, np.asarray(m, np.float64)
        if inv:
            Z, Z0 = CC.inverse(Z), CC.inverse(Z0)
        R, R0 = (Z, Z0) if R is None else (CC.compose(R, Z), CC.compose(R0, Z0))
    D = R - R0
    D[:, 2] = CC.wrap(D[:, 2])
    return D.T @ D / n_draws


@pytest.mark.parametrize("case", ["composite16", "transport7_1_11"])
def test_first_order_covariance_is_the_sample_covariance(pgo, case):
    """Every contributing measurement perturbed by N(0, Sigma_e), n = 200000 draws: the sample covariance of the transported
    measurement against the plan's coarse_cov, relative in the Frobenius norm.  Bound: the sampling error 5 sqrt(2 / n) the
    issue states, plus the second-order term.  The latter: with t the accumulated heading error, variance V = the sum of the
    theta variances of the factors, a lever arm l turns by l (sin t, 1 - cos t) ~ l (t, t^2 / 2); the quadratic part has
    variance l^2 V^2 / 2 against the linear part's l^2 V -- a ratio V / 2 -- and E[t^2 / 2] = V / 2 shifts the mean, which
    the sample covariance about the unperturbed product sees squared, l^2 V^2 / 4: together below V relative."""
    n_draws = 200000
    rng = np.random.default_rng(4)
    sig = np.array([0.02, 0.02, 0.01])
    if case == "composite16":
        S, n = 16, 33
        extra = []
    else:
        S, n = 16, 40
        extra = [(7, 16 + 11, 1)]
    th = np.cumsum(rng.normal(0, 0.3, n))
    P = np.stack([np.cumsum(np.cos(th)), np.cumsum(np.sin(th)), th], -1)
    ia = np.concatenate([np.arange(n - 1), [e[0] for e in extra]]).astype(np.int32)
    ib = np.concatenate([np.arange(1, n), [e[1] for e in extra]]).astype(np.int32)
    ia[3], ib[3] = ib[3], ia[3]                                          # one chain edge stored the other way round
    kind = np.concatenate([np.zeros(n - 1), [e[2] for e in extra]]).astype(np.uint8)
    meas = CC.relative(P[ia], P[ib])
    info = np.tile(CI.vec6(np.diag(1 / sig ** 2)), (len(ia), 1))
    if extra:
        info[n - 1] = CI.vec6(np.diag(1 / np.array([0.05, 0.05, 0.02]) ** 2))
    Sg = np.linalg.inv(CI.mat(info))
    got = pgo.coarsen_info_plan(n, ia, ib, meas, kind, S, info)
    z = lambda i: (meas[i], Sg[i], ia[i] != i)
    if case == "composite16":
        factors, slot = [z(i) for i in range(16)], 0
    else:
        factors = [z(i) for i in range(7)] + [(meas[n - 1], Sg[n - 1], False)] + [(m, s_, not v) for m, s_, v in reversed([z(i) for i in range(16, 27)])]
        slot = len(got["ia"]) - 1
        assert got["origin"][slot] == n - 1
    V = sum(f[1][2, 2] for f in factors)
    sample, want = monte_carlo(factors, n_draws, 5), CI.mat(got["cov"][slot])
    rel = np.linalg.norm(sample - want) / np.linalg.norm(want)
    bound = 5 * np.sqrt(2 / n_draws) + V
    print("%s: |sample - plan| / |plan| = %.3e (bound %.3e: sampling %.3e + second order %.3e)" % (case, rel, bound, 5 * np.sqrt(2 / n_draws), V))
    assert rel <= bound


# ------------------------------------------------------------------------------------------------ 4. symmetry
def test_an_edge_stored_the_other_way_round_gives_the_inverse_pair(pgo):
    """(b, a, m^-1) with information H^-T Omega H^-1 is the same constraint: the coarse pair is the inverse pair.  The
    congruence by H of the coarse mean amplifies a relative error by at most cond(H)^2."""
    n, ia, ib, meas, kind, info = graph_with_info(pgo, "exact130")
    S = 7
    a = pgo.coarsen_info_plan(n, ia, ib, meas, kind, S, info)
    ref = CI.restate_coarsen_info(n, ia, ib, meas, kind, info, S)
    rel_cov, _ = CI.bounds(n, ia, ib, meas, info, S, ref)
    K = a["n_poses"]
    e = int(a["origin"][K])                                              # the first kept loop
    ia2, ib2, meas2, info2 = ia.copy(), ib.copy(), meas.copy(), info.copy()
    ia2[e], ib2[e] = ib[e], ia[e]
    meas2[e], Sg = CI.pair_inverse((meas[e], np.linalg.inv(CI.mat(info[e]))))
    info2[e] = CI.vec6(np.linalg.inv(Sg))
    b = pgo.coarsen_info_plan(n, ia2, ib2, meas2, kind, S, info2)
    assert (b["ia"][K], b["ib"][K]) == (a["ib"][K], a["ia"][K])
    m_inv, S_inv = CI.pair_inverse((a["meas"][K], CI.mat(a["cov"][K])))
    tol_xy, tol_th = CC.bounds(n, ia, ib, meas, S)
    CC.assert_close_poses(b["meas"][K], m_inv, 2 * tol_xy, 2 * tol_th, "inverse mean")
    c, s = np.cos(a["meas"][K, 2]), np.sin(a["meas"][K, 2])
    H = np.array([[-c, -s, m_inv[1]], [s, -c, -m_inv[0]], [0, 0, -1]])
    CI.assert_close_cov(b["cov"][K], CI.vec6(S_inv), 2 * rel_cov[K] * np.linalg.cond(H) ** 2, "inverse covariance")
    keep = np.arange(len(a["ia"])) != K                                   # nothing else moves
    assert a["cov"][keep].tobytes() == b["cov"][keep].tobytes()
    # a chain edge stored the other way round: the same Z_i, every coarse edge within the bounds
    i = 10
    ia3, ib3, meas3, info3 = ia.copy(), ib.copy(), meas.copy(), info.copy()
    ia3[i], ib3[i] = ib[i], ia[i]
    meas3[i], Sg = CI.pair_inverse((meas[i], np.linalg.inv(CI.mat(info[i]))))
    info3[i] = CI.vec6(np.linalg.inv(Sg))
    c3 = pgo.coarsen_info_plan(n, ia3, ib3, meas3, kind, S, info3)
    ref3 = CI.restate_coarsen_info(n, ia3, ib3, meas3, kind, info3, S)
    CI.assert_close_cov(c3["cov"], a["cov"], 2 * CI.bounds(n, ia3, ib3, meas3, info3, S, ref3)[0], "chain edge reversed")


# ------------------------------------------------------------------------------------------------ 5. refusals
def first_bad_used_edge(n, ia, ib, info, S):
    chain, _ = CC.chain_edges(n, ia, ib)
    is_chain = np.zeros(len(ia), bool)
    is_chain[chain[:n - 1]] = True
    used = is_chain | (ia // S != ib // S)
    M = CI.mat(info)
    bad = ~np.isfinite(M).all(axis=(-2, -1))
    bad[~bad] = np.linalg.eigvalsh(M[~bad]).min(axis=-1) <= 0
    return int(np.nonzero(used & bad)[0][0])


def test_refusals(pgo):
    g = CC.dataset(pgo, "CSAIL")                                           # EDGE2 read positionally: indefinite matrices
    n, ia, ib, meas, kind = CC.arrays(g)
    info = np.array(g.info)
    for S in (2, 16):
        with pytest.raises(pgo.PgoError) as e:
            pgo.coarsen_info_plan(n, ia, ib, meas, kind, S, info)
        assert e.value.status == NUMERIC and ("edge %d " % first_bad_used_edge(n, ia, ib, info, S)) in str(e.value)
    P, ia, ib, meas, kind = chain_graph(40, [(2, 9, 1), (2, 20, 1)])
    info = CI.random_spd_info(len(ia), 4)
    ok = pgo.coarsen_info_plan(40, ia, ib, meas, kind, 16, info)
    for e_bad, entry in ((40, np.nan), (12, np.inf), (40, -1.0)):          # a kept loop, a chain edge; NaN, inf, indefinite
        bad = info.copy()
        bad[e_bad, 3] = entry
        bad[30, 0] = -2.0                                                # a later chain edge as well: the smallest is named
        with pytest.raises(pgo.PgoError) as e:
            pgo.coarsen_info_plan(40, ia, ib, meas, kind, 16, bad)
        assert e.value.status == NUMERIC and ("edge %d " % min(e_bad, 30)) in str(e.value)
    dropped = info.copy()
    dropped[39] = [1.0, 2.0, 0, 1.0, 0, np.nan]                          # (2, 9) lies inside one segment: it may hold anything
    got = pgo.coarsen_info_plan(40, ia, ib, meas, kind, 16, dropped)
    assert got["cov"].tobytes() == ok["cov"].tobytes() and list(got["origin"]) == [-1, -1, 40]
    with pytest.raises(pgo.PgoError) as e:                               # a cap that is too small: the counts are still returned
        pgo.coarsen_info_plan(40, ia, ib, meas, kind, 4, info, edge_cap=9)
    assert e.value.status == INVALID_ARG and (e.value.n_poses, e.value.n_edges) == (10, 11)
    with pytest.raises(pgo.PgoError) as e:
        pgo.coarsen_info_plan(40, ia, ib, meas, kind, 1, info)
    assert e.value.status == INVALID_ARG
