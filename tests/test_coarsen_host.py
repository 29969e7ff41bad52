"""pgo_coarsen_plan and pgo_prolong_eval (include/pgo.h, "hierarchical initialisation"; host only) against the numpy
restatement of tests/_coarsen_cases.py: structure exactly, measurements and poses to the bounds derived there."""
import numpy as np
import pytest

import _coarsen_cases as CC

INVALID_ARG, NUMERIC, UNSUPPORTED = -1, -7, -8


def plan(pgo, n, ia, ib, meas, kind, S, **kw):
    return pgo.coarsen_plan(n, ia, ib, meas, kind, S, **kw)


def check_against_restatement(pgo, n, ia, ib, meas, kind, S, X=None):
    got, want = plan(pgo, n, ia, ib, meas, kind, S), CC.restate_coarsen(n, ia, ib, meas, kind, S)
    CC.assert_same_structure(got, want)
    tol_xy, tol_th = CC.bounds(n, ia, ib, meas, S)
    for k in ("meas", "C", "Cend"):
        CC.assert_close_poses(got[k], want[k], tol_xy, tol_th, "S=%d %s" % (S, k))
    assert not got["C"][::S].any()                                  # C_{kS} is the identity, exactly
    assert np.abs(got["meas"][:, 2]).max() <= np.pi
    K = got["n_poses"]
    if X is None:
        X = np.random.default_rng(S).normal(0, 5, (K, 3))
    tol_xy, tol_th = CC.bounds(n, ia, ib, meas, S, X)
    P = pgo.prolong_eval(n, S, got["C"], got["Cend"], X)
    CC.assert_close_poses(P, CC.restate_prolong(n, S, want["C"], want["Cend"], X), tol_xy, tol_th, "S=%d prolong" % S)
    assert P[::S].tobytes() == np.ascontiguousarray(X).tobytes()      # key poses come back bitwise
    return got


@pytest.mark.parametrize("S", CC.STRIDES)
@pytest.mark.parametrize("name", ["synth600", "intel50"])
def test_plan_and_prolongation_are_the_restatement(pgo, name, S):
    g = getattr(CC, name)(pgo)
    n, ia, ib, meas, kind = CC.arrays(g)
    got = check_against_restatement(pgo, n, ia, ib, meas, kind, S)
    assert got["n_poses"] == -(-n // S) and (got["origin"][:got["n_poses"] - 1] == -1).all()
    assert (np.diff(got["origin"][got["n_poses"] - 1:]) > 0).all()      # the caller's edge order, stable


@pytest.mark.parametrize("S", [2, 16, 64, 65])
def test_known_answer(pgo, S):
    """measurements that are the exact relatives of a pose set P: every coarse measurement is the relative of its key poses,
    and the key poses of P prolong to P.  On top of the bounds of _coarsen_cases.bounds: every measurement carries the rounding
    of its own evaluation, <= 4 eps |m| (P is exact by definition), which a composite sums over its segment (<= 4 eps L) and
    the relative of the key poses has once more; L and |relative| are below the largest coordinate difference R of P."""
    n = 403
    P, ia, ib, meas, kind = CC.exact_graph(n, 60, seed=11)
    got = plan(pgo, n, ia, ib, meas, kind, S)
    key = P[::S]
    R = np.ptp(P[:, :2], axis=0).max() * np.sqrt(2)
    tol_xy, tol_th = CC.bounds(n, ia, ib, meas, S, key)
    tol_xy += 8 * CC.EPS * (S + 1) * R
    tol_th += 8 * CC.EPS * (np.abs(P[:, 2]).max() + np.pi)
    CC.assert_close_poses(got["meas"], CC.relative(key[got["ia"]], key[got["ib"]]), tol_xy, tol_th, "coarse measurements")
    CC.assert_close_poses(pgo.prolong_eval(n, S, got["C"], got["Cend"], key), P, tol_xy, tol_th, "prolonged key poses")


def chain_graph(n, extra=()):
    """a straight chain of unit steps plus the edges of `extra` = (a, b, kind), measurements the exact relatives"""
    P = np.stack([np.arange(n, dtype=float), np.zeros(n), np.zeros(n)], -1)
    ia = np.concatenate([np.arange(n - 1), [e[0] for e in extra]]).astype(np.int32)
    ib = np.concatenate([np.arange(1, n), [e[1] for e in extra]]).astype(np.int32)
    kind = np.concatenate([np.zeros(n - 1), [e[2] for e in extra]]).astype(np.uint8)
    return P, ia, ib, CC.relative(P[ia], P[ib]), kind


def test_two_key_poses_and_a_last_segment_of_one_pose(pgo):
    S = 16
    P, ia, ib, meas, kind = chain_graph(S + 1, [(0, S, 1)])
    got = check_against_restatement(pgo, S + 1, ia, ib, meas, kind, S)
    assert got["n_poses"] == 2 and list(got["origin"]) == [-1, S] and got["Cend"].shape == (1, 3)
    assert np.array_equal(got["meas"], [[S, 0, 0], [S, 0, 0]])


def test_n_a_multiple_of_the_stride(pgo):
    S, n = 7, 70
    P, ia, ib, meas, kind = chain_graph(n, [(3, 66, 1)])
    got = check_against_restatement(pgo, n, ia, ib, meas, kind, S)
    assert got["n_poses"] == 10 and len(got["ia"]) == 10 and got["Cend"].shape == (9, 3)
    assert (got["ia"][-1], got["ib"][-1]) == (0, 9) and np.array_equal(got["meas"][-1], [63, 0, 0])


def test_a_loop_that_runs_backwards(pgo):
    g = CC.dataset(pgo, "MIT")
    n, ia, ib, meas, kind = CC.arrays(g)
    chain, _ = CC.chain_edges(n, ia, ib)
    back = np.nonzero((ia > ib) & ~np.isin(np.arange(len(ia)), chain))[0]
    assert len(back) == 20
    got = check_against_restatement(pgo, n, ia, ib, meas, kind, 16)
    sel = np.isin(got["origin"], back)
    assert sel.sum() == (ia[back] // 16 != ib[back] // 16).sum() > 0 and (got["ia"][sel] >= got["ib"][sel]).all()


def test_a_duplicate_edge(pgo):
    """CSAIL lists the loop (323, 855) twice: both copies are carried, parallel coarse edges are not merged"""
    g = CC.dataset(pgo, "CSAIL")
    n, ia, ib, meas, kind = CC.arrays(g)
    dup = np.nonzero((np.minimum(ia, ib) == 323) & (np.maximum(ia, ib) == 855))[0]
    assert len(dup) == 2
    for S in (2, 16):
        got = check_against_restatement(pgo, n, ia, ib, meas, kind, S)
        sel = np.isin(got["origin"], dup)
        assert sel.sum() == 2 and len(set(zip(got["ia"][sel], got["ib"][sel]))) == 1
    # a second edge between consecutive poses: the first copy is the chain edge, the others are edges like any other, carried
    # next to the composite when they straddle a segment boundary
    P, ia, ib, meas, kind = chain_graph(40, [(15, 16, 0), (16, 15, 0)])
    got = check_against_restatement(pgo, 40, ia, ib, meas, kind, 16)
    assert list(got["origin"]) == [-1, -1, 39, 40] and list(got["ia"][2:]) == [0, 1] and list(got["ib"][2:]) == [1, 0]
    assert np.array_equal(got["meas"][2], [16, 0, 0]) and np.array_equal(got["meas"][3], [-16, 0, 0])


def test_an_edge_inside_one_segment_is_dropped(pgo):
    P, ia, ib, meas, kind = chain_graph(40, [(2, 9, 1), (17, 30, 2), (2, 20, 2)])
    got = check_against_restatement(pgo, 40, ia, ib, meas, kind, 16)
    assert list(got["origin"]) == [-1, -1, 41] and got["kind"][-1] == 2


def test_refusals(pgo):
    P, ia, ib, meas, kind = chain_graph(40, [(2, 20, 1)])
    with pytest.raises(pgo.PgoError) as e:                         # a missing chain pair, named
        plan(pgo, 40, np.delete(ia, [7, 12]), np.delete(ib, [7, 12]), np.delete(meas, [7, 12], 0), np.delete(kind, [7, 12]), 4)
    assert e.value.status == UNSUPPORTED and "poses 7 and 8" in str(e.value)
    for n, S in ((16, 16), (5, 16), (40, 1), (40, 257), (40, 0)):
        with pytest.raises(pgo.PgoError) as e:
            plan(pgo, n, ia[:n - 1], ib[:n - 1], meas[:n - 1], kind[:n - 1], S)
        assert e.value.status == INVALID_ARG
        with pytest.raises(pgo.PgoError) as e:
            pgo.prolong_eval(n, S, np.zeros((n, 3)), np.zeros((1, 3)), np.zeros((2, 3)))
        assert e.value.status == INVALID_ARG
    bad = meas.copy()
    bad[[30, 11], [0, 2]] = [np.inf, np.nan]
    with pytest.raises(pgo.PgoError) as e:
        plan(pgo, 40, ia, ib, bad, kind, 4)
    assert e.value.status == NUMERIC and "edge 11 " in str(e.value)
    with pytest.raises(pgo.PgoError) as e:                         # a cap that is too small: the counts are still returned
        plan(pgo, 40, ia, ib, meas, kind, 4, edge_cap=9)
    assert e.value.status == INVALID_ARG and (e.value.n_poses, e.value.n_edges) == (10, 10)
    assert len(plan(pgo, 40, ia, ib, meas, kind, 4, edge_cap=10)["ia"]) == 10
    assert len(plan(pgo, 256 + 1, *chain_graph(257)[1:], 256)["ia"]) == 1      # the largest stride
