"""Shared by test_coarsen_host.py, test_coarsen_native.py and test_gpu_coarsen.py: the coarsening and the prolongation of
include/pgo.h ("hierarchical initialisation") restated in numpy from the definitions -- rotations from the angle at every
composition, left to right --, the graphs the tests run on, and the error bounds of the comparisons."""
import os

import numpy as np

from conftest import DATA

EPS = np.finfo(np.float64).eps
STRIDES = (2, 7, 16, 64, 65, 256)


def wrap(a):
    return np.arctan2(np.sin(a), np.cos(a))


def compose(A, B):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    c, s = np.cos(A[..., 2]), np.sin(A[..., 2])
    return np.stack([A[..., 0] + c * B[..., 0] - s * B[..., 1], A[..., 1] + s * B[..., 0] + c * B[..., 1], A[..., 2] + B[..., 2]], -1)


def inverse(A):
    A = np.asarray(A, np.float64)
    c, s = np.cos(A[..., 2]), np.sin(A[..., 2])
    return np.stack([-(c * A[..., 0] + s * A[..., 1]), -(-s * A[..., 0] + c * A[..., 1]), -A[..., 2]], -1)


def relative(Pa, Pb):
    """the measurement of an edge (a, b) that the poses satisfy exactly: Pa^-1 o Pb, angle not wrapped"""
    return compose(inverse(Pa), Pb)


def chain_edges(n, ia, ib):
    """chain[i] = the first edge joining i and i + 1 in either orientation; the first pair without one (or -1)"""
    chain = np.full(n, -1, np.int64)
    for e, (a, b) in enumerate(zip(ia, ib)):
        lo, hi = min(a, b), max(a, b)
        if hi == lo + 1 and chain[lo] < 0:
            chain[lo] = e
    gaps = np.nonzero(chain[:n - 1] < 0)[0]
    return chain, (int(gaps[0]) if len(gaps) else -1)


def restate_coarsen(n, ia, ib, meas, kind, S):
    """the dict pgo.coarsen_plan returns"""
    ia, ib, meas, kind = np.asarray(ia), np.asarray(ib), np.asarray(meas, np.float64).reshape(-1, 3), np.asarray(kind)
    chain, gap = chain_edges(n, ia, ib)
    assert gap < 0
    K = -(-n // S)
    Z = np.array([meas[chain[i]] if ia[chain[i]] == i else inverse(meas[chain[i]]) for i in range(n - 1)]).reshape(-1, 3)
    Cc, Cend = np.zeros((n, 3)), np.zeros((K - 1, 3))
    for i in range(n):
        if i % S:
            Cc[i] = compose(Cc[i - 1], Z[i - 1])
    for k in range(K - 1):
        Cend[k] = compose(Cc[(k + 1) * S - 1], Z[(k + 1) * S - 1])
    is_chain = np.zeros(len(ia), bool)
    is_chain[chain[:n - 1]] = True
    keep = np.nonzero(~is_chain & (ia // S != ib // S))[0]
    tm = compose(compose(Cc[ia[keep]], meas[keep]), inverse(Cc[ib[keep]])) if len(keep) else np.zeros((0, 3))
    cm = np.concatenate([Cend, tm])
    cm[:, 2] = wrap(cm[:, 2])
    return {"n_poses": K, "ia": np.concatenate([np.arange(K - 1), ia[keep] // S]).astype(np.int32),
            "ib": np.concatenate([np.arange(1, K), ib[keep] // S]).astype(np.int32), "meas": cm,
            "kind": np.concatenate([np.zeros(K - 1, np.uint8), kind[keep].astype(np.uint8)]),
            "origin": np.concatenate([np.full(K - 1, -1), keep]).astype(np.int32), "C": Cc, "Cend": Cend}


def restate_prolong(n, S, Cc, Cend, X):
    X = np.asarray(X, np.float64).reshape(-1, 3)
    K = -(-n // S)
    out = np.zeros((n, 3))
    for i in range(n):
        k = i // S
        t = (i - k * S) / S
        if i == k * S:
            out[i] = X[k]
            continue
        F = compose(X[k], Cc[i])
        if k < K - 1:
            B = compose(compose(X[k + 1], inverse(Cend[k])), Cc[i])
            out[i] = [(1 - t) * F[0] + t * B[0], (1 - t) * F[1] + t * B[1], F[2] + t * wrap(B[2] - F[2])]
        else:
            out[i] = F
    return out


def bounds(n, ia, ib, meas, S, X=None):
    """(tol_xy, tol_theta) for two evaluations of the coarse measurements that differ in rounding and association only, and
    -- with the coarse poses X -- of the prolongation.  Derived, with eps the unit roundoff spacing, L = the longest path length of
    a segment (sum of the |translation| of its chain motions: every |C_i| is below it), Th = the largest sum of |theta| along
    a segment and M = the largest |translation| of a measurement:
      * the angle of a composite is a sum of at most S terms, each partial sum below Th: error <= S eps Th; its rotation, from
        one sincos (<= 2 eps) or from S products of carried (cos, sin) pairs (<= 4 eps each): at most S (Th + 4) eps =: A;
      * each of the S compositions rounds a translation below L three times (<= 3 eps L), and the rotation error A turns what
        follows, also below L: a composite's translation is good to S (Th + 7) eps L;
      * C_a o m o C_b^-1 adds the two composites' errors, turns m and C_b by A, and rounds sums below 2 L + M eight times:
        (S (Th + 7) + 8) eps (2 L + M) per evaluation; two evaluations, and a factor 2 for the products' second-order terms:
        tol_xy = 4 (S (Th + 7) + 8) eps (2 L + M);
      * theta = th_a + m_th - th_b, wrapped: three sums of S terms and the wrap's sincos / atan2 (<= 4 eps pi):
        tol_theta = 2 (2 S + 4) eps (2 Th + 2 pi), compared modulo 2 pi.
    The prolongation composes X_k (and X_{k+1} o Cend^-1) with C_i and blends: the same composites' errors, plus roundings of
    sums below |X| + 2 L (16 of them), plus the angle error of X_{k+1} o Cend^-1 turning C_i: tol_xy + 16 eps (Xmax + 2 L) + A L,
    which tol_xy's S (Th + 7) eps L already contains; theta likewise with 8 eps (|X_th| + Th + pi)."""
    ia, ib, meas = np.asarray(ia), np.asarray(ib), np.asarray(meas, np.float64).reshape(-1, 3)
    chain, gap = chain_edges(n, ia, ib)
    assert gap < 0
    step = np.hypot(meas[chain[:n - 1], 0], meas[chain[:n - 1], 1])
    turn = np.abs(meas[chain[:n - 1], 2])
    K = -(-n // S)
    L = max(step[k * S:(k + 1) * S].sum() for k in range(K))
    Th = max(turn[k * S:(k + 1) * S].sum() for k in range(K))
    M = np.hypot(meas[:, 0], meas[:, 1]).max()
    tol_xy = 4 * (S * (Th + 7) + 8) * EPS * (2 * L + M)
    tol_th = 2 * (2 * S + 4) * EPS * (2 * Th + 2 * np.pi)
    if X is not None:
        X = np.asarray(X, np.float64).reshape(-1, 3)
        tol_xy += 16 * EPS * (np.abs(X[:, :2]).max() + 2 * L)
        tol_th += 8 * EPS * (np.abs(X[:, 2]).max() + Th + np.pi)
    return tol_xy, tol_th


def assert_same_structure(got, want):
    assert got["n_poses"] == want["n_poses"]
    for k in ("ia", "ib", "kind", "origin"):
        assert np.array_equal(got[k], want[k]), k


def assert_close_poses(got, want, tol_xy, tol_th, what=""):
    got, want = np.asarray(got).reshape(-1, 3), np.asarray(want).reshape(-1, 3)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not len(got):
        return
    dxy, dth = np.abs(got[:, :2] - want[:, :2]).max(), np.abs(wrap(got[:, 2] - want[:, 2])).max()
    print("%s: max |dxy| %.3e (bound %.3e), max |dtheta| %.3e (bound %.3e)" % (what, dxy, tol_xy, dth, tol_th))
    assert dxy <= tol_xy and dth <= tol_th, (what, dxy, tol_xy, dth, tol_th)


def arrays(g):
    return g.n_poses, np.array(g.ia), np.array(g.ib), np.array(g.meas), np.array(g.kind)


def synth600(pgo):
    return pgo.synth_manhattan(600, 4.0, 0.1, 3)


def intel50(pgo):
    g = pgo.ReadG2O(os.path.join(DATA, "INTEL.g2o"))
    g.add_random_C(50, 1)
    return g


def dataset(pgo, name):
    return pgo.ReadG2O(os.path.join(DATA, name + ".g2o"))


def exact_graph(n, n_loops, seed):
    """poses P on a smooth random walk (angles not wrapped) and a graph whose measurements are their exact relatives: the chain,
    with every fifth edge stored reversed, and n_loops loops in both orientations"""
    rng = np.random.default_rng(seed)
    th = np.cumsum(rng.normal(0, 0.2, n))
    P = np.stack([np.cumsum(np.cos(th)), np.cumsum(np.sin(th)), th], -1)
    P -= P[0]
    i = np.arange(n - 1)
    rev = i % 5 == 4
    ia, ib = np.where(rev, i + 1, i), np.where(rev, i, i + 1)
    la, lb = rng.integers(0, n, n_loops), rng.integers(0, n, n_loops)
    ok = np.abs(la - lb) > 1
    ia, ib = np.concatenate([ia, la[ok]]).astype(np.int32), np.concatenate([ib, lb[ok]]).astype(np.int32)
    kind = np.concatenate([np.zeros(n - 1, np.uint8), np.ones(int(ok.sum()), np.uint8)])
    return P, ia, ib, relative(P[ia], P[ib]), kind
