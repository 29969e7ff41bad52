"""The restatement of the PCG preconditioners (oracle.Precond) against its definition, on the CPU: for every family the
explicitly formed dense M (written out block by block here, independently of the sparse masks the restatement uses) and
np.linalg.solve must give the same z = M^-1 r.  The GPU tests (test_gpu_precond.py) judge the HIP kernels by this
restatement, so it has to be right first.  Small graphs (<= 300 poses): ragged last groups / segments / aggregates, a
constant pose inside a group, none at all, duplicate edges, a closure between consecutive poses, an unjoined consecutive
pair and edge-less poses that make whole aggregates dead."""
import os

import numpy as np
import pytest

from conftest import DATA


def small_graph(O, n=230, n_free=0):
    """the first n poses of MIT and the edges among them, made awkward: the odometry edge 40-41 removed, 10-11 tripled,
    a closure-kind edge 60-61, and n_free edge-less poses appended"""
    g = O.read_g2o(os.path.join(DATA, "MIT.g2o"))
    keep = (g.ia < n) & (g.ib < n) & ~((g.ia == 40) & (g.ib == 41))
    ia, ib, meas, info, kind = g.ia[keep], g.ib[keep], g.meas[keep], g.info[keep], g.kind[keep]
    k10 = np.nonzero((ia == 10) & (ib == 11))[0][:1]
    k60 = np.nonzero((ia == 60) & (ib == 61))[0][:1]
    ia = np.concatenate([ia, ia[k10], ia[k10], ia[k60]]).astype(np.int32)
    ib = np.concatenate([ib, ib[k10], ib[k10], ib[k60]]).astype(np.int32)
    meas = np.concatenate([meas, meas[k10] * 1.01, meas[k10] * 0.99, meas[k60] + 0.02])
    info = np.concatenate([info, info[k10], info[k10], info[k60]])
    kind = np.concatenate([kind, kind[k10], kind[k10], np.ones(1, np.uint8)]).astype(np.uint8)
    poses = np.array(g.poses[:n])
    if n_free:
        poses = np.concatenate([poses, poses[-1] + np.arange(1, n_free + 1)[:, None] * np.array([0.5, 0.25, 0.0])])
    return O.Graph(np.arange(len(poses), dtype=np.int32), poses, ia, ib, meas, info, kind)


def state(O, g, fixed_pose, radius=1e3, seed=0):
    rng = np.random.default_rng(seed)
    x = np.array(g.poses) + 0.01 * rng.standard_normal(g.poses.shape)
    return x, O.lm_system(g, x, g.poses, radius, method=1, fixed_pose=fixed_pose)


def dense_A(sysm, perm):
    N3 = len(sysm.d2)
    A = sysm.H.toarray() + np.diag(sysm.d2)
    q = (3 * np.asarray(perm)[:, None] + np.arange(3)).reshape(-1)
    Ai = np.zeros_like(A)
    Ai[np.ix_(q, q)] = A
    assert Ai.shape == (N3, N3)
    return Ai, q


def dense_m1(A, block_poses, chain_len):
    N = A.shape[0] // 3
    M = np.zeros_like(A)
    if chain_len:
        for i in range(N):
            for j in (i - 1, i, i + 1):
                if 0 <= j < N and i // chain_len == j // chain_len:
                    M[3 * i:3 * i + 3, 3 * j:3 * j + 3] = A[3 * i:3 * i + 3, 3 * j:3 * j + 3]
    else:
        for g0 in range(0, N, block_poses):
            sl = slice(3 * g0, 3 * min(N, g0 + block_poses))
            M[sl, sl] = A[sl, sl]
    return M


def dense_p(xi, s, in_graph, agg):
    N = len(xi)
    na = (N + agg - 1) // agg
    P = np.zeros((3 * N, 3 * na))
    for a in range(na):
        idx = range(a * agg, min(N, (a + 1) * agg))
        c = xi[list(idx), :2].mean(axis=0)
        for i in idx:
            if not in_graph[i]:
                continue
            B = np.array([[1.0, 0.0, -(xi[i, 1] - c[1])], [0.0, 1.0, xi[i, 0] - c[0]], [0.0, 0.0, 1.0]])
            for k in range(3):
                if s[3 * i + k] > 0:
                    P[3 * i + k, 3 * a:3 * a + 3] = B[k] / s[3 * i + k]
    return P


@pytest.mark.parametrize("fixed_pose", [17, -1])
@pytest.mark.parametrize("family", [dict(block_poses=1), dict(block_poses=32), dict(block_poses=7), dict(chain_len=8),
                                    dict(chain_len=64), dict(block_poses=32, coarse_poses=16),
                                    dict(block_poses=32, coarse_poses=20), dict(chain_len=8, coarse_poses=16)])
@pytest.mark.parametrize("permuted", [False, True])
def test_restatement_matches_the_dense_definition(oracle, family, fixed_pose, permuted):
    O = oracle
    g = small_graph(O, 230, n_free=40 if family.get("coarse_poses") == 16 else 0)   # 270 poses: aggregates 15, 16 dead
    N = g.n_poses
    x, sysm = state(O, g, fixed_pose)
    perm = np.random.default_rng(1).permutation(N) if permuted else np.arange(N)
    M = O.Precond(sysm, x, perm=perm, **family)
    A, q = dense_A(sysm, perm)
    np.testing.assert_array_equal(M.to_internal(np.arange(3 * N)), np.argsort(q))
    assert abs(M.A.toarray() - A).max() == 0.0
    M1 = dense_m1(A, family.get("block_poses", 1), family.get("chain_len", 0))
    rng = np.random.default_rng(2)
    R = rng.standard_normal((3 * N, 3))
    Z1 = np.linalg.solve(M1, R)
    Z = Z1.copy()
    if family.get("coarse_poses"):
        xi = np.empty_like(x)
        xi[perm] = x
        s = sysm.s[M.qinv]
        in_graph = np.array([np.any(sysm.H.toarray()[3 * i:3 * i + 3, :] != 0) for i in range(N)])[np.argsort(perm)]
        P = dense_p(xi, s, in_graph, family["coarse_poses"])
        np.testing.assert_allclose(M.P.toarray(), P, rtol=1e-15, atol=0)
        Ac = P.T @ A @ P
        dead = np.all(P == 0.0, axis=0)
        Ac[dead, dead] = 1.0
        Z += P @ np.linalg.solve(Ac, P.T @ R)
        assert M.n_dead == int(dead.reshape(-1, 3).all(axis=1).sum()) == (2 if N == 270 and not permuted else 0)
    for k in range(R.shape[1]):
        z1, z = M.apply1(R[:, k]), M.apply(R[:, k])
        assert np.abs(z1 - Z1[:, k]).max() <= 1e-9 * np.abs(Z1[:, k]).max()
        assert np.abs(z - Z[:, k]).max() <= 1e-9 * np.abs(Z[:, k]).max()
    # the one-level matrix is the SPD block-diagonal part it claims to be, and nothing else
    assert abs(M.M1.toarray() - M1).max() == 0.0
    assert np.all(np.linalg.eigvalsh(M1) > 0)


def test_pcg_iterations_solves_the_lm_system(oracle):
    """pcg_iterations (built on lm_system / Precond) returns a solution of the system to its tolerance"""
    O = oracle
    g = small_graph(O, 230)
    x, sysm = state(O, g, 0, radius=1e4)
    A = sysm.H + np.diag(sysm.d2)
    for coarse in (0, 16):
        k, y = O.pcg_iterations(g, x, g.poses, 1e4, method=1, rtol=1e-10, block_poses=32, coarse_poses=coarse)
        assert 0 < k < 2000
        assert np.linalg.norm(A @ y - sysm.b) <= 1.01e-10 * np.linalg.norm(sysm.b)
