"""pgo_pose_covariance (ceres::Covariance with a constant pose) on the GPU, against a sparse direct restatement of
(J'J)^-1 at the handle's own poses (oracle.evaluate / evaluate_sc, the constant pose removed, METHOD 2: the pose block of the
joint (poses, switches) inverse), and the properties the C-ABI promises: agreement across solver and preconditioner
variants, bitwise repeatability, an LM state left untouched, and the error statuses."""
import os

import numpy as np
import pytest

from conftest import DATA, oracle_graph

pytestmark = pytest.mark.gpu

BLOCK_REL = 1e-7     # per-block relative Frobenius error against the sparse direct inverse
RES_MAX = 1e-5      # true residual |S e - A x| / |S e| a column may end with (rtol, or the double-precision floor above it)
VARIANT = 1e-9       # agreement of two variants of the same solve, relative to the largest entry


def load(pgo, name, n_out=0, seed=1):
    g = pgo.ReadG2O(os.path.join(DATA, name + ".g2o"))
    if n_out:
        g.add_random_C(n_out, seed)
    return g


def pick(n, fixed=0, k=24):
    """first free pose, last pose, a spread in between and the constant pose"""
    idx = np.unique(np.linspace(1, n - 1, k - 1).astype(np.int64))
    return np.concatenate([[fixed], idx])


def reference_blocks(O, og, poses, idx, method, switches=None, fixed=0, info=False, cross=False):
    """Sigma's blocks at `poses` by a sparse LU of J'J (constant pose removed)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl

    N, E = og.n_poses, og.n_edges
    ia, ib = np.asarray(og.ia), np.asarray(og.ib)
    if method == 2:
        _, _, J, Js, _ = O.evaluate_sc(og, poses, switches)
    else:
        _, _, J = O.evaluate(og, poses, method=method, info_weighting=info)
    rows = np.repeat(np.arange(3 * E).reshape(E, 3), 6, axis=1).reshape(-1)
    cols = np.concatenate([3 * ia[:, None] + np.arange(3), 3 * ib[:, None] + np.arange(3)], axis=1)
    cols = np.tile(cols, (1, 3)).reshape(-1)
    Jp = sp.csr_matrix((J.reshape(-1), (rows, cols)), shape=(3 * E, 3 * N))
    if method == 2:   # switch columns of the robust edges, plus the prior rows sqrt(lambda) (1 - s)
        robust = np.nonzero(np.asarray(og.kind) != 0)[0]
        nr = robust.size
        Js_m = sp.csr_matrix((Js[robust].reshape(-1), (np.repeat(3 * robust[:, None] + np.arange(3), 1, axis=0).reshape(-1),
                                                        np.repeat(np.arange(nr), 3))), shape=(3 * E, nr))
        prior = sp.csr_matrix((-np.ones(nr), (np.arange(nr), np.arange(nr))), shape=(nr, nr))
        Jfull = sp.vstack([sp.hstack([Jp, Js_m]), sp.hstack([sp.csr_matrix((nr, 3 * N)), prior])]).tocsc()
    else:
        Jfull = Jp.tocsc()
    H = (Jfull.T @ Jfull).tocsc()
    keep = np.ones(H.shape[0], bool)
    keep[3 * fixed:3 * fixed + 3] = False
    pos = -np.ones(H.shape[0], np.int64)
    pos[keep] = np.arange(keep.sum())
    lu = spl.splu(H[keep][:, keep].tocsc())
    idx = np.asarray(idx)
    n = idx.size
    rhs = np.zeros((keep.sum(), 3 * n))
    for j, i in enumerate(idx):
        for c in range(3):
            if i != fixed:
                rhs[pos[3 * i + c], 3 * j + c] = 1.0
    X = lu.solve(rhs)
    full = np.zeros((H.shape[0], 3 * n))
    full[keep] = X
    rows3 = (3 * idx[:, None] + np.arange(3)).reshape(-1)
    M = full[rows3]            # (3n x 3n): row block a, column block b = Sigma_ab
    M = 0.5 * (M + M.T)
    if cross:
        return M
    return np.stack([M[3 * j:3 * j + 3, 3 * j:3 * j + 3] for j in range(n)])


def block_errors(got, ref):
    err = []
    for a, b in zip(got, ref):
        nb = np.linalg.norm(b)
        err.append(np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a))
    return np.array(err)


CASES = [   # (graph, outliers, method, info weighting, LM iterations before the call, options)
    ("INTEL", 50, 0, False, 5, {}),
    ("INTEL", 50, 1, False, 5, {}),
    ("INTEL", 50, 2, False, 5, {}),
    ("MIT", 0, 1, False, 5, {"block_rel": 2e-7}),   # cond(J'J) 4e10: the true residual's floor is ~2e-7
    ("MIT", 0, 2, False, 5, {}),
    ("M3500", 0, 1, False, 3, {}),
    ("FRH", 0, 1, False, 3, {}),
]


@pytest.mark.parametrize("name,n_out,method,info,iters,kw", CASES,
                         ids=["%s%s-m%d%s" % (c[0], "+%d" % c[1] if c[1] else "", c[2], "-info" if c[3] else "") for c in CASES])
def test_blocks_match_sparse_direct_inverse(pgo, oracle, name, n_out, method, info, iters, kw):
    g = load(pgo, name, n_out)
    og = oracle_graph(oracle, g)
    block_rel = kw.get("block_rel", BLOCK_REL)
    s = pgo.Solver(g, pgo.Options(method=method, max_iters=iters, info_weighting=int(info)))
    s.solve()
    poses = s.poses()
    idx = pick(g.n_poses)
    got, rep = s.covariance(idx)
    sw = s.switches() if method == 2 else None
    ref = reference_blocks(oracle, og, poses, idx, method, sw, info=info)
    err = block_errors(got[1:], ref[1:])
    assert err.max() <= block_rel, (err.max(), int(np.argmax(err)), rep)
    assert np.array_equal(got[0], np.zeros((3, 3)))   # the constant pose
    assert rep["columns"] == 3 * idx.size and rep["passes"] == (idx.size + 7) // 8
    assert rep["max_rel_residual"] <= RES_MAX and rep["pcg_iters_max"] > 0
    # every block symmetric positive definite (the constant pose aside)
    assert all(np.linalg.eigvalsh(b).min() > 0 for b in got[1:])
    s.close()


def test_information_weighting_is_refused(pgo):
    g = load(pgo, "INTEL", 50)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=2, info_weighting=1))
    s.solve()
    with pytest.raises(pgo.PgoError) as e:
        s.covariance([1])
    assert e.value.status == -8
    s.close()


def test_cross_matrix_is_symmetric_and_matches(pgo, oracle):
    g = load(pgo, "INTEL", 50)
    og = oracle_graph(oracle, g)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.solve()
    idx = np.array([0, 1, 400, 942])
    M, rep = s.covariance(idx, cross=True)
    assert M.shape == (12, 12) and np.array_equal(M, M.T)
    assert np.array_equal(M[:3], np.zeros((3, 12)))
    ref = reference_blocks(oracle, og, s.poses(), idx, 1, cross=True)
    for a in range(1, 4):
        for b in range(1, 4):
            blk, rb = M[3 * a:3 * a + 3, 3 * b:3 * b + 3], ref[3 * a:3 * a + 3, 3 * b:3 * b + 3]
            assert np.linalg.norm(blk - rb) <= BLOCK_REL * np.linalg.norm(ref[3 * a:3 * a + 3, 3 * a:3 * a + 3]), (a, b)
    diag, _ = s.covariance(idx)
    for a in range(4):
        assert np.abs(M[3 * a:3 * a + 3, 3 * a:3 * a + 3] - diag[a]).max() <= VARIANT * np.abs(diag).max()
    s.close()


def _cov(pgo, g, idx, knobs=(), **opt):
    for k, v in knobs:
        pgo.set_knob(k, v)
    try:
        s = pgo.Solver(g, pgo.Options(method=1, max_iters=4, **opt))
        s.solve()
        c, rep = s.covariance(idx)
        s.close()
    finally:
        for k, _ in knobs:
            pgo.set_knob(k, -1)
    return c, rep


def test_variants_agree(pgo):
    """one system, several solver paths: the direct vs the PCG handle, with and without the coarse level, the product kernel
    layouts and the number of poses per pass"""
    g = load(pgo, "INTEL", 50)
    idx = pick(g.n_poses, k=17)
    base, _ = _cov(pgo, g, idx, linear_solver=1)
    scale = np.abs(base).max()
    others = [
        _cov(pgo, g, idx, linear_solver=2)[0],
        _cov(pgo, g, idx, linear_solver=1, pcg_coarse_poses=0)[0],
        _cov(pgo, g, idx, knobs=[("pad_tiles", 1)], linear_solver=1)[0],
        _cov(pgo, g, idx, knobs=[("spmv_pipe", 0)], linear_solver=1)[0],
        _cov(pgo, g, idx, knobs=[("spmv_pipe", 2)], linear_solver=1)[0],
        _cov(pgo, g, idx, knobs=[("cov_poses_per_pass", 1)], linear_solver=1)[0],
        _cov(pgo, g, idx, knobs=[("cov_poses_per_pass", 16)], linear_solver=1)[0],
    ]
    for k, o in enumerate(others):
        assert np.abs(o - base).max() <= VARIANT * scale, (k, np.abs(o - base).max() / scale)


def test_repeat_is_bitwise(pgo):
    g = load(pgo, "M3500")
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=2))
    s.solve()
    idx = pick(g.n_poses, k=10)
    a, ra = s.covariance(idx)
    b, rb = s.covariance(idx)
    assert np.array_equal(a, b) and ra["pcg_iters_total"] == rb["pcg_iters_total"]
    s.close()


def _records(s):
    return [{k: v for k, v in r.items() if k != "seconds"} for r in s.iter_records()]


@pytest.mark.parametrize("name,n_out,method,opts", [("INTEL", 50, 1, {}), ("INTEL", 50, 2, {}), ("M3500", 0, 1, {}),
                                                    ("M3500", 0, 1, {"pcg_rtol": 0.1})],
                         ids=["INTEL+50-m1", "INTEL+50-m2", "M3500-m1", "M3500-m1-inexact"])
def test_lm_state_is_untouched(pgo, name, n_out, method, opts):
    g = load(pgo, name, n_out)
    o = dict(method=method, max_iters=12, **opts)
    ref = pgo.Solver(g, pgo.Options(**o))
    ref.lm_begin()
    ref.lm_step(5)
    ref.lm_step(100)
    s = pgo.Solver(g, pgo.Options(**o))
    s.lm_begin()
    s.lm_step(5)
    s.covariance(pick(g.n_poses, k=9))
    s.lm_step(100)
    assert np.array_equal(s.poses(), ref.poses())
    assert _records(s) == _records(ref)
    s.close()
    ref.close()


def test_large_synthetic_graph(pgo):
    """100k poses, the inexact-mode handle (created without the coarse level: the call builds it) after 5 LM iterations,
    8 poses: every column's TRUE residual |S e - A x| / |S e| is within the tolerance, the blocks are symmetric positive
    definite"""
    g = pgo.synth_manhattan(100000, 4.0, 0.1, 7)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5, pcg_rtol=0.1))
    assert s.info().pcg_coarse_poses == 0
    s.solve()
    idx = np.array([1, 17, 5000, 33333, 50001, 77777, 90000, 99999])
    M, rep = s.covariance(idx, cross=True)
    assert np.array_equal(M, M.T)
    assert all(np.linalg.eigvalsh(M[3 * j:3 * j + 3, 3 * j:3 * j + 3]).min() > 0 for j in range(idx.size))
    assert rep["max_rel_residual"] <= RES_MAX and rep["passes"] == 1, rep
    assert s.info().pcg_coarse_poses == 0   # (the LM loop still runs on one level)
    s.close()


def test_errors(pgo):
    g = load(pgo, "INTEL")
    s = pgo.Solver(g, pgo.Options(method=1, fixed_pose=-1, max_iters=1))
    with pytest.raises(pgo.PgoError) as e:
        s.covariance([1, 2])
    assert e.value.status == -8
    s.close()
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=1))
    with pytest.raises(pgo.PgoError) as e:
        s.covariance([1, g.n_poses])
    assert e.value.status == -1
    with pytest.raises(pgo.PgoError) as e:
        s.covariance([-1])
    assert e.value.status == -1
    bad = s.poses()
    bad[77, 2] = np.nan
    s.set_poses(bad)
    with pytest.raises(pgo.PgoError) as e:
        s.covariance([3])
    assert e.value.status == -7 and "pose 77" in str(e.value)
    s.close()
    # an isolated pose: INTEL with one more pose that no edge touches
    poses = np.vstack([np.array(g.poses), [[1.0, 2.0, 0.3]]])
    h = pgo.Graph.from_arrays(poses, np.array(g.ia), np.array(g.ib), np.array(g.meas), np.array(g.kind))
    s = pgo.Solver(h, pgo.Options(method=1, max_iters=1, linear_solver=1))
    with pytest.raises(pgo.PgoError) as e:
        s.covariance([5])
    assert e.value.status == -7 and ("pose %d" % g.n_poses) in str(e.value)
    s.close()
