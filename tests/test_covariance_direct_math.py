"""CPU restatement (numpy) of pgo_pose_covariance with solver = 1: the columns of Sigma = S (S J'J S + I_fixed)^-1 S through the
direct solve's algebra at D'D = 0 --

    A = T + V'V,   Z = T^-1 V',   C = I + V Z = L L',   X0 = T^-1 B,   X = X0 - Z C^-1 V X0,   refinement against A

-- with the chain split direct_setup() makes, the block LDL' recurrence of T and LAPACK's Cholesky of C
(_direct_restatement.restate), on the oracle's system (oracle.lm_system at radius = infinity: D'D = 0, identity rows on the
constant pose).  Without damping T must be positive definite on its own (the smallest eigenvalue over all pivots S_i of
its block LDL' is printed), and 24 diagonal blocks must meet the bound tests/test_gpu_covariance.py sets against the sparse
direct inverse, with ONE refinement step: what tests/test_gpu_covariance_direct.py asks of the GPU is reachable by the method.

The state of the system.  The cases (INTEL + 50 with METHOD 1, MIT with METHOD 0) are taken where
tests/test_direct_solve_math.py, the restatement of the LM solve, takes the oracle's system: at the graph's own poses, LM
iteration 1 (what a handle has when the call comes before any solve).  INTEL + 50 is checked after five LM iterations of the
oracle as well, the state of the GPU tests.  MIT with METHOD 0 after five iterations is a test of its own, because there the
method reaches its limit: 2.3e-6 with one refinement step against BLOCK_REL = 1e-7.  Without a robust loss the 20
closures enter V with full weight against an undamped chain of 808 poses whose Jacobi scales stem from the first iteration:
cond(I + V Z) = 3e5, cond(T) = 2.8e12, cond(A) = 1.7e11 (at the graph's poses: 9e2, 5.9e10, 5.1e9).  The true residual per
refinement step is 11 (none), 1.5, 4.7e-3, 1.7e-4, 2.3e-6, the block error 1.3e-5, 2.3e-6, 4.3e-7, 3.5e-7, 2.8e-7.
test_mit_method0_after_lm_is_at_the_methods_limit asserts what the library's rule promises there (every step lowers a
column's residual by 10 % or more while it is above rtol, and the mandatory step plus three more end within RES_MAX, the
acceptance threshold) and prints the block error, which stays a factor 3 above BLOCK_REL: solver = 0 is the path for such
a system."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from _direct_restatement import _chain_split, _factor, restate
from conftest import DATA
from test_gpu_covariance import BLOCK_REL, RES_MAX, block_errors, pick, reference_blocks

RTOL = 1e-10   # pgo_covariance_options_default


def _setup(oracle, name, n_out, method, lm_iters):
    """graph, poses, the undamped system there, the 24 picked poses and their right-hand sides S e_k"""
    g = oracle.read_g2o(os.path.join(DATA, name + ".g2o"))
    if n_out:
        g = oracle.add_random_C(g, n_out, 1)
    poses0 = np.array(g.poses)
    poses = oracle.lm_direct(g, oracle.Options(method=method, max_iters=lm_iters)).poses if lm_iters else poses0
    sysm = oracle.lm_system(g, poses, poses0, np.inf, method=method)
    assert not sysm.d2[3:].any() and np.array_equal(sysm.d2[:3], np.ones(3))   # D'D = 0, identity rows on the constant pose
    idx = pick(g.n_poses)
    B = np.zeros((3 * g.n_poses, 3 * idx.size))
    for j, i in enumerate(idx):
        for c in range(3):
            B[3 * i + c, 3 * j + c] = sysm.s[3 * i + c]          # S e_k (zero on the constant pose)
    return g, poses, sysm, idx, B


def _smallest_pivot(g, sysm):
    """the chain alone, undamped: the smallest eigenvalue over the pivots S_i of its block LDL'"""
    rows_c = np.repeat(_chain_split(g), 3)
    Ac = sysm.JS.tocsr()[rows_c]
    T = (Ac.T @ Ac + sp.diags(sysm.d2)).tocsr()
    _, Sinv = _factor(T)
    ev = [np.linalg.eigvalsh(0.5 * (Si + Si.T)) for Si in Sinv]
    assert all(e.min() > 0.0 for e in ev)
    return min(1.0 / e.max() for e in ev)


def _residuals(sysm, B, X):
    A = (sysm.H + sp.diags(sysm.d2)).tocsr()
    nb = np.linalg.norm(B, axis=0)
    return np.linalg.norm(B - A @ X, axis=0)[nb > 0] / nb[nb > 0]


def _blocks(sysm, idx, X):
    M = (sysm.s[:, None] * X)[(3 * idx[:, None] + np.arange(3)).reshape(-1)]   # Sigma's columns, the picked rows
    M = 0.5 * (M + M.T)
    return np.stack([M[3 * j:3 * j + 3, 3 * j:3 * j + 3] for j in range(idx.size)])


CASES = [("INTEL", 50, 1, 0), ("MIT", 0, 0, 0), ("INTEL", 50, 1, 5)]


@pytest.mark.parametrize("name,n_out,method,lm_iters", CASES, ids=["INTEL+50-m1", "MIT-m0", "INTEL+50-m1-after-5-iterations"])
def test_direct_algebra_gives_the_covariance_blocks(oracle, name, n_out, method, lm_iters):
    g, poses, sysm, idx, B = _setup(oracle, name, n_out, method, lm_iters)
    piv = _smallest_pivot(g, sysm)
    X = restate(sysm, g, 0, B, 1)
    res = _residuals(sysm, B, X)
    got = _blocks(sysm, idx, X)
    err = block_errors(got[1:], reference_blocks(oracle, g, poses, idx, method)[1:])
    print(f"{name}+{n_out} METHOD {method} after {lm_iters} LM iterations: smallest pivot eigenvalue of T {piv:.3e}, true residual "
          f"after one refinement step {res.max():.2e}, largest block error against the sparse direct inverse {err.max():.2e}")
    assert piv > 0.0
    assert np.array_equal(got[0], np.zeros((3, 3)))
    assert err.max() <= BLOCK_REL, (err.max(), int(np.argmax(err)))


def test_mit_method0_after_lm_is_at_the_methods_limit(oracle):
    g, poses, sysm, idx, B = _setup(oracle, "MIT", 0, 0, 5)
    piv = _smallest_pivot(g, sysm)
    out = restate(sysm, g, 0, B, (0, 1, 2, 3, 4))
    res = np.stack([_residuals(sysm, B, out[k]) for k in range(5)])
    ref = reference_blocks(oracle, g, poses, idx, 0)
    err = [block_errors(_blocks(sysm, idx, out[k])[1:], ref[1:]).max() for k in range(5)]
    print(f"MIT METHOD 0 after 5 LM iterations: smallest pivot eigenvalue of T {piv:.3e}; per refinement step 0..4 the largest true "
          f"residual {[float('%.2e' % r) for r in res.max(axis=1)]} and block error {[float('%.2e' % e) for e in err]} (BLOCK_REL {BLOCK_REL:g})")
    assert piv > 0.0
    for k in range(1, 4):   # the rule keeps stepping: a column above rtol gains 10 % or more from the next step
        above = res[k] > RTOL
        assert (res[k + 1][above] <= 0.9 * res[k][above]).all(), k
    assert res[4].max() <= RES_MAX, res[4].max()   # the mandatory step and three more: accepted, not PGO_ERR_NUMERIC
