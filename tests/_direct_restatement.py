"""numpy restatement of the direct linear solve of csrc/direct.hip.h, shared by test_direct_solve_math.py,
test_direct_restatement.py (CPU) and test_gpu_direct.py / test_gpu_fuzz.py (GPU): chain split, block LDL' recurrence of the
odometry chain T, segment-parallel sweeps joined through prefix products, every other edge as a low-rank term V'V through the
Woodbury identity (I + V Z by LAPACK's Cholesky), iterative refinement against the whole matrix.  The same algorithm as the
kernels in fp64 with LAPACK's arithmetic: what it reaches on a system is what the method allows there.  (The kernels
factorise the chain in pieces cut at separator poses and join them through a Schur complement; algebraically that is
the one recurrence over the whole chain run here.)"""
import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

EPS = 2.0 ** -53


def _chain_split(g):
    """the first edge of every pair of consecutive poses (either orientation) is the chain's; all others are low-rank terms"""
    chain = -np.ones(g.n_poses, np.int64)
    for e, (a, b) in enumerate(zip(g.ia, g.ib)):
        lo, hi = min(a, b), max(a, b)
        if hi == lo + 1 and chain[lo] < 0:
            chain[lo] = e
    is_chain = np.zeros(g.n_edges, bool)
    is_chain[chain[chain >= 0]] = True
    return is_chain


def _chain_blocks(T):
    """the 3x3 blocks M_i = T[i, i] and C_i = T[i, i - 1] (C_0 = 0) of a sparse block-tridiagonal matrix, without densifying it"""
    n = T.shape[0] // 3
    co = sp.coo_matrix(T)
    bi, bj = co.row // 3, co.col // 3
    assert np.all(np.abs(bi - bj) <= 1), "T is not block tridiagonal"
    M, Cb = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    d = bi == bj
    np.add.at(M, (bi[d], co.row[d] % 3, co.col[d] % 3), co.data[d])
    lo = bj == bi - 1
    np.add.at(Cb, (bi[lo], co.row[lo] % 3, co.col[lo] % 3), co.data[lo])
    return M, Cb


def _factor(T):
    """k_dlr_factor: W_i = C_i S_{i-1}^-1, S_i = M_i - W_i C_i'"""
    n = T.shape[0] // 3
    M, Cb = _chain_blocks(T)
    W, Sinv = [np.zeros((3, 3))] * n, [None] * n
    Sinv[0] = np.linalg.inv(M[0])
    for i in range(1, n):
        C = Cb[i]
        W[i] = C @ Sinv[i - 1]
        Sinv[i] = np.linalg.inv(M[i] - W[i] @ C.T)
    return W, Sinv


def _solve_segmented(W, Sinv, B, nseg=32):
    """k_dlr_prefix / _fwd / _mid / _fix: sweeps cut into segments, joined through the prefix products G, Gb"""
    n = len(W)
    L = -(-n // nseg)
    segs = [(s0, min(n, s0 + L)) for s0 in range(0, n, L)]
    Wn = W + [np.zeros((3, 3))]
    G, Gb = [None] * n, [None] * n
    for i0, i1 in segs:
        g = np.eye(3)
        for i in range(i0, i1):
            g = -W[i] @ g
            G[i] = g
        g = np.eye(3)
        for i in range(i1 - 1, i0 - 1, -1):
            g = -Wn[i + 1].T @ g
            Gb[i] = g
    X = B.copy().reshape(n, 3, -1)
    E = []
    for i0, i1 in segs:                       # local forward sweeps
        t = np.zeros_like(X[0])
        for i in range(i0, i1):
            t = X[i] - W[i] @ t
            X[i] = t
        E.append(t)
    tin, E2 = np.zeros_like(X[0]), []
    tins = []
    for q, (i0, i1) in enumerate(segs):
        tins.append(tin)
        tin = E[q] + G[i1 - 1] @ tin
    for q, (i0, i1) in enumerate(segs):       # true t on the fly, local backward sweeps
        z = np.zeros_like(X[0])
        for i in range(i1 - 1, i0 - 1, -1):
            t = X[i] + G[i] @ tins[q]
            z = Sinv[i] @ t - Wn[i + 1].T @ z
            X[i] = z
        E2.append(z)
    xin = np.zeros_like(X[0])
    for q in range(len(segs) - 1, -1, -1):    # incoming x from the right
        i0, i1 = segs[q]
        if q < len(segs) - 1:
            for i in range(i0, i1):
                X[i] = X[i] + Gb[i] @ xin
        xin = E2[q] + Gb[i0] @ xin
    return X.reshape(3 * n, -1)


def restate(sysm, g, fixed_pose, B, refine):
    """Y = (H + D'D)^-1 B as the direct solve computes it.  sysm = oracle.lm_system(...) (its rows and columns of the constant
    pose are those of the identity, which the recurrence passes through like any other pose: W = 0 on both sides of it), g a
    graph with n_poses / n_edges / ia / ib, B = [3N, k] right-hand sides (zero on the constant pose), refine = steps of
    iterative refinement, or a tuple of step counts: then a dict {steps: Y} from one factorisation.  Raises
    numpy.linalg.LinAlgError where the Cholesky factorisation of I + V Z breaks down."""
    N = g.n_poses
    B = np.asarray(B, np.float64).reshape(3 * N, -1)
    if fixed_pose >= 0:
        assert not B[3 * fixed_pose:3 * fixed_pose + 3].any()
    rows_c = np.repeat(_chain_split(g), 3)
    JS = sysm.JS.tocsr()
    Ac, V = JS[rows_c], JS[~rows_c]
    K = V.shape[0]
    T = (Ac.T @ Ac + sp.diags(sysm.d2)).tocsr()
    A = (sysm.H + sp.diags(sysm.d2)).tocsr()
    W, Sinv = _factor(T)
    Vd = V.toarray()
    ZT = _solve_segmented(W, Sinv, np.concatenate([Vd.T, B], axis=1))
    Z, Tb = ZT[:, :K], ZT[:, K:]
    cf = sl.cho_factor(np.eye(K) + Vd @ Z) if K else None

    def woodbury(t):
        return t - Z @ sl.cho_solve(cf, Vd @ t) if K else t

    counts = (refine,) if np.isscalar(refine) else tuple(refine)
    Y = woodbury(Tb)
    out = {0: Y}
    for it in range(max(counts)):
        res = B - A @ Y
        Y = Y + woodbury(_solve_segmented(W, Sinv, res))
        out[it + 1] = Y
    return out[refine] if np.isscalar(refine) else {k: out[k] for k in counts}


def system_matrix(sysm):
    return (sysm.H + sp.diags(sysm.d2)).tocsr()


def product_ld(A, y):
    """A y accumulated in numpy.longdouble (A: CSR with a full diagonal)"""
    A = A.tocsr()
    assert np.all(np.diff(A.indptr) > 0)
    prod = A.data.astype(np.longdouble) * np.asarray(y, np.float64)[A.indices].astype(np.longdouble)
    return np.add.reduceat(prod, A.indptr[:-1])


def norm_inf(A):
    return float(abs(A).sum(axis=1).max())


def rounding_floor(A):
    """4 x (largest number of nonzeros in a row of A) x 2^-53: the first-order rounding bound of one row of the residual
    product itself; a backward error below it measures the test's arithmetic, not the solver"""
    return 4.0 * float(np.diff(A.tocsr().indptr).max()) * EPS


def backward_error(A, y, b, Ay=None, a_norm=None):
    """|b - A y| / (|A| |y| + |b|), infinity norms, the residual in numpy.longdouble; Ay: a product computed elsewhere (the
    handle's own operator) in place of A y"""
    Ay = product_ld(A, y) if Ay is None else np.asarray(Ay, np.float64).astype(np.longdouble)
    res = np.abs(np.asarray(b, np.float64).astype(np.longdouble) - Ay).max()
    den = (norm_inf(A) if a_norm is None else a_norm) * np.abs(y).max() + np.abs(b).max()
    return float(res / den)
