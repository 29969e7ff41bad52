"""numpy restatement of pgo_posterior_sample: the noise stream of csrc/sample.h (vectorised Philox4x32-10 + Box-Muller), the
right-hand side b = J' eps (+ R eps_p) from the oracle's per-edge Jacobian blocks (built as
tests/test_gpu_covariance.py::reference_blocks builds its J; other losses through tests/_loss_restatement.py), the draws
delta = H^-1 b by a sparse LU, and the exact marginal blocks the estimate is judged against."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TWO_PI = 6.283185307179586476925286766559
STREAM_EDGE, STREAM_PRIOR = 0, 1


def philox(ctr, key):
    """Philox4x32-10: ctr (..., 4), key (2,) or (..., 2), as unsigned integers -> (..., 4) uint64 holding 32-bit words"""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & MASK for i in range(4)]
    key = np.asarray(key).astype(np.uint64)
    k0, k1 = key[..., 0] & MASK, key[..., 1] & MASK
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & MASK, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1)


def uniform(lo, hi):
    """((hi << 21 | lo >> 11) + 0.5) 2^-53, the one tie that would round to 1 taken downwards"""
    k = (hi << np.uint64(21)) | (lo >> np.uint64(11))
    return np.minimum((k.astype(np.float64) + 0.5) * 2.0 ** -53, 1.0 - 2.0 ** -53)


def triples(seed, stream, index, sample):
    """the standard normal triples of (seed, stream, index[i], sample[i]): (n, 3); index and sample broadcast"""
    index, sample = np.broadcast_arrays(np.asarray(index, np.uint64), np.asarray(sample, np.uint64))
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    z = np.empty(index.shape + (3,))
    for word in (0, 1):
        ctr = np.stack([index, np.full(index.shape, word, np.uint64), sample, np.full(index.shape, stream, np.uint64)], axis=-1)
        o = philox(ctr, key)
        u0, u1 = uniform(o[..., 0], o[..., 1]), uniform(o[..., 2], o[..., 3])
        r = np.sqrt(-2.0 * np.log(u0))
        if word == 0:
            z[..., 0], z[..., 1] = r * np.cos(TWO_PI * u1), r * np.sin(TWO_PI * u1)
        else:
            z[..., 2] = r * np.cos(TWO_PI * u1)
    return z


def chol3_psd(L):
    """sample_chol3_psd of csrc/sample.h on (n, 3, 3) symmetric blocks: lower R with R R' = L, a zero pivot a zero column"""
    L = np.asarray(L, np.float64).reshape(-1, 3, 3)
    R = np.zeros_like(L)
    for k, l in enumerate(L):
        if l[0, 0] > 0.0:
            R[k, 0, 0] = np.sqrt(l[0, 0])
            R[k, 1, 0], R[k, 2, 0] = l[0, 1] / R[k, 0, 0], l[0, 2] / R[k, 0, 0]
        d1 = l[1, 1] - R[k, 1, 0] ** 2
        if d1 > 1e-14 * l[1, 1]:
            R[k, 1, 1] = np.sqrt(d1)
            R[k, 2, 1] = (l[1, 2] - R[k, 2, 0] * R[k, 1, 0]) / R[k, 1, 1]
        d2 = l[2, 2] - R[k, 2, 0] ** 2 - R[k, 2, 1] ** 2
        if d2 > 1e-14 * l[2, 2]:
            R[k, 2, 2] = np.sqrt(d2)
    return R


class Problem:
    """J (E, 3, 6) per edge in the caller's edge order (zero rows for an inactive edge), the constant poses, optional priors
    (pose (n,), Lw (n, 3, 3) = rho' Lambda): H = J'J (+ Lw on the priors' diagonal blocks) on the free poses, factorised once"""

    def __init__(self, n_poses, ia, ib, J, constant=(0,), prior_pose=None, prior_Lw=None):
        import scipy.sparse as sp

        self.N, self.E = int(n_poses), len(ia)
        self.ia, self.ib = np.asarray(ia, np.int64), np.asarray(ib, np.int64)
        self.J = np.asarray(J, np.float64).reshape(self.E, 3, 6)
        rows = np.repeat(np.arange(3 * self.E).reshape(self.E, 3), 6, axis=1).reshape(-1)
        cols = np.tile(np.concatenate([3 * self.ia[:, None] + np.arange(3), 3 * self.ib[:, None] + np.arange(3)], axis=1), (1, 3)).reshape(-1)
        self.Jm = sp.csr_matrix((self.J.reshape(-1), (rows, cols)), shape=(3 * self.E, 3 * self.N))
        self.absJm = abs(self.Jm)
        H = (self.Jm.T @ self.Jm).tolil()
        self.prior_pose = None if prior_pose is None else np.asarray(prior_pose, np.int64)
        if self.prior_pose is not None:
            self.prior_R = chol3_psd(prior_Lw)
            for p, Lw in zip(self.prior_pose, np.asarray(prior_Lw).reshape(-1, 3, 3)):
                H[3 * p:3 * p + 3, 3 * p:3 * p + 3] = H[3 * p:3 * p + 3, 3 * p:3 * p + 3].toarray() + Lw
        self.free = np.ones(3 * self.N, bool)
        for c in constant:
            self.free[3 * c:3 * c + 3] = False
        self.Hf = H.tocsc()[self.free][:, self.free].tocsc()
        self._lu = None

    @property
    def lu(self):
        """the sparse LU of H on the free poses, at its first use (the right-hand side alone needs none)"""
        if self._lu is None:
            import scipy.sparse.linalg as spl
            self._lu = spl.splu(self.Hf)
        return self._lu

    def eps(self, seed, sample):
        return triples(seed, STREAM_EDGE, np.arange(self.E), sample)

    def rhs(self, seed, sample):
        """b (N, 3) = J' eps (+ R eps_p), zero on the constant poses; and sum |J| |eps| per row (the scale of its rounding)"""
        e = self.eps(seed, sample).reshape(-1)
        b, mag = self.Jm.T @ e, self.absJm.T @ np.abs(e)
        if self.prior_pose is not None:
            zp = triples(seed, STREAM_PRIOR, np.arange(len(self.prior_pose)), sample)
            for k, p in enumerate(self.prior_pose):
                b[3 * p:3 * p + 3] += self.prior_R[k] @ zp[k]
                mag[3 * p:3 * p + 3] += np.abs(self.prior_R[k]) @ np.abs(zp[k])
        b[~self.free] = 0.0
        return b.reshape(self.N, 3), mag.reshape(self.N, 3)

    def solve(self, b):
        """delta (..., N, 3) = H^-1 b on the free poses, zero on the constant ones"""
        b = np.asarray(b, np.float64).reshape(-1, 3 * self.N)
        out = np.zeros_like(b)
        out[:, self.free] = self.lu.solve(np.ascontiguousarray(b[:, self.free].T)).T
        return out.reshape(-1, self.N, 3)

    def deltas(self, seed, first, n):
        return self.solve(np.stack([self.rhs(seed, first + s)[0] for s in range(n)]))

    def exact_blocks(self, poses=None):
        """Sigma_i (n, 3, 3) of the poses given (all: by 3 solves each, so keep the list short on large graphs)"""
        poses = np.arange(self.N) if poses is None else np.asarray(poses, np.int64)
        rhs = np.zeros((3 * len(poses), 3 * self.N))
        for j, p in enumerate(poses):
            for c in range(3):
                rhs[3 * j + c, 3 * p + c] = 1.0 if self.free[3 * p + c] else 0.0
        X = self.solve(rhs)
        B = np.stack([X[3 * j:3 * j + 3, p, :] for j, p in enumerate(poses)])
        return 0.5 * (B + np.transpose(B, (0, 2, 1)))

    def cond_estimate(self):
        """||H||_1 ||H^-1||_1 (onenormest): what a relative residual is multiplied by"""
        import scipy.sparse.linalg as spl
        inv = spl.LinearOperator(self.Hf.shape, matvec=self.lu.solve, rmatvec=self.lu.solve)
        return float(spl.onenormest(self.Hf) * spl.onenormest(inv))


def second_moment(deltas):
    d = np.asarray(deltas)
    return np.einsum("sni,snj->nij", d, d) / d.shape[0]


def whitened_errors(C, Sigma):
    """|| L^-1 C L^-T - I ||_F per pose, Sigma = L L' (positive definite blocks only)"""
    out = np.empty(len(C))
    for k, (c, s) in enumerate(zip(C, Sigma)):
        Li = np.linalg.inv(np.linalg.cholesky(s))
        out[k] = np.linalg.norm(Li @ c @ Li.T - np.eye(3))
    return out


def wishart_cap(n_samples):
    """3 sqrt(12 / S): 12 / S is the exact expectation of || Wishart(S, I) / S - I ||_F^2 in 3 dimensions"""
    return 3.0 * np.sqrt(12.0 / n_samples)


# ------------------------------------------------------------------------------------------------ the shared cases
# (name, seed, samples): the estimator cases of tests/test_sample_host.py and tests/test_gpu_sample.py, both at the graph's
# INITIAL poses so that the CPU test and the GPU test judge the same linearisation
ESTIMATOR_CASES = {"intel50-m1": (11, 1024), "w257": (7, 192)}
_PROBLEMS = {}


def case_graph(pgo, name):
    """(pgo graph, method) of a shared case"""
    import os
    from conftest import DATA
    import _solo_cases as SC
    if name == "intel50-m1":
        g = pgo.ReadG2O(os.path.join(DATA, "INTEL.g2o"))
        g.add_random_C(50, 1)
        return g, 1
    return SC.pgo_graph(pgo, name), 0


def case_problem(pgo, O, name):
    """the restated Problem of a shared case at its initial poses (computed once, never changed)"""
    from conftest import oracle_graph
    if name not in _PROBLEMS:
        g, method = case_graph(pgo, name)
        og = oracle_graph(O, g)
        _, _, J = O.evaluate(og, og.poses, method=method)
        _PROBLEMS[name] = Problem(og.n_poses, og.ia, og.ib, J)
    return _PROBLEMS[name]
