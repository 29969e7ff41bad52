"""Shared by test_coarsen_info_host.py, test_coarsen_info_native.py and test_gpu_coarsen_info.py: coarsening with information
(include/pgo.h, "hierarchical initialisation", "with information") restated in numpy from the definitions -- pairs (motion,
3x3 covariance), rotations from the angle at every composition, left to right, inverses by numpy.linalg.inv --, the closed
form of the straight unit chain, and the error bounds of the comparisons."""
import numpy as np

import _coarsen_cases as CC

EPS = CC.EPS
IDX = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # info6 / cov6 order: xx xy xt yy yt tt


def mat(v6):
    v6 = np.asarray(v6, np.float64)
    M = np.zeros(v6.shape[:-1] + (3, 3))
    for k, (i, j) in enumerate(IDX):
        M[..., i, j] = M[..., j, i] = v6[..., k]
    return M


def vec6(M):
    M = np.asarray(M, np.float64)
    return np.stack([M[..., i, j] for i, j in IDX], -1)


def pair_identity():
    return np.zeros(3), np.zeros((3, 3))


def pair_compose(PA, PB):
    (A, SA), (B, SB) = PA, PB
    c, s = np.cos(A[2]), np.sin(A[2])
    F = np.array([[1, 0, -(s * B[0] + c * B[1])], [0, 1, c * B[0] - s * B[1]], [0, 0, 1]])
    G = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return CC.compose(A, B), F @ SA @ F.T + G @ SB @ G.T


def pair_inverse(PA):
    A, SA = PA
    B = CC.inverse(A)
    c, s = np.cos(A[2]), np.sin(A[2])
    H = np.array([[-c, -s, B[1]], [s, -c, -B[0]], [0, 0, -1]])
    return B, H @ SA @ H.T


def unit_info(E):
    return np.tile([1.0, 0, 0, 1, 0, 1], (E, 1))


def restate_coarsen_info(n, ia, ib, meas, kind, info, S):
    """CC.restate_coarsen's dict with "cov", "info" (n_coarse, 6), "Ccov" (n, 6) and "Cendcov" (K - 1, 6)"""
    ia, ib, meas = np.asarray(ia), np.asarray(ib), np.asarray(meas, np.float64).reshape(-1, 3)
    out = CC.restate_coarsen(n, ia, ib, meas, kind, S)
    Sig = np.linalg.inv(mat(unit_info(len(ia)) if info is None else info))
    chain, _ = CC.chain_edges(n, ia, ib)
    K = out["n_poses"]

    def Z(i):
        e = chain[i]
        P = (meas[e], Sig[e])
        return P if ia[e] == i else pair_inverse(P)

    Cp = [pair_identity() for _ in range(n)]
    Cend = []
    for i in range(n):
        if i % S:
            Cp[i] = pair_compose(Cp[i - 1], Z(i - 1))
    for k in range(K - 1):
        Cend.append(pair_compose(Cp[(k + 1) * S - 1], Z((k + 1) * S - 1)))
    cov = [c[1] for c in Cend]
    for e in out["origin"][K - 1:]:
        m, sg = pair_compose(pair_compose(Cp[ia[e]], (meas[e], Sig[e])), pair_inverse(Cp[ib[e]]))
        cov.append(sg)
    cov = np.array(cov).reshape(-1, 3, 3)
    out["cov"], out["info"] = vec6(cov), vec6(np.linalg.inv(cov))
    out["Ccov"] = vec6(np.array([c[1] for c in Cp]))
    out["Cendcov"] = vec6(np.array([c[1] for c in Cend]).reshape(-1, 3, 3))
    return out


def straight_chain_cov(j):
    """Sigma after j unit steps (1, 0, 0) with unit information: integers, exact in binary64 for j <= 256"""
    j = np.asarray(j, np.int64)
    z = np.zeros_like(j)
    return np.stack([j, z, z, j + (j - 1) * j * (2 * j - 1) // 6, j * (j - 1) // 2, j], -1).astype(np.float64)


def random_spd_info(E, seed, cond=1e4):
    """E random SPD matrices with eigenvalues log-uniform in [1, cond], as info6"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.normal(size=(E, 3, 3)))[0]
    lam = np.exp(rng.uniform(0, np.log(cond), (E, 3)))
    return vec6(Q @ (lam[..., None] * np.swapaxes(Q, -1, -2)))


def _chain_sums(n, ia, ib, meas, info, S, ref):
    """what bounds and bounds_C share: per pose the prefix sums, from its key pose, of tr Sigma_i, Sigma_i[theta theta] and
    cond(Omega_i) |Sigma_i|_F over the chain motions before it, the radius of its segment up to it (max |C_j|, j <= i), the
    same four for whole segments, and (Sigma, cond) of every edge"""
    ia, ib, meas = np.asarray(ia), np.asarray(ib), np.asarray(meas, np.float64).reshape(-1, 3)
    chain, _ = CC.chain_edges(n, ia, ib)
    Om = mat(unit_info(len(ia)) if info is None else info)
    good = np.isfinite(Om).all(axis=(-2, -1))
    Sg, kap = np.zeros_like(Om), np.ones(len(Om))
    Sg[good], kap[good] = np.linalg.inv(Om[good]), np.linalg.cond(Om[good])
    tr, tt, iv = np.trace(Sg, axis1=-2, axis2=-1), Sg[:, 2, 2], kap * np.linalg.norm(Sg, axis=(-2, -1))
    ce = chain[:n - 1]
    rad = np.hypot(ref["C"][:, 0], ref["C"][:, 1])
    pre = np.zeros((n, 3))
    prad = np.zeros(n)
    for i in range(n):
        if i % S:
            pre[i] = pre[i - 1] + [tr[ce[i - 1]], tt[ce[i - 1]], iv[ce[i - 1]]]
            prad[i] = max(prad[i - 1], rad[i])
    K = -(-n // S)
    seg, srad = np.zeros((K - 1, 3)), np.zeros(K - 1)
    for k in range(K - 1):
        j = (k + 1) * S - 1
        seg[k] = pre[j] + [tr[ce[j]], tt[ce[j]], iv[ce[j]]]
        srad[k] = max(prad[j], np.hypot(ref["Cend"][k, 0], ref["Cend"][k, 1]))
    return pre, prad, seg, srad, (tr, tt, iv)


def _rel_cov(ncomp, dia, sums, tol_xy, A, Sref):
    W = 2 * (sums[..., 0] + dia ** 2 * sums[..., 1])
    absb = 2 * (3 * 132 * EPS * ncomp * W + 4 * (tol_xy + A) * W + 32 * EPS * (1 + dia) ** 2 * sums[..., 2])
    rel = absb / np.linalg.norm(Sref, axis=(-2, -1))
    return rel, np.linalg.cond(Sref) * (rel + 64 * EPS)


def bounds(n, ia, ib, meas, info, S, ref):
    """(rel_cov [n_coarse], rel_info [n_coarse]): bounds on the Frobenius-norm relative distance of two evaluations of the
    coarse covariances / informations that differ in rounding and association only; ref = the reference's dict (C, Cend, cov,
    origin: the bound uses the reference's own values, never the code under test).  First order in eps, per coarse edge:
      * its covariance is sum_i D_i Sigma_i D_i' over the factors i on its path (the chain motions of C_a, the edge, those of
        C_b); D_i, the derivative of the whole product in factor i, is a rotation and a lever arm r_i: the position of the
        path's end seen from factor i.  Every lever arm on the path, of any partial product in any association, joins two
        points of the path: it is below the path's diameter Dia.  Dia <= 2 rad for a composite (rad = max |C_j| over the
        segment) and <= 2 rad_a + |m| + 2 rad_b for a kept edge (rad_a = max |C_j|, j <= a, in a's segment).
      * Scale.  A partial product's covariance has xx, yy <= sum_i (tr Sigma_i + r_i^2 Sigma_i[tt]) (twice that with the cross
        terms 2 r Sigma[x theta] <= Sigma[xx] + r^2 Sigma[tt]), and an inverted factor's H Sigma H' the same with r = |m_i|.
        So with W = 2 sum_i (tr Sigma_i + Dia^2 Sigma_i[tt]) every xy entry of every node is below W, every x-theta entry
        below sqrt(W T) and theta-theta = T := sum_i Sigma_i[tt], with Dia^2 T <= W.
      * One node.  F Sigma_A F' + G Sigma_B G' forms an entry from at most 12 rounded operations; the terms of an xy entry
        are below (sx + |f| st)^2 <= 2 (sx^2 + f^2 st^2) <= 6 W, of an x-theta entry below 2 (sqrt(W T) + Dia T), theta-theta
        is one sum: errors e_xy <= 12 eps 6 W, e_xt <= 12 eps 4 sqrt(W T), e_tt <= eps T.  The rest of the product carries them
        to the result by a rotation and a lever arm below Dia: e_xy + 2 Dia e_xt + Dia^2 e_tt <= 12 eps (6 + 4 + 1) W =
        132 eps W per entry, 3 x 132 eps W in the Frobenius norm.  ncomp nodes feed an edge: one per factor but the first,
        one inversion per reversed factor, the closing inverse: ncomp <= 2 (factors) + 1.
      * The means.  D_i is formed from computed lever arms and rotations, good to tol_xy and A = S (Th + 4) eps (CC.bounds).
        d(D_i Sigma_i D_i') <= 2 |dD_i| |Sigma_i D_i'|: the lever column meets (Sigma[x theta] + r Sigma[tt]) <= W_i / max(Dia, 1)
        and the rotation meets at most W_i, with sum_i W_i = W: 4 (tol_xy + A) W, once per factor, not per node.
      * The inversions.  Omega_i^-1 is good to 32 eps cond(Omega_i) |Omega_i^-1|_F (Cholesky, inverse of the factor, product; LU
        in the restatement), in every entry, carried to the result by |D_i|_2^2 <= (1 + Dia)^2.
      * Two evaluations: a factor 2.
          abs = 2 (3 x 132 eps ncomp W + 4 (tol_xy + A) W + 32 eps (1 + Dia)^2 sum_i cond(Omega_i) |Sigma_i|_F)
          rel_cov = abs / |Sigma_ref|_F
      * the information is the inverse of that covariance: a relative perturbation rel_cov of Sigma, and the 32 eps of the
        inversion itself, are amplified by cond(Sigma_ref):      rel_info = cond(Sigma_ref) (rel_cov + 2 * 32 eps)."""
    ia, ib, meas = np.asarray(ia), np.asarray(ib), np.asarray(meas, np.float64).reshape(-1, 3)
    pre, prad, seg, srad, (tr, tt, iv) = _chain_sums(n, ia, ib, meas, info, S, ref)
    chain, _ = CC.chain_edges(n, ia, ib)
    turn = np.abs(meas[chain[:n - 1], 2])
    K = -(-n // S)
    A = S * (max(turn[k * S:(k + 1) * S].sum() for k in range(K)) + 4) * EPS
    tol_xy, _ = CC.bounds(n, ia, ib, meas, S)
    e = ref["origin"][K - 1:]
    a, b = ia[e], ib[e]
    own = np.stack([tr[e], tt[e], iv[e]], -1)
    sums = np.concatenate([seg, pre[a] + own + pre[b]])
    dia = np.concatenate([2 * srad, 2 * prad[a] + np.hypot(meas[e, 0], meas[e, 1]) + 2 * prad[b]])
    ncomp = np.concatenate([np.full(K - 1, 2 * S + 1), 2 * (a % S + b % S + 1) + 1])
    return _rel_cov(ncomp, dia, sums, tol_xy, A, mat(ref["cov"]))


def bounds_C(n, ia, ib, meas, info, S, ref):
    """rel_cov of bounds for the covariances of the composites C_i, one per pose that is no key pose (the path: the chain
    motions from the key pose to i); ref carries C, Cend and Ccov"""
    ia, ib, meas = np.asarray(ia), np.asarray(ib), np.asarray(meas, np.float64).reshape(-1, 3)
    pre, prad, seg, srad, _ = _chain_sums(n, ia, ib, meas, info, S, ref)
    chain, _ = CC.chain_edges(n, ia, ib)
    turn = np.abs(meas[chain[:n - 1], 2])
    K = -(-n // S)
    A = S * (max(turn[k * S:(k + 1) * S].sum() for k in range(K)) + 4) * EPS
    tol_xy, _ = CC.bounds(n, ia, ib, meas, S)
    i = np.nonzero(np.arange(n) % S != 0)[0]
    return _rel_cov(2 * (i % S) + 1, 2 * prad[i], pre[i], tol_xy, A, mat(ref["Ccov"][i]))[0]


def assert_close_cov(got6, want6, rel_bound, what=""):
    """Frobenius-relative distance of every matrix against its bound; prints the largest measured / bound ratio"""
    G, W = mat(np.reshape(got6, (-1, 6))), mat(np.reshape(want6, (-1, 6)))
    assert G.shape == W.shape, (what, G.shape, W.shape)
    if not len(G):
        return
    rel = np.linalg.norm(G - W, axis=(-2, -1)) / np.linalg.norm(W, axis=(-2, -1))
    rb = np.broadcast_to(rel_bound, rel.shape)
    k = int(np.argmax(rel / rb))
    print("%s: max relative distance %.3e, worst against its bound at %d: %.3e (bound %.3e)" % (what, rel.max(), k, rel[k], rb[k]))
    assert np.isfinite(G).all() and (rel <= rb).all(), (what, k, rel[k], rb[k])
