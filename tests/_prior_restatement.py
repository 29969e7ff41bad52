"""numpy restatement of absolute pose priors (pgo_set_priors, csrc/prior.h) and of the LM loop with them: the reference of
tests/test_prior_native.py, tests/test_prior_host.py and tests/test_gpu_priors.py.

lm() restates the loop of _loss_restatement.lm for METHOD 0 / 1 (priors refuse METHOD 2) with extra residual rows per prior,
sqrt(rho') R d with Jacobian sqrt(rho') R on the pose's three columns, Lambda = R'R an eigen root (Lambda may be
semi-definite).  Without priors nothing is appended and every statement is the one _loss_restatement.lm runs: the result is
bitwise the same (tests/test_prior_host.py).

Priors are a dict: pose (n,) int, mean (n, 3), info (n, 3, 3) symmetric; the loss is a (name, a) pair."""
import math

import numpy as np

import _loss_restatement as LR

TWO_PI = 2.0 * math.pi
IDX6 = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])   # I11 I12 I13 I22 I23 I33 of a symmetric 3x3


def info6(mats):
    return np.asarray(mats, np.float64).reshape(-1, 3, 3)[:, IDX6[0], IDX6[1]]


def info_mat(rows6):
    rows6 = np.asarray(rows6, np.float64).reshape(-1, 6)
    M = np.zeros((len(rows6), 3, 3))
    M[:, IDX6[0], IDX6[1]] = rows6
    M[:, IDX6[1], IDX6[0]] = rows6
    return M


def make(pose, mean, info):
    pose = np.asarray(pose, np.int64).reshape(-1)
    info = np.asarray(info, np.float64)
    info = info_mat(info) if info.size == 6 * len(pose) else info.reshape(-1, 3, 3)
    return dict(pose=pose, mean=np.asarray(mean, np.float64).reshape(-1, 3), info=info)


def residuals(pri, poses):
    """d (n, 3) with the heading wrapped by the IEEE remainder, and chi2 = max(0, d' Lambda d)"""
    x = np.asarray(poses, np.float64).reshape(-1, 3)[pri["pose"]]
    d = x - pri["mean"]
    d[:, 2] = [math.remainder(v, TWO_PI) for v in d[:, 2]]
    chi2 = np.maximum(0.0, np.einsum("ni,nij,nj->n", d, pri["info"], d))
    return d, chi2


def closed(pose, mean, rows6, loss):
    """pgo_prior_eval in the association order of csrc/prior.h, on Python floats: (d, chi2, sum |terms| of chi2, rho triple)"""
    l00, l01, l02, l11, l12, l22 = (float(v) for v in rows6)
    d = [float(pose[0]) - float(mean[0]), float(pose[1]) - float(mean[1]), math.remainder(float(pose[2]) - float(mean[2]), TWO_PI)]
    q = [l00 * d[0] + l01 * d[1] + l02 * d[2], l01 * d[0] + l11 * d[1] + l12 * d[2], l02 * d[0] + l12 * d[1] + l22 * d[2]]
    s = d[0] * q[0] + d[1] * q[1] + d[2] * q[2]
    mag = sum(abs(a * d[i] * d[j]) for (i, j, a) in ((0, 0, l00), (0, 1, 2 * l01), (0, 2, 2 * l02), (1, 1, l11), (1, 2, 2 * l12), (2, 2, l22)))
    s = max(0.0, s)
    return np.array(d), s, mag, tuple(float(v) for v in LR.rho(loss[0], loss[1], np.array(s)))


def cost(pri, loss, poses):
    return 0.5 * float(LR.rho(loss[0], loss[1], residuals(pri, poses)[1])[0].sum())


def roots(pri):
    """R (n, 3, 3) with R'R = Lambda: sqrt(max(w, 0)) V' of the eigen decomposition"""
    w, V = np.linalg.eigh(pri["info"])
    return np.sqrt(np.maximum(w, 0.0))[:, :, None] * np.transpose(V, (0, 2, 1))


def rows(pri, loss, poses, apply_loss=True):
    """(cost, r (3n,), J (n, 3, 3)) of the priors' corrected rows"""
    d, chi2 = residuals(pri, poses)
    r0, r1, _ = LR.rho(loss[0], loss[1], chi2)
    R = roots(pri)
    sc = np.sqrt(r1) if apply_loss else np.ones_like(r1)
    return 0.5 * float(r0.sum()), (sc[:, None] * np.einsum("nij,nj->ni", R, d)).reshape(-1), sc[:, None, None] * R


def normal_eq_terms(pri, loss, poses, scale, apply_loss=True, chi2=None):
    """the priors' share of the scaled system: dH (n, 3, 3) = S (rho' Lambda) S, dg (n, 3) = S (rho' Lambda d), and the cost.
    chi2: the values to evaluate the loss at instead of this function's own (rho' is ill-conditioned near a loss's bend: Tukey's
    (1 - s / a^2)^2 loses 1 / (1 - s / a^2) in relative accuracy), for a caller that checks chi2 on its own"""
    d, own = residuals(pri, poses)
    chi2 = own if chi2 is None else np.asarray(chi2, np.float64)
    r0, r1, _ = LR.rho(loss[0], loss[1], chi2)
    w = r1 if apply_loss else np.ones_like(r1)
    S = np.asarray(scale, np.float64).reshape(-1, 3)[pri["pose"]]
    L = w[:, None, None] * pri["info"]
    return S[:, :, None] * L * S[:, None, :], S * np.einsum("nij,nj->ni", L, d), 0.5 * float(r0.sum())


def lm(O, og, losses, cls, priors=None, prior_loss=("trivial", 0.0), method=1, max_iters=50, fixed_pose=0, info_weighting=False,
       phi=0.5, ftol=1e-6, gtol=1e-10, ptol=1e-8, radius0=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3,
       min_lm_diagonal=1e-6, max_lm_diagonal=1e32):
    """_loss_restatement.lm for METHOD 0 / 1, with the priors' rows appended to the residual vector and the Jacobian"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    assert method in (0, 1)
    N, E = og.n_poses, og.n_edges
    ia, ib = np.asarray(og.ia, np.int64), np.asarray(og.ib, np.int64)
    n_pri = 0 if priors is None else len(priors["pose"])
    z = np.array(og.poses, np.float64).reshape(-1)
    free = np.ones(3 * N, bool)
    if fixed_pose >= 0:
        free[3 * fixed_pose:3 * fixed_pose + 3] = False
    free_idx = np.nonzero(free)[0]
    rows_p = np.repeat(np.arange(3 * E).reshape(E, 3), 6, axis=1).reshape(-1)
    cols_p = np.tile(np.concatenate([3 * ia[:, None] + np.arange(3), 3 * ib[:, None] + np.arange(3)], axis=1), (1, 3))
    cols_p = cols_p.reshape(-1)
    if n_pri:
        rows_q = np.repeat(np.arange(3 * n_pri), 3)
        cols_q = np.tile(3 * priors["pose"][:, None] + np.arange(3), (1, 3)).reshape(-1)

    def ev(zv, with_j):
        x = zv[:3 * N].reshape(N, 3)
        cost, r, J = LR.evaluate(O, og, losses, cls, x, method, True, info_weighting, phi)
        if n_pri:
            pc, pr, pJ = rows(priors, prior_loss, x)
            cost = cost + pc
        if not with_j:
            return cost, None, None
        A = sp.csr_matrix((J.reshape(-1), (rows_p, cols_p)), shape=(3 * E, 3 * N))
        rv = r.reshape(-1)
        if n_pri:
            A = sp.vstack([A, sp.csr_matrix((pJ.reshape(-1), (rows_q, cols_q)), shape=(3 * n_pri, 3 * N))]).tocsr()
            rv = np.concatenate([rv, pr])
        return cost, rv, A[:, free_idx].tocsc()

    res = LR.Result()
    cost, rvec, A = ev(z, True)
    res.initial_cost = res.final_cost = cost
    if not np.isfinite(cost):
        res.termination = 6
        res.poses = z[:3 * N].reshape(N, 3)
        return res
    s = 1.0 / (1.0 + np.sqrt(np.asarray(A.multiply(A).sum(axis=0)).reshape(-1)))
    grad = A.T @ rvec
    gmax = float(np.max(np.abs(grad)))
    x_norm = float(np.linalg.norm(z[free_idx]))
    radius, dec, prev_success, invalid_run = radius0, 2.0, True, 0
    recs = [dict(iter=0, step_ok=1, cost=cost, cost_change=0.0, gradient_max_norm=gmax, step_norm=0.0,
                 relative_decrease=0.0, radius=radius)]
    it, term = 0, 4
    while True:
        it += 1
        if it > max_iters:
            term, it = 4, it - 1
            break
        if prev_success and gmax <= gtol:
            term, it = 2, it - 1
            break
        if radius < min_radius:
            term, it = 5, it - 1
            break
        As = A @ sp.diags(s)
        H = (As.T @ As).tocsc()
        D2 = np.clip(H.diagonal(), min_lm_diagonal, max_lm_diagonal) / radius
        y = spla.splu((H + sp.diags(D2)).tocsc()).solve(s * grad)
        m = As @ (-y)
        model = float(-m @ (rvec + 0.5 * m))
        rec = dict(iter=it, step_ok=0, cost=cost, cost_change=0.0, gradient_max_norm=gmax, step_norm=0.0,
                   relative_decrease=0.0, radius=radius)
        if not np.all(np.isfinite(y)) or not (model > 0.0):
            invalid_run += 1
            if invalid_run >= 5:
                term = 6
                break
            radius /= dec
            dec *= 2.0
            prev_success = False
            rec.update(step_ok=-1, radius=radius)
            recs.append(rec)
            continue
        invalid_run = 0
        delta = np.zeros_like(z)
        delta[free_idx] = -s * y
        cand = z + delta
        cand_cost = ev(cand, False)[0]
        if not np.isfinite(cand_cost):
            cand_cost = np.finfo(np.float64).max
        step_norm = float(np.linalg.norm(delta))
        cost_change = cost - cand_cost
        rec.update(step_norm=step_norm, cost_change=cost_change)
        if step_norm <= ptol * (x_norm + ptol):
            term = 3
            recs.append(rec)
            break
        if abs(cost_change) <= ftol * cost:
            term = 1
            recs.append(rec)
            break
        rho_ = cost_change / model if cand_cost < np.finfo(np.float64).max else -np.inf
        rec.update(relative_decrease=rho_)
        if rho_ > min_relative_decrease:
            z = cand
            x_norm = float(np.linalg.norm(z[free_idx]))
            cost, rvec, A = ev(z, True)
            if not np.isfinite(cost):
                term = 6
                break
            grad = A.T @ rvec
            gmax = float(np.max(np.abs(grad)))
            radius = min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho_ - 1.0) ** 3))
            dec, prev_success = 2.0, True
            res.successful_steps += 1
            rec.update(step_ok=1, cost=cost, gradient_max_norm=gmax)
        else:
            radius /= dec
            dec *= 2.0
            prev_success = False
            rec.update(step_ok=0, cost=cand_cost)
        rec.update(radius=radius)
        recs.append(rec)
    res.poses = z[:3 * N].reshape(N, 3)
    res.termination, res.iterations, res.final_cost, res.records = term, it, cost, recs
    return res


# ---------------------------------------------------------------- priors as anchor edges (tests 2 and 5)
# Route A: one extra pose at the origin, constant, and one edge of kind 0 from it per prior, with measurement z and information
# Omega.  Route B: the prior z with Lambda = Q Omega Q', Q = diag(R(z_theta), 1), and no constant pose.  The edge residual is
# R(z_theta)'(p - z_xy) and asin(sin(theta - z_theta)): both routes state the same problem while every heading residual stays
# below pi / 2 (the edge model folds with asin).
N_ANCHOR_PRIORS = 12


def anchor_case(O, og, start, seed=11, n_pri=N_ANCHOR_PRIORS):
    """-> (og_a: the graph with the anchor pose appended and the anchor edges, all informations identity but the anchors';
           og_b: the graph with identity informations; the priors for og_b), both graphs starting at `start` (N, 3)"""
    rng = np.random.default_rng(seed)
    N, E = og.n_poses, og.n_edges
    start = np.asarray(start, np.float64).reshape(N, 3)
    pose = np.sort(rng.choice(np.arange(1, N), n_pri, replace=False))
    z = start[pose] + rng.normal(size=(n_pri, 3)) * np.array([0.05, 0.05, 0.02])
    B = rng.normal(size=(n_pri, 3, 3))
    Om = np.einsum("nij,nkj->nik", B, B) + 0.5 * np.eye(3)   # SPD
    Om = 0.5 * (Om + np.transpose(Om, (0, 2, 1)))
    c, s = np.cos(z[:, 2]), np.sin(z[:, 2])
    Q = np.zeros((n_pri, 3, 3))
    Q[:, 0, 0], Q[:, 0, 1], Q[:, 1, 0], Q[:, 1, 1], Q[:, 2, 2] = c, -s, s, c, 1.0
    Lam = np.einsum("nij,njk,nlk->nil", Q, Om, Q)
    Lam = 0.5 * (Lam + np.transpose(Lam, (0, 2, 1)))
    ident = np.tile(info6(np.eye(3)[None]), (E, 1))
    og_b = O.Graph(np.array(og.pose_id), start.copy(), np.array(og.ia), np.array(og.ib), np.array(og.meas), ident, np.array(og.kind))
    # (the anchor edges, kind 0, are appended after the graph's own edges, which keep their order)
    ids_a = np.concatenate([np.array(og.pose_id), [int(np.max(og.pose_id)) + 1]])
    poses_a = np.vstack([start, np.zeros((1, 3))])
    ia_a = np.concatenate([np.array(og.ia), np.full(n_pri, N)]).astype(np.int32)
    ib_a = np.concatenate([np.array(og.ib), pose]).astype(np.int32)
    meas_a = np.vstack([np.array(og.meas), z])
    info_a = np.vstack([ident, info6(Om)])
    kind_a = np.concatenate([np.array(og.kind), np.zeros(n_pri, np.uint8)]).astype(np.uint8)
    og_a = O.Graph(ids_a, poses_a, ia_a, ib_a, meas_a, info_a, kind_a)
    return og_a, og_b, make(pose, z, Lam)
