"""numpy restatement of Ceres' robust losses (pgo_set_losses) and of the LM loop around them: the reference of
tests/test_loss_host.py and tests/test_gpu_loss.py.

The oracle (oracle/) knows one loss, Huber, and stays as it is.  Here the corrector of each block's loss is applied to
the PLAIN residual blocks that oracle.evaluate(..., delta=0.0, apply_loss=False) and oracle.evaluate_sc return (after
DCS / the switch / whitening), and the minimiser is Ceres' TrustRegionMinimizer + LevenbergMarquardtStrategy as
oracle/pgo_oracle.c states it (Jacobi scaling, LM diagonal, radius and decrease-factor rules, tolerance tests), with a
sparse LU for the linear solve.  Losses are (name, a) pairs; `cls` is each block's class in the caller's edge order."""
import numpy as np

TYPES = {"trivial": 0, "huber": 1, "softlone": 2, "cauchy": 3, "arctan": 4, "tukey": 5}
DBL_MIN = np.finfo(np.float64).tiny


def rho(name, a, s):
    """(rho(s), rho'(s), rho''(s)) of Ceres 2.x LossFunction::Evaluate, vectorised over s >= 0"""
    s = np.asarray(s, np.float64)
    if name == "trivial":
        return s.copy(), np.ones_like(s), np.zeros_like(s)
    if name == "huber":
        b = a * a
        out = s > b
        so = np.where(out, s, 1.0)
        r = np.sqrt(so)
        r1 = np.maximum(DBL_MIN, a / r)
        return np.where(out, 2.0 * a * r - b, s), np.where(out, r1, 1.0), np.where(out, -r1 / (2.0 * so), 0.0)
    if name == "softlone":
        b = a * a
        c = 1.0 / b
        sm = 1.0 + s * c
        t = np.sqrt(sm)
        r1 = np.maximum(DBL_MIN, 1.0 / t)
        return 2.0 * b * (t - 1.0), r1, -(c * r1) / (2.0 * sm)
    if name == "cauchy":
        b = a * a
        c = 1.0 / b
        sm = 1.0 + s * c
        inv = 1.0 / sm
        return b * np.log(sm), np.maximum(DBL_MIN, inv), -c * inv * inv
    if name == "arctan":
        b = 1.0 / (a * a)
        sm = 1.0 + s * s * b
        inv = 1.0 / sm
        return a * np.arctan2(s, a), np.maximum(DBL_MIN, inv), -2.0 * s * b * inv * inv
    if name == "tukey":
        a2 = a * a
        inside = s <= a2
        v = 1.0 - s / a2
        return (np.where(inside, a2 / 3.0 * (1.0 - v * v * v), a2 / 3.0), np.where(inside, v * v, 0.0),
                np.where(inside, -2.0 / a2 * v, 0.0))
    raise ValueError(name)


def classes(kind, n_classes, edge_class=None):
    """each block's class: explicit, or min(kind, n_classes - 1) (pgo_set_losses with edge_class NULL)"""
    if edge_class is not None:
        return np.asarray(edge_class, np.int64)
    return np.minimum(np.asarray(kind, np.int64), n_classes - 1)


def block_rho(losses, cls, s):
    r0, r1, r2 = np.empty_like(s), np.empty_like(s), np.empty_like(s)
    for k, (name, a) in enumerate(losses):
        m = cls == k
        r0[m], r1[m], r2[m] = rho(name, a, s[m])
    return r0, r1, r2


def evaluate(O, og, losses, cls, poses=None, method=1, apply_loss=True, info_weighting=False, phi=0.5):
    """pgo_eval with per-class losses, METHOD 0 / 1: cost = 1/2 sum rho(|e|^2), r and J scaled by sqrt(rho')"""
    c, r, J = O.evaluate(og, poses, method, phi, 0.0, False, True, True, 1, info_weighting)
    s = (r * r).sum(axis=1)
    r0, r1, _ = block_rho(losses, cls, s)
    if apply_loss:
        sc = np.sqrt(r1)[:, None]
        r, J = sc * r, sc * J
    return (0.5 * r0.sum() if np.isfinite(c) else np.nan), r, J


def evaluate_sc(O, og, losses, cls, poses=None, switches=None, lam=1.0, apply_loss=True):
    """METHOD 2: the loss acts on s e (s the switch); r, J and d e / d s of a block scaled by the same sqrt(rho')"""
    c, r, J, Js, q = O.evaluate_sc(og, poses, switches, lam, 0.0, False)
    s = (r * r).sum(axis=1)
    r0, r1, _ = block_rho(losses, cls, s)
    if apply_loss:
        sc = np.sqrt(r1)[:, None]
        r, J, Js = sc * r, sc * J, sc * Js
    cost = 0.5 * r0.sum() + 0.5 * (q * q).sum()
    return (cost if np.isfinite(c) else np.nan), r, J, Js, q


class Result:
    def __init__(self):
        self.poses = self.switches = None
        self.termination, self.iterations, self.successful_steps = 4, 0, 0
        self.initial_cost = self.final_cost = 0.0
        self.records = []


def lm(O, og, losses, cls, method=1, max_iters=50, fixed_pose=0, lam=1.0, info_weighting=False, phi=0.5,
       ftol=1e-6, gtol=1e-10, ptol=1e-8, radius0=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3,
       min_lm_diagonal=1e-6, max_lm_diagonal=1e32):
    """ceres::Solve with the library's defaults; METHOD 2 on the joint (poses, switches) vector like oracle.lm_direct_sc"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    N, E = og.n_poses, og.n_edges
    ia, ib = np.asarray(og.ia, np.int64), np.asarray(og.ib, np.int64)
    sc_e = np.nonzero(np.asarray(og.kind) != 0)[0] if method == 2 else np.zeros(0, np.int64)
    M = len(sc_e)
    z = np.concatenate([np.array(og.poses, np.float64).reshape(-1), np.ones(M)])
    free = np.ones(3 * N + M, bool)
    if fixed_pose >= 0:
        free[3 * fixed_pose:3 * fixed_pose + 3] = False
    free_idx = np.nonzero(free)[0]
    rows_p = np.repeat(np.arange(3 * E).reshape(E, 3), 6, axis=1).reshape(-1)
    cols_p = np.tile(np.concatenate([3 * ia[:, None] + np.arange(3), 3 * ib[:, None] + np.arange(3)], axis=1), (1, 3))
    cols_p = cols_p.reshape(-1)
    sw_col = 3 * N + np.arange(M)

    def ev(zv, with_j):
        x = zv[:3 * N].reshape(N, 3)
        if method == 2:
            sw = np.ones(E)
            sw[sc_e] = zv[3 * N:]
            cost, r, J, Js, q = evaluate_sc(O, og, losses, cls, x, sw, lam)
            if not with_j:
                return cost, None, None
            A = sp.csr_matrix((np.concatenate([J.reshape(-1), Js[sc_e].reshape(-1), np.full(M, -np.sqrt(lam))]),
                               (np.concatenate([rows_p, (3 * sc_e[:, None] + np.arange(3)).reshape(-1), 3 * E + np.arange(M)]),
                                np.concatenate([cols_p, np.repeat(sw_col, 3), sw_col]))), shape=(3 * E + M, 3 * N + M))
            return cost, np.concatenate([r.reshape(-1), q[sc_e]]), A[:, free_idx].tocsc()
        cost, r, J = evaluate(O, og, losses, cls, x, method, True, info_weighting, phi)
        if not with_j:
            return cost, None, None
        A = sp.csr_matrix((J.reshape(-1), (rows_p, cols_p)), shape=(3 * E, 3 * N))
        return cost, r.reshape(-1), A[:, free_idx].tocsc()

    res = Result()
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
    if method == 2:
        sw = np.ones(E)
        sw[sc_e] = z[3 * N:]
        res.switches = sw
    res.termination, res.iterations, res.final_cost, res.records = term, it, cost, recs
    return res


def covariance_blocks(O, og, losses, cls, poses, idx, method=1, fixed=0):
    """diagonal blocks of (J'J)^-1 at `poses` (J the corrected Jacobian, constant pose removed) by a sparse LU"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl

    N, E = og.n_poses, og.n_edges
    ia, ib = np.asarray(og.ia, np.int64), np.asarray(og.ib, np.int64)
    _, _, J = evaluate(O, og, losses, cls, poses, method)
    rows = np.repeat(np.arange(3 * E).reshape(E, 3), 6, axis=1).reshape(-1)
    cols = np.tile(np.concatenate([3 * ia[:, None] + np.arange(3), 3 * ib[:, None] + np.arange(3)], axis=1), (1, 3)).reshape(-1)
    Jm = sp.csr_matrix((J.reshape(-1), (rows, cols)), shape=(3 * E, 3 * N)).tocsc()
    H = (Jm.T @ Jm).tocsc()
    keep = np.ones(3 * N, bool)
    keep[3 * fixed:3 * fixed + 3] = False
    pos = -np.ones(3 * N, np.int64)
    pos[keep] = np.arange(keep.sum())
    lu = spl.splu(H[keep][:, keep].tocsc())
    out = np.zeros((len(idx), 3, 3))
    for j, i in enumerate(idx):
        if i == fixed:
            continue
        rhs = np.zeros((keep.sum(), 3))
        for c in range(3):
            rhs[pos[3 * i + c], c] = 1.0
        X = lu.solve(rhs)
        B = X[pos[3 * i:3 * i + 3]]
        out[j] = 0.5 * (B + B.T)
    return out
