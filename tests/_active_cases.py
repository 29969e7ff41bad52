"""Shared inputs of the active-set tests (pgo_set_active): INTEL + 50 bogus loops (seed 1), the layer and window masks, the
numpy restatement of pgo_active_plan, and the EXTRACTED problem -- the active edges and the used poses renumbered 0..n-1
in order -- which is what the masked handle is compared with (never with itself)."""
import os

import numpy as np

from conftest import DATA

N_INTEL, E_INTEL = 1228, 1533          # 1227 odometry / 256 closure / 50 bogus
WINDOW_EDGE, WINDOW_RADIUS, WINDOW_ANCHOR = 1233, 5, 39


def intel(pgo):
    g = pgo.ReadG2O(os.path.join(DATA, "INTEL.g2o"))
    g.add_random_C(50, 1)
    return g


def arrays(g):
    return {k: np.array(getattr(g, k)) for k in ("poses", "ia", "ib", "meas", "kind", "info")}


def layer_mask(kind, seed=0):
    """all odometry plus the loops where default_rng(seed).random(#loops) < 0.5"""
    m = np.ones(len(kind), bool)
    loops = np.nonzero(kind != 0)[0]
    m[loops] = np.random.default_rng(seed).random(len(loops)) < 0.5
    return m


def window_masks(a, edge=WINDOW_EDGE, radius=WINDOW_RADIUS):
    """(edge mask, pose_constant mask, anchor): the poses within `radius` of either end of `edge`, the odometry edges with
    both ends among them plus `edge` itself; the smallest used pose is the anchor"""
    ia, ib, kind = a["ia"], a["ib"], a["kind"]
    n = len(a["poses"])
    inw = np.zeros(n, bool)
    for p in (ia[edge], ib[edge]):
        inw[max(0, p - radius):min(n, p + radius + 1)] = True
    m = (kind == 0) & inw[ia] & inw[ib]
    m[edge] = True
    anchor = int(min(ia[m].min(), ib[m].min()))
    pc = np.zeros(n, bool)
    pc[anchor] = True
    return m, pc, anchor


def plan(n_poses, ia, ib, edge_active=None, pose_constant=None, fixed_pose=0):
    """numpy restatement of pgo_active_plan: (constant[n], n_active_edges, n_free_poses)"""
    act = np.ones(len(ia), bool) if edge_active is None else np.asarray(edge_active) != 0
    used = np.zeros(n_poses, bool)
    used[np.asarray(ia)[act]] = True
    used[np.asarray(ib)[act]] = True
    const = ~used
    if pose_constant is not None:
        const |= np.asarray(pose_constant) != 0
    if fixed_pose >= 0:
        const[fixed_pose] = True
    return const.astype(np.uint8), int(act.sum()), int((~const).sum())


def extract(pgo, a, edge_active, anchor):
    """(Graph of the extracted problem, used poses (old indices), the anchor's new index)"""
    act = np.asarray(edge_active) != 0
    used = np.unique(np.concatenate([a["ia"][act], a["ib"][act]]))
    new = -np.ones(len(a["poses"]), np.int64)
    new[used] = np.arange(len(used))
    g = pgo.Graph.from_arrays(a["poses"][used], new[a["ia"][act]], new[a["ib"][act]], a["meas"][act], a["kind"][act],
                              a["info"][act])
    return g, used, int(new[anchor])


def lm_direct_const(O, g, opt, constant):
    """oracle.lm_direct's policy (Ceres TrustRegionMinimizer + LevenbergMarquardtStrategy, sparse direct solve of the
    normal equations) with ANY set of constant poses: oracle.lm_direct takes one.  Residuals and Jacobians come from
    oracle.evaluate; with constant = {opt.fixed_pose} the two agree (the tests check that before they rely on this).
    Returns (poses, termination, iterations, final_cost, step_ok history)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    N, E = g.n_poses, g.n_edges
    x = np.array(g.poses, np.float64, copy=True)
    free_idx = np.nonzero(np.repeat(~(np.asarray(constant) != 0), 3))[0]
    rows = np.repeat(np.arange(3 * E).reshape(E, 3), 6, axis=1).reshape(-1)
    cols = np.concatenate([3 * g.ia[:, None] + np.arange(3), 3 * g.ib[:, None] + np.arange(3)], axis=1)
    cols = np.tile(cols, (1, 3)).reshape(-1).astype(np.int64)

    def ev(p, with_j):
        c, r, J = O.evaluate(g, p, opt.method, opt.phi, opt.huber_delta, True, with_j, with_j)
        if not with_j:
            return c, None, None
        A = sp.csr_matrix((J.reshape(-1), (rows, cols)), shape=(3 * E, 3 * N))[:, free_idx].tocsc()
        return c, r.reshape(-1), A

    cost, rvec, A = ev(x, True)
    s = 1.0 / (1.0 + np.sqrt(np.asarray(A.multiply(A).sum(axis=0)).reshape(-1))) if opt.jacobi_scaling else np.ones(A.shape[1])
    grad = A.T @ rvec
    gmax = float(np.max(np.abs(grad)))
    x_norm = float(np.linalg.norm(x.reshape(-1)[free_idx]))
    radius, dec, prev_success, invalid_run = opt.radius0, 2.0, True, 0
    hist, it, term = [1], 0, 4
    while True:
        it += 1
        if it > opt.max_iters or (prev_success and gmax <= opt.gtol) or radius < opt.min_radius:
            term = 4 if it > opt.max_iters else (2 if prev_success and gmax <= opt.gtol else 5)
            it -= 1
            break
        As = A @ sp.diags(s)
        H = (As.T @ As).tocsc()
        D2 = np.clip(H.diagonal(), opt.min_lm_diagonal, opt.max_lm_diagonal) / radius
        y = spla.splu((H + sp.diags(D2)).tocsc()).solve(s * grad)
        m = As @ (-y)
        model = float(-m @ (rvec + 0.5 * m))
        if not np.all(np.isfinite(y)) or not (model > 0.0):
            invalid_run += 1
            if invalid_run >= 5:
                term = 6
                break
            radius /= dec
            dec *= 2.0
            prev_success = False
            hist.append(-1)
            continue
        invalid_run = 0
        delta = np.zeros(3 * N)
        delta[free_idx] = -s * y
        cand = x + delta.reshape(N, 3)
        cand_cost = ev(cand, False)[0]
        if not np.isfinite(cand_cost):
            cand_cost = np.finfo(np.float64).max
        step_norm = float(np.linalg.norm(delta))
        cost_change = cost - cand_cost
        if step_norm <= opt.ptol * (x_norm + opt.ptol) or abs(cost_change) <= opt.ftol * cost:
            term = 3 if step_norm <= opt.ptol * (x_norm + opt.ptol) else 1
            hist.append(0)
            break
        rho = cost_change / model if cand_cost < np.finfo(np.float64).max else -np.inf
        if rho > opt.min_relative_decrease:
            x = cand
            x_norm = float(np.linalg.norm(x.reshape(-1)[free_idx]))
            cost, rvec, A = ev(x, True)
            if not np.isfinite(cost):
                term = 6
                break
            grad = A.T @ rvec
            gmax = float(np.max(np.abs(grad)))
            radius = min(opt.max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            dec, prev_success = 2.0, True
            hist.append(1)
        else:
            radius /= dec
            dec *= 2.0
            prev_success = False
            hist.append(0)
    return x, term, it, cost, hist
