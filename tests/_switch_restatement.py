"""numpy / scipy.sparse restatement of METHOD 2's LM iteration on the JOINT parameter vector [poses; one switch per robust
edge], shared by test_switch_restatement.py (CPU) and test_gpu_switch_system.py / test_gpu_direct.py (GPU).

The kernels never form this system: k_switch_prepare / k_assemble<true> / k_switch_backsub (csrc/kernels.hip.h) eliminate each
switch per edge and solve the reduced pose system.  Here the joint damped system is written down as Ceres states it
(oracle.lm_direct_sc is the same policy), the switches are eliminated with one sparse Schur complement, and both routes to
the step are carried side by side: what they disagree by, delta_ref, is the reference's own error.

Notation, per robust edge e (rows 3e .. 3e+2 of the Jacobian and its prior row): j = d e / d s (after the loss corrector),
sigma = the switch column's Jacobi scale, X = the edge's rows of J S (pose columns),
    h_ss = sigma^2 (|j|^2 + lambda),  den = h_ss + clip(h_ss) / radius_elim,  g_s = sigma (j.r - sqrt(lambda) q),
    c = sigma^2 / den,  gamma = sigma g_s / den.
The reduced pose system is  sum X'(I - c j j')X + D'D  and  sum X'(r - gamma j);  with
    kappa = (1 - sqrt(1 - c |j|^2)) / |j|^2 = c / (1 + sqrt(1 - c |j|^2))       ((I - kappa j j')^2 = I - c j j')
it is the normal-equation system of the EQUIVALENT Jacobian X~ = X - kappa j (j'X) and residual
r~ = (I - kappa j j')^-1 (r - gamma j): H = JS'JS and b = JS'r~, which is what oracle.LMSystem carries."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

LD = np.longdouble


def _indices(og):
    E, N = og.n_edges, og.n_poses
    ia, ib = np.asarray(og.ia, np.int64), np.asarray(og.ib, np.int64)
    sc = np.nonzero(np.asarray(og.kind) != 0)[0]
    M = len(sc)
    rows_p = np.repeat(np.arange(3 * E).reshape(E, 3), 6, axis=1).reshape(-1)
    cols_p = np.concatenate([3 * ia[:, None] + np.arange(3), 3 * ib[:, None] + np.arange(3)], axis=1)
    cols_p = np.tile(cols_p, (1, 3)).reshape(-1)
    rows_s = (3 * sc[:, None] + np.arange(3)).reshape(-1)
    cols_s = np.repeat(3 * N + np.arange(M), 3)
    rows = np.concatenate([rows_p, rows_s, 3 * E + np.arange(M)])
    cols = np.concatenate([cols_p, cols_s, 3 * N + np.arange(M)])
    return sc, M, rows, cols


def joint_jacobian(O, og, poses, switches, lam, delta=0.01, threads=1):
    """(cost, A, rvec, j): the joint Jacobian [3E + M, 3N + M] (pose columns, one switch column per robust edge, the prior rows
    -sqrt(lambda)), loss applied, the residual vector [r; q] and j = d e / d s of the robust edges [M, 3]"""
    E, N = og.n_edges, og.n_poses
    sc, M, rows, cols = _indices(og)
    cost, r, J, Js, q = O.evaluate_sc(og, np.asarray(poses, np.float64).reshape(N, 3), switches, lam, delta, True, True, threads)
    vals = np.concatenate([J.reshape(-1), Js[sc].reshape(-1), np.full(M, -np.sqrt(lam))])
    A = sp.csr_matrix((vals, (rows, cols)), shape=(3 * E + M, 3 * N + M))
    return cost, A, np.concatenate([r.reshape(-1), q[sc]]), Js[sc].copy()


def column_scales(O, og, poses0, lam, fixed, jacobi_scaling=1, delta=0.01, threads=1):
    """Ceres' Jacobi scaling, from the Jacobian of iteration 0 (poses0, switches 1): 1 / (1 + column norm); for a switch column
    that is 1 / (1 + sqrt(|j|^2 + lambda)).  0 on the constant pose (its columns are dropped).  jacobi_scaling = 0: ones."""
    N = og.n_poses
    _, A0, _, _ = joint_jacobian(O, og, poses0, None, lam, delta, threads)
    s = 1.0 / (1.0 + np.sqrt(np.asarray(A0.multiply(A0).sum(axis=0)).reshape(-1))) if jacobi_scaling else np.ones(A0.shape[1])
    if fixed >= 0:
        s[3 * fixed:3 * fixed + 3] = 0.0
    return s


def joint_system(O, og, poses, switches, poses0, radius, lam, fixed, jacobi_scaling=1, radius_elim=None, min_diag=1e-6,
                 max_diag=1e32, delta=0.01, threads=1):
    """The joint LM system at the state (poses, switches, radius) and the reduced pose system the kernels solve.
    D'D = clip(diag) / radius on the UNREDUCED column norms (1 on the constant pose); radius_elim (default: radius) is the radius
    of the switch block alone -- after a rejected step the handle keeps the elimination of the previous radius under the LM
    diagonal of the current one until the next iteration re-assembles; pgo_debug_system_spmv and pgo_debug_direct_solve both
    see that system (include/pgo.h, in the comment on pgo_debug_direct_solve).
    Returns a namespace: A, rhs (the joint system, CSR), AS, rvec, s, d2 (joint), sysm (oracle.LMSystem of the reduced pose
    system: H without the LM diagonal, d2, b, s, JS the equivalent Jacobian [3E, 3N]), r_tilde [3E], the per-edge sc (edge
    indices), j, sigma, hss, den, gs, c, gamma, and cost."""
    N, E = og.n_poses, og.n_edges
    re = radius if radius_elim is None else radius_elim
    sc, M, _, _ = _indices(og)
    s = column_scales(O, og, poses0, lam, fixed, jacobi_scaling, delta, threads)
    sw = np.ones(E) if switches is None else np.asarray(switches, np.float64)
    cost, Aj, rvec, j = joint_jacobian(O, og, poses, sw, lam, delta, threads)
    AS = (Aj @ sp.diags(s)).tocsr()
    Hj = (AS.T @ AS).tocsr()
    diag = np.clip(Hj.diagonal(), min_diag, max_diag)
    d2 = diag / radius
    d2[3 * N:] = diag[3 * N:] / re
    if fixed >= 0:
        d2[3 * fixed:3 * fixed + 3] = 1.0
    A = (Hj + sp.diags(d2)).tocsr()
    rhs = AS.T @ rvec
    # ---- the switches eliminated: A_ss is diagonal, so the Schur complement stays sparse
    sigma = s[3 * N:]
    hss = Hj.diagonal()[3 * N:]
    den = hss + d2[3 * N:]
    gs = rhs[3 * N:]
    A_ps = Hj[:3 * N, 3 * N:].tocsr()
    H_red = (Hj[:3 * N, :3 * N] - A_ps @ sp.diags(1.0 / den) @ A_ps.T).tocsr() if M else Hj[:3 * N, :3 * N].tocsr()
    b_red = rhs[:3 * N] - (A_ps @ (gs / den) if M else 0.0)
    c = sigma * sigma / den
    gamma = sigma * gs / den
    # ---- the equivalent Jacobian and residual
    n2 = (j * j).sum(axis=1)
    w = np.sqrt(1.0 - c * n2)                 # (c |j|^2 < 1: den > sigma^2 |j|^2 as long as lambda > 0)
    kap = c / (1.0 + w)
    er = (3 * sc[:, None, None] + np.arange(3)[None, :, None] + np.zeros((1, 1, 3), np.int64)).reshape(-1)
    ec = (3 * sc[:, None, None] + np.arange(3)[None, None, :] + np.zeros((1, 3, 1), np.int64)).reshape(-1)
    jj = j[:, :, None] * j[:, None, :]
    K = (sp.identity(3 * E, format="csr") - sp.csr_matrix(((kap[:, None, None] * jj).reshape(-1), (er, ec)), shape=(3 * E, 3 * E))).tocsr()
    Kinv = (sp.identity(3 * E, format="csr") + sp.csr_matrix((((kap / w)[:, None, None] * jj).reshape(-1), (er, ec)), shape=(3 * E, 3 * E))).tocsr()
    JS = (K @ AS[:3 * E, :3 * N]).tocsr()
    rg = rvec[:3 * E].copy()
    rg[(3 * sc[:, None] + np.arange(3)).reshape(-1)] -= (gamma[:, None] * j).reshape(-1)
    r_tilde = Kinv @ rg
    sysm = O.LMSystem(H_red, d2[:3 * N].copy(), np.asarray(b_red).reshape(-1), s[:3 * N].copy(), JS)
    return SimpleNamespace(N=N, E=E, M=M, sc=sc, A=A, rhs=rhs, AS=AS, rvec=rvec, s=s, d2=d2, sysm=sysm, r_tilde=r_tilde, j=j,
                           sigma=sigma, hss=hss, den=den, gs=gs, c=c, gamma=gamma, cost=cost, A_ps=A_ps, fixed=fixed, lam=lam)


def unscaled_reduced(O, og, poses, switches, poses0, radius, lam, fixed, jacobi_scaling=1, min_diag=1e-6, max_diag=1e32,
                     delta=0.01, threads=1):
    """(g [3N], hdiag [N, 9]): P'(r - gamma j) and the diagonal 3x3 blocks of P'(I - c j j')P, P the pose columns of the Jacobian
    with UNIT pose scales (0 on the constant pose) and c, gamma those of the state's own assembly (the switch scales stay) --
    what Solver.normal_eq() returns on a METHOD 2 handle"""
    S = joint_system(O, og, poses, switches, poses0, radius, lam, fixed, jacobi_scaling, None, min_diag, max_diag, delta, threads)
    N, E, sc = S.N, S.E, S.sc
    _, Aj, rvec, j = joint_jacobian(O, og, poses, switches, lam, delta, threads)
    unit = np.ones(3 * N)
    if fixed >= 0:
        unit[3 * fixed:3 * fixed + 3] = 0.0
    P = (Aj[:3 * E, :3 * N] @ sp.diags(unit)).tocsr()
    rg = rvec[:3 * E].copy()
    rows = (3 * sc[:, None] + np.arange(3)).reshape(-1)
    rg[rows] -= (S.gamma[:, None] * j).reshape(-1)
    V = sp.csr_matrix((j.reshape(-1), (np.repeat(np.arange(S.M), 3), rows)), shape=(S.M, 3 * E)) @ P     # row e: j'P
    H = (P.T @ P - V.T @ sp.diags(S.c) @ V).tocsr()
    hd = np.stack([H[3 * i:3 * i + 3, 3 * i:3 * i + 3].toarray().reshape(-1) for i in range(N)])
    return P.T @ rg, hd


def gradient(O, og, poses, switches, lam, fixed, delta=0.01, threads=1):
    """the unscaled joint gradient A'r at a state: namespace with pose_max, switch_max, gmax (over the free poses and the
    switches), g2 = |A'r|_2, a_norm = |A|_2, r_norm = |r|_2"""
    N = og.n_poses
    _, A, rvec, _ = joint_jacobian(O, og, poses, switches, lam, delta, threads)
    g = A.T @ rvec
    if fixed >= 0:
        g[3 * fixed:3 * fixed + 3] = 0.0
    pm = float(np.abs(g[:3 * N]).max())
    sm = float(np.abs(g[3 * N:]).max()) if len(g) > 3 * N else 0.0
    return SimpleNamespace(pose_max=pm, switch_max=sm, gmax=max(pm, sm), g2=float(np.linalg.norm(g)), a_norm=norm2_bound(A),
                           r_norm=float(np.linalg.norm(rvec)))


def norm2_bound(A):
    """sqrt(|A|_1 |A|_inf) >= |A|_2"""
    B = abs(sp.csr_matrix(A))
    return float(np.sqrt(B.sum(axis=0).max() * B.sum(axis=1).max())) if B.nnz else 0.0


def _solve(A, b):
    """A^-1 b for a dense symmetric positive definite A, one step of iterative refinement with the residual in longdouble"""
    y = np.linalg.solve(A, b)
    res = (b.astype(LD) - A.astype(LD) @ y.astype(LD)).astype(np.float64)
    return y + np.linalg.solve(A, res)


def cond2(A):
    ev = np.linalg.eigvalsh(A.toarray() if sp.issparse(A) else A)
    return float(ev[-1] / ev[0])


QUANTITIES = ("step_norm", "model", "cost_change", "rho", "gmax")


def joint_step(O, og, poses, switches, poses0, radius, lam, fixed, jacobi_scaling=1, min_diag=1e-6, max_diag=1e32,
               min_relative_decrease=1e-3, ftol=1e-6, ptol=1e-8, delta=0.01, threads=1):
    """One LM step from the state (poses, switches, radius), by two routes: the joint solve, and the reduced pose solve followed by
    the back-substitution of the switches (its residual in numpy.longdouble).  Returns a namespace with, from the JOINT route:
    cand_poses, cand_switches, step_norm (over poses and switches), model = -m.(r + m/2) with m = -(A S) y, cost, cand_cost,
    cost_change, rho, valid (finite and model > 0), term (0, or Ceres' 3 = PTOL / 1 = FTOL when the step ends the solve),
    step_ok (rho > min_relative_decrease; False when term), gmax (at the candidate), and
      delta_ref[q]   |q_joint - q_reduced| for q in QUANTITIES and for "vector" (largest entry of the step vectors' difference),
      kappa          cond_2 of the reduced pose system,  kappa_joint  of the joint one,
      sens[q]        first-order change of q per unit of |dy|_2 (step_tolerances),
      y_norm         |y|_2 of the pose part,  backsub  an upper bound of |A_ss^-1 A_sp|_2 (norm2_bound),
      S              the joint_system."""
    S = joint_system(O, og, poses, switches, poses0, radius, lam, fixed, jacobi_scaling, None, min_diag, max_diag, delta, threads)
    N, M, sc = S.N, S.M, S.sc
    poses = np.asarray(poses, np.float64).reshape(N, 3)
    sw = np.ones(S.E) if switches is None else np.asarray(switches, np.float64)
    Ad = S.A.toarray()
    Ar = (S.sysm.H + sp.diags(S.sysm.d2)).toarray()
    y_joint = _solve(Ad, S.rhs)
    yp = _solve(Ar, S.sysm.b)
    # back-substitution: y_s = (g_s - A_sp y_p) / den, the residual in longdouble
    t = (S.A_ps.T.toarray().astype(LD) @ yp.astype(LD)) if M else np.zeros(0, LD)
    ys = ((S.gs.astype(LD) - t) / S.den.astype(LD)).astype(np.float64)
    y_red = np.concatenate([yp, ys])
    free = S.s > 0.0
    z = np.concatenate([poses.reshape(-1), sw[sc]])
    x_norm = float(np.linalg.norm(z[free]))

    def quantities(y):
        d = -S.s * y
        cp = poses + d[:3 * N].reshape(N, 3)
        cs = sw.copy()
        cs[sc] = sw[sc] + d[3 * N:]
        m = (S.AS @ (-y)).astype(LD)
        model = float(-(m @ (S.rvec.astype(LD) + 0.5 * m)))
        cc_ = O.evaluate_sc(og, cp, cs, lam, delta, True, False, threads)[0]
        if not np.isfinite(cc_):
            cc_ = np.finfo(np.float64).max
        G = gradient(O, og, cp, cs, lam, fixed, delta, threads)
        return SimpleNamespace(y=y, d=d, cand_poses=cp, cand_switches=cs, step_norm=float(np.linalg.norm(d)), model=model,
                               cand_cost=cc_, cost_change=S.cost - cc_, rho=(S.cost - cc_) / model, gmax=G.gmax, G=G)

    qj, qr = quantities(y_joint), quantities(y_red)
    out = qj
    out.S, out.cost, out.x_norm = S, S.cost, x_norm
    out.reduced = qr
    out.delta_ref = {q: abs(getattr(qj, q) - getattr(qr, q)) for q in QUANTITIES}
    out.delta_ref["vector"] = float(np.abs(qj.d - qr.d).max())
    out.valid = bool(np.isfinite(y_joint).all() and qj.model > 0.0)
    out.term = 0
    if out.valid and qj.step_norm <= ptol * (x_norm + ptol):
        out.term = 3
    elif out.valid and abs(qj.cost_change) <= ftol * S.cost:
        out.term = 1
    out.step_ok = bool(out.valid and not out.term and qj.rho > min_relative_decrease)
    out.kappa, out.kappa_joint = cond2(Ar), cond2(Ad)
    out.y_norm = float(np.linalg.norm(yp))
    out.backsub = norm2_bound(sp.diags(1.0 / S.den) @ S.A_ps.T) if M else 0.0
    # first-order sensitivities to an error dy of the joint scaled solution (|dy|_2 = 1):
    #   vectors, step_norm   d = -S y with s <= 1:                        |dd| <= |dy|
    #   model                y.b - y'Hy / 2 has the gradient b - H y = D'D y at the LM solution (H without the LM diagonal)
    #   cost_change          cost(x + d): the gradient of the cost at the candidate, |A'r|_2 there
    #   gmax                 d (A'r) = A'A dx + dA'r, and |dA| <= |A| |dx| for this edge model (the derivatives of the
    #                        Jacobian's entries by the headings are entries of the Jacobian again)
    out.sens = {"vector": 1.0, "step_norm": 1.0, "model": float(np.linalg.norm(S.d2 * y_joint)), "cost_change": qj.G.g2,
                "gmax": qj.G.a_norm ** 2 + qj.G.a_norm * qj.G.r_norm}
    return out


RATIO = 10.0       # test_gpu_direct.py's: the difference in norms and the summation order
FLOOR = 1e-12      # relative


def accepted_radius(radius, rho, max_radius=1e16):
    return min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))


def step_tolerances(st, rel_residual, radius=None, max_radius=1e16):
    """Absolute tolerance per quantity of joint_step's result for a step whose linear solve reports the relative residual
    rel_residual = |b - A y| / |b|:  RATIO x (delta_ref(q) + sens(q) |dy|), at least FLOOR relative, where
      |dy|_2 <= sqrt(1 + |A_ss^-1 A_sp|^2) kappa rel_residual |y_p|_2
    -- the pose solve is off by at most kappa rel_residual relative, and the switches follow from the poses through the
    back-substitution y_s = A_ss^-1 (g_s - A_sp y_p).  cost_change is a difference of two costs and is bounded relative to the
    current cost; rho = cost_change / model follows from those two; the radius after an accepted step from rho."""
    dy = np.sqrt(1.0 + st.backsub ** 2) * st.kappa * rel_residual * st.y_norm
    scale = {"vector": max(1.0, float(np.abs(st.cand_poses).max())), "step_norm": st.step_norm, "model": abs(st.model),
             "cost_change": st.cost, "gmax": st.gmax}
    tol = {q: max(RATIO * (st.delta_ref[q] + st.sens[q] * dy), FLOOR * scale[q]) for q in scale}
    tol["rho"] = max(RATIO * st.delta_ref["rho"] + (tol["cost_change"] + abs(st.rho) * tol["model"]) / abs(st.model), FLOOR * abs(st.rho))
    if radius is not None:
        r0 = accepted_radius(radius, st.rho, max_radius)
        tol["radius"] = max(abs(accepted_radius(radius, st.rho + sgn * tol["rho"], max_radius) - r0) for sgn in (-1.0, 1.0))
        tol["radius"] = max(tol["radius"], FLOOR * r0)
    return tol
