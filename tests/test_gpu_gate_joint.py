"""pgo_edge_gate_joint on the GPU: the joint covariance P_full = [J_j Sigma J_k'] of all candidates from one covariance solve
(k_gate_cross after every pass, k_gate_symmetrise) and the sequential elimination on it (k_gate_joint_step).

References: Sigma's cross matrix by the sparse direct inverse of test_gpu_gate.py (its helpers are copied below, as that file
copied its own), r and J of a candidate by oracle.edge(dcs=False); the elimination by the host statement
(gate_joint_evaluate) and by the numpy elimination of test_gate_joint_host.py.

Tolerances (none is fitted to the code under test):
  P_full block (j, k)   BLOCK_REL |J_j|_2 |J_k|_2 |Sigma_[ab_j, ab_k]|_F: the suite's per-block bound on Sigma pushed through both Jacobians
  device against host   the rule of test_gate_joint_host.py, from numpy's float64 and longdouble eliminations of the device's own P_full
  against a live handle first-order propagation of the block bound through the downdate (test_against_the_live_handle)
  two variants of one solve: VARIANT = 1e-9 relative to the largest entry, as test_gpu_gate.py"""
import os

import numpy as np
import pytest

from conftest import DATA, oracle_graph
from test_gate_joint_host import CHI2_95, compare, eliminate, tolerances

pytestmark = pytest.mark.gpu

BLOCK_REL = 1e-7     # test_gpu_covariance.py: per-block relative Frobenius error against the sparse direct inverse
VARIANT = 1e-9       # test_gpu_covariance.py: agreement of two variants of the same solve, relative to the largest entry
EPS = np.finfo(np.float64).eps
FIELDS = ("r", "J", "P", "chi2", "chi2_marginal", "info_gain")
JFIELDS = ("r_cond", "P_cond", "chi2_cond", "info_gain_cond")


# ----------------------------------------------------------------------------------- helpers copied from test_gpu_gate.py
def load(pgo, name, n_out=0, seed=1):
    g = pgo.ReadG2O(os.path.join(DATA, name + ".g2o"))
    if n_out:
        g.add_random_C(n_out, seed)
    return g


def normal_matrix(O, og, poses, method, fixed=0, apply_loss=True):
    """(J'J with the constant pose removed as a sparse LU, keep mask, position of every kept row)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl

    N, E = og.n_poses, og.n_edges
    ia, ib = np.asarray(og.ia), np.asarray(og.ib)
    _, _, J = O.evaluate(og, poses, method=method, apply_loss=apply_loss)
    rows = np.repeat(np.arange(3 * E).reshape(E, 3), 6, axis=1).reshape(-1)
    cols = np.concatenate([3 * ia[:, None] + np.arange(3), 3 * ib[:, None] + np.arange(3)], axis=1)
    cols = np.tile(cols, (1, 3)).reshape(-1)
    Jp = sp.csr_matrix((J.reshape(-1), (rows, cols)), shape=(3 * E, 3 * N)).tocsc()
    H = (Jp.T @ Jp).tocsc()
    keep = np.ones(H.shape[0], bool)
    keep[3 * fixed:3 * fixed + 3] = False
    pos = -np.ones(H.shape[0], np.int64)
    pos[keep] = np.arange(keep.sum())
    return spl.splu(H[keep][:, keep].tocsc()), keep, pos


def reference_cross(O, og, poses, idx, method, fixed=0, apply_loss=True):
    """Sigma's (3n x 3n) cross matrix over the poses idx by a sparse LU of J'J -- test_gpu_gate.reference_blocks(cross=True)"""
    lu, keep, pos = normal_matrix(O, og, poses, method, fixed, apply_loss)
    idx = np.asarray(idx)
    n = idx.size
    rhs = np.zeros((keep.sum(), 3 * n))
    for j, i in enumerate(idx):
        for c in range(3):
            if i != fixed:
                rhs[pos[3 * i + c], 3 * j + c] = 1.0
    X = lu.solve(rhs)
    full = np.zeros((keep.size, 3 * n))
    full[keep] = X
    M = full[(3 * idx[:, None] + np.arange(3)).reshape(-1)]
    return 0.5 * (M + M.T)


def candidates(rng, poses, n, noise=0.05, lo=0):
    """n random pairs a != b with the measurement the current estimate predicts, plus noise"""
    N = len(poses)
    ia = rng.integers(lo, N, n)
    ib = rng.integers(lo, N, n)
    ib = np.where(ib == ia, (ib + 1 - lo) % (N - lo) + lo, ib)
    meas = np.zeros((n, 3))
    for k in range(n):
        pa, pb = poses[ia[k]], poses[ib[k]]
        c, s = np.cos(pa[2]), np.sin(pa[2])
        d = pb[:2] - pa[:2]
        th = pb[2] - pa[2]
        meas[k] = [c * d[0] + s * d[1], -s * d[0] + c * d[1], np.arctan2(np.sin(th), np.cos(th))]
    return ia.astype(np.int32), ib.astype(np.int32), meas + noise * rng.standard_normal((n, 3))


def subgraph(pgo, g, n):
    """the first n poses of g and the edges among them"""
    ia, ib = np.array(g.ia), np.array(g.ib)
    m = (ia < n) & (ib < n)
    return pgo.Graph.from_arrays(np.array(g.poses)[:n], ia[m], ib[m], np.array(g.meas)[m], np.array(g.kind)[m], np.array(g.info)[m])


def full_info(w):
    a, b, c, d, e, f = w
    return np.array([[a, b, c], [b, d, e], [c, e, f]])


def same_bits(a, b, fields):
    for f in fields:
        assert np.array_equal(a[f], b[f], equal_nan=True), f


def blocks(P, n):
    return np.stack([P[3 * k:3 * k + 3, 3 * k:3 * k + 3] for k in range(n)])


def joint_reference(O, poses, ia, ib, meas, sigma, uniq):
    """(J as a dense 3n x 3|uniq| matrix from oracle.edge, P_ref = J Sigma J', the per-block bounds (n x n))"""
    at = {int(p): j for j, p in enumerate(uniq)}
    n = len(ia)
    J = np.zeros((3 * n, 3 * len(uniq)))
    rows6, norms = [], np.zeros(n)
    for k in range(n):
        _, Jk = O.edge(poses[ia[k]], poses[ib[k]], meas[k], dcs=False)
        a, b = at[int(ia[k])], at[int(ib[k])]
        J[3 * k:3 * k + 3, 3 * a:3 * a + 3] = Jk[:, :3]
        J[3 * k:3 * k + 3, 3 * b:3 * b + 3] = Jk[:, 3:]
        rows6.append(np.concatenate([3 * a + np.arange(3), 3 * b + np.arange(3)]))
        norms[k] = np.linalg.norm(Jk, 2)
    bound = np.zeros((n, n))
    for j in range(n):
        for k in range(n):
            bound[j, k] = BLOCK_REL * norms[j] * norms[k] * np.linalg.norm(sigma[np.ix_(rows6[j], rows6[k])])
    return J, J @ sigma @ J.T, bound


def check_blocks(P, P_ref, bound, label):
    n = bound.shape[0]
    d = np.array([[np.linalg.norm((P - P_ref)[3 * j:3 * j + 3, 3 * k:3 * k + 3]) for k in range(n)] for j in range(n)])
    print(f"{label}: worst block error / bound = {(d / bound).max():.3e} over {n * n} blocks")
    assert (d <= bound).all(), (label, np.unravel_index(np.argmax(d / bound), d.shape), (d / bound).max())


# ---------------------------------------------------------------------------------------------- the shared case 1
@pytest.fixture(scope="module")
def case1(pgo, oracle):
    """a handle on INTEL (METHOD 1, 5 LM iterations) and the 50 loops add_random_C(50, 1) appends to a second copy: the joint call
    by PCG, 16 candidates per pass (4 passes: blocks across passes), and by the direct solve (one pass); the reference once"""
    g = load(pgo, "INTEL")
    g2 = load(pgo, "INTEL", 50)
    E = g.n_edges
    ia, ib, meas, info = (np.array(x[E:]) for x in (g2.ia, g2.ib, g2.meas, g2.info))
    assert len(ia) == 50
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.solve()
    assert s.info().linear_solver == 2
    poses = s.poses()
    uniq = np.unique(np.concatenate([ia, ib]))
    sigma = reference_cross(oracle, oracle_graph(oracle, g), poses, uniq, 1)
    J, P_ref, bound = joint_reference(oracle, poses, ia, ib, meas, sigma, uniq)
    runs = {"pcg": dict(solver=0, poses_per_pass=16), "direct": dict(solver=1)}
    c = dict(s=s, ia=ia, ib=ib, meas=meas, info=info, P_ref=P_ref, bound=bound, runs=runs)
    for name, opts in runs.items():
        c[name] = s.gate_joint(ia, ib, meas, full=True, **opts)
    yield c
    s.close()


# ------------------------------------------------------------------------------------------------- 1. parity of P_full
@pytest.mark.parametrize("run", ["pcg", "direct"])
def test_p_full_parity(pgo, case1, run):
    c = case1
    out, joint, rep = c[run]
    assert rep["passes"] == (4 if run == "pcg" else 1) and rep["columns"] == 150, rep
    check_blocks(joint["P_full"], c["P_ref"], c["bound"], f"INTEL m1, 50 loops, {run}")
    ref, _ = c["s"].gate(c["ia"], c["ib"], c["meas"], **c["runs"][run])
    same_bits(out, ref, FIELDS + ("status",))
    assert np.array_equal(blocks(joint["P_full"], 50), out["P"])
    assert np.array_equal(joint["P_full"], joint["P_full"].T)
    assert np.linalg.eigvalsh(joint["P_full"]).min() > -64 * EPS * np.linalg.norm(joint["P_full"], 2)


# --------------------------------------------------------------------------- 2. the device elimination against the host's
def searched_gate(r, P, W):
    """a chi2 gate at which the numpy reference accepts between a quarter and three quarters of the candidates, clear of every
    chi2_cond by 1e-6 relative: searched over the midpoints of the sorted chi2_cond of the all-rejecting run"""
    n = len(W)
    base = np.sort(eliminate(r, P, W, None, np.zeros(n, int))["chi2_cond"])
    for gate in 0.5 * (base[:-1] + base[1:])[n // 4:]:
        ref = eliminate(r, P, W, None, None, gate)
        acc = int(ref["accepted"].sum())
        if n / 4 <= acc <= 3 * n / 4 and (np.abs(ref["chi2_cond"] - gate) > 1e-6 * gate).all():
            return float(gate)
    raise AssertionError("no chi2 gate splits the candidates")


@pytest.mark.parametrize("run, own_info", [("pcg", False), ("direct", False), ("direct", True)])
def test_device_elimination_against_the_host_statement(pgo, case1, run, own_info):
    c = case1
    s, ia, ib, meas = c["s"], c["ia"], c["ib"], c["meas"]
    w = c["info"] if own_info else None
    W = [full_info(x) for x in w] if own_info else [np.eye(3)] * 50
    out, joint, _ = c[run] if not own_info else s.gate_joint(ia, ib, meas, w, full=True, **c["runs"][run])
    P, r = joint["P_full"], out["r"]
    gates = [CHI2_95, searched_gate(r, P, W)]
    for gate in gates:
        got = joint if (gate == CHI2_95 and not own_info) else s.gate_joint(ia, ib, meas, w, chi2_gate=gate, **c["runs"][run])[1]
        ref64, refld = eliminate(r, P, W, None, None, gate), eliminate(r, P, W, None, None, gate, dtype=np.longdouble)
        assert (np.abs(ref64["chi2_cond"] - gate) > 1e-6 * gate).all() and (ref64["info_gain_cond"] > 1e-6).all()
        host = pgo.gate_joint_evaluate(r, P, w, out["status"], None, gate)
        tol = tolerances(ref64, refld, P)
        compare(got, ref64, tol, f"{run}, own information {own_info}, chi2_gate {gate:.6g}: device against numpy")
        compare(got, host, tol, f"{run}, own information {own_info}, chi2_gate {gate:.6g}: device against host")
        assert np.array_equal(got["accepted"], host["accepted"]) and np.array_equal(got["accepted"], ref64["accepted"])
        assert got["n_accepted"] == host["n_accepted"] == ref64["accepted"].sum()
        print(f"  accepted {got['n_accepted']} of 50")
    assert 50 / 4 <= got["n_accepted"] <= 3 * 50 / 4


# --------------------------------------------------------------------------------------- 3. against the live handle
def test_against_the_live_handle(pgo, oracle):
    """INTEL + 50 in ONE graph, METHOD 0, Trivial loss, the 50 bogus edges inactive; they are the candidates, Omega = I.  The first
    5 evaluable ones are forced in (set A), the others rejected; then set_active makes A residual blocks and the independent gate
    judges the other 45 at the same poses: its P[k] is P_cond[k], its r is unchanged and r_cond[k] = r_k + J_k delta, delta the
    Gauss-Newton step of the augmented problem.

    Bounds.  Q is the joint block matrix over {k} u A, S = Q_AA + I, G_k = Q_kA S^-1, so P_cond[k] = Q_kk - Q_kA S^-1 Q_Ak.  An
    error E in Q moves it, to first order, by E_kk - E_kA G_k' - G_k E_Ak + G_k E_AA G_k' = [I, -G_k] E [I, -G_k]', hence
    |dP_cond|_F <= (1 + |G_k|_2)^2 |E|_F with |E|_F <= b_k, the root-sum-square of the parity bounds of test_p_full_parity over
    the blocks of {k} u A.  In the same way r_cond[k] = r_k - G_k r_A moves by -(E_kA - G_k E_AA) S^-1 r_A:
    |dr_cond| <= (1 + |G_k|_2) b_k |S^-1 r_A|_2, plus the 1e-11 per component the suite holds r itself to."""
    g = load(pgo, "INTEL", 50)
    g0 = load(pgo, "INTEL")
    E, N = g0.n_edges, g.n_poses
    ia, ib, meas = (np.array(x[E:]) for x in (g.ia, g.ib, g.meas))
    active = np.ones(g.n_edges, bool)
    active[E:] = False
    s = pgo.Solver(g, pgo.Options(method=0, max_iters=5, huber_delta=0.0))
    s.set_active(active)
    s.solve()
    poses = s.poses()
    opts = dict(solver=1) if s.info().linear_solver == 2 else dict(poses_per_pass=16)
    ind, _ = s.gate(ia, ib, meas, **opts)
    A = np.nonzero(ind["status"] == 0)[0][:5]
    rest = np.setdiff1d(np.arange(50), A)
    force = np.zeros(50, np.int8)
    force[A] = 1
    out, joint, _ = s.gate_joint(ia, ib, meas, force=force, full=True, **opts)
    assert joint["n_accepted"] == 5 and joint["accepted"][A].all()
    active[E + A] = True
    s.set_active(active)
    s.set_poses(poses)
    live, _ = s.gate(ia[rest], ib[rest], meas[rest], **(dict(solver=1) if s.info().linear_solver == 2 else dict(poses_per_pass=16)))
    assert np.array_equal(s.poses(), poses)
    # the reference: Sigma of the problem WITHOUT the bogus edges, plain Jacobians
    uniq = np.unique(np.concatenate([ia, ib]))
    og0 = oracle_graph(oracle, g0)
    sigma = reference_cross(oracle, og0, poses, uniq, 0, apply_loss=False)
    J, P_ref, bound = joint_reference(oracle, poses, ia, ib, meas, sigma, uniq)
    check_blocks(joint["P_full"], P_ref, bound, "INTEL + 50 m0 Trivial, bogus edges inactive")
    rowsA = (3 * A[:, None] + np.arange(3)).reshape(-1)
    S = P_ref[np.ix_(rowsA, rowsA)] + np.eye(15)
    rA = np.array([oracle.edge(poses[ia[a]], poses[ib[a]], meas[a], dcs=False)[0] for a in A]).reshape(-1)
    SirA = np.linalg.solve(S, rA)
    # delta of the augmented normal equations (Lambda + J_A' J_A) delta = -J_A' r_A by a sparse solve
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    keep_e = np.concatenate([np.arange(E), E + A])
    og1 = oracle.Graph(np.array(g.pose_ids), np.array(g.poses), np.array(g.ia)[keep_e], np.array(g.ib)[keep_e], np.array(g.meas)[keep_e],
                       np.array(g.info)[keep_e], np.array(g.kind)[keep_e])
    lu, keep, pos = normal_matrix(oracle, og1, poses, 0, apply_loss=False)
    rhs = np.zeros(3 * N)
    for a in A:
        ra, Ja = oracle.edge(poses[ia[a]], poses[ib[a]], meas[a], dcs=False)
        rhs[3 * ia[a]:3 * ia[a] + 3] -= Ja[:, :3].T @ ra
        rhs[3 * ib[a]:3 * ib[a] + 3] -= Ja[:, 3:].T @ ra
    delta = np.zeros(3 * N)
    delta[keep] = lu.solve(rhs[keep])
    worst_P = worst_r = 0.0
    for j, k in enumerate(rest):
        rows = 3 * k + np.arange(3)
        G = np.linalg.solve(S, P_ref[np.ix_(rowsA, rows)]).T
        both = np.concatenate([[k], A])
        b = np.sqrt((bound[np.ix_(both, both)] ** 2).sum())
        g2 = 1 + np.linalg.norm(G, 2)
        dP = np.linalg.norm(live["P"][j] - joint["P_cond"][k])
        assert dP <= g2 ** 2 * b, (k, dP, g2 ** 2 * b)
        rk, Jk = oracle.edge(poses[ia[k]], poses[ib[k]], meas[k], dcs=False)
        r_ref = rk + Jk[:, :3] @ delta[3 * ia[k]:3 * ia[k] + 3] + Jk[:, 3:] @ delta[3 * ib[k]:3 * ib[k] + 3]
        dr = np.linalg.norm(joint["r_cond"][k] - r_ref)
        tol_r = g2 * b * np.linalg.norm(SirA) + 3e-11   # (+ the 1e-11 per component r itself is held to)
        assert dr <= tol_r, (k, dr, tol_r)
        worst_P, worst_r = max(worst_P, dP / (g2 ** 2 * b)), max(worst_r, dr / tol_r)
    print(f"live handle: worst |P - P_cond| / bound = {worst_P:.3e}, worst |r_cond - (r + J delta)| / bound = {worst_r:.3e}")
    s.close()


# --------------------------------------------------------------------------------------------------- 4. smallest shapes
@pytest.fixture(scope="module", params=["pcg", "direct"])
def small(pgo, request):
    """subgraph(INTEL, 300): a PCG handle; MIT: a handle on the direct solve, solver = 1"""
    if request.param == "pcg":
        g = subgraph(pgo, load(pgo, "INTEL"), 300)
        opts = dict(poses_per_pass=16)
    else:
        g = load(pgo, "MIT")
        opts = dict(solver=1)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5, linear_solver=1 if request.param == "pcg" else 0))
    s.solve()
    assert s.info().linear_solver == (2 if request.param == "direct" else 1)
    yield s, opts, g
    s.close()


def host_agrees(pgo, out, joint, force=None, info=None):
    host = pgo.gate_joint_evaluate(out["r"], joint["P_full"], info, out["status"], force, np.inf)
    assert np.array_equal(host["accepted"], joint["accepted"]) and np.array_equal(host["status"], joint["status"])
    scale = max(np.nanmax(np.abs(host["P_cond"])), 1e-300)
    for f in JFIELDS:   # two evaluations of one statement on one input: VARIANT is generous, the exact rule is test 2's
        assert np.array_equal(np.isnan(host[f]), np.isnan(joint[f])), f
        assert np.nanmax(np.abs(host[f] - joint[f]), initial=0.0) <= VARIANT * max(np.nanmax(np.abs(host[f]), initial=0.0), scale), f


def test_sizes_1_2_16_17(pgo, small):
    s, opts, g = small
    poses = s.poses()
    ia, ib, meas = candidates(np.random.default_rng(41), poses, 17, lo=1)
    ia[1] = ia[0]                                                 # candidates 0 and 1 share a pose
    ib[1] = ib[0] % (len(poses) - 2) + 1 if ib[0] % (len(poses) - 2) + 1 != ia[0] else ib[0] % (len(poses) - 2) + 2
    for n in (1, 2, 16, 17):
        force = np.ones(n, np.int8)
        out, joint, rep = s.gate_joint(ia[:n], ib[:n], meas[:n], force=force, chi2_gate=np.inf, full=True, **opts)
        assert rep["columns"] == 3 * n and joint["n_accepted"] == n
        if "solver" not in opts:
            assert rep["passes"] == (n + 15) // 16
        ref, _ = s.gate(ia[:n], ib[:n], meas[:n], **opts)
        same_bits(out, ref, FIELDS + ("status",))
        assert np.array_equal(blocks(joint["P_full"], n), out["P"]) and np.array_equal(joint["P_full"], joint["P_full"].T)
        assert joint["chi2_cond"][0] == out["chi2_marginal"][0] and joint["info_gain_cond"][0] == out["info_gain"][0]   # n = 1 is the independent gate
        assert np.array_equal(joint["P_cond"][0], out["P"][0]) and np.array_equal(joint["r_cond"][0], out["r"][0])
        host_agrees(pgo, out, joint, force)
        if n >= 2:
            assert np.abs(joint["P_full"][0:3, 3:6]).max() > 0      # a shared pose: correlated
            assert joint["info_gain_cond"][1] != out["info_gain"][1]
        two, jtwo, _ = s.gate_joint(ia[:n], ib[:n], meas[:n], force=force, chi2_gate=np.inf, full=True, **opts)   # two calls are bitwise equal
        same_bits(joint, jtwo, JFIELDS + ("accepted", "status", "P_full"))
        assert (joint["chi2_joint"], joint["info_gain_joint"]) == (jtwo["chi2_joint"], jtwo["info_gain_joint"])
    pgo.set_knob("gate_joint_shape", 0)     # the other shape of the elimination, one launch of one workgroup: the same bits
    try:
        _, jb, _ = s.gate_joint(ia, ib, meas, force=force, chi2_gate=np.inf, full=True, **opts)
    finally:
        pgo.set_knob("gate_joint_shape", -1)
    same_bits(joint, jb, JFIELDS + ("accepted", "status", "P_full"))


def test_256_runs_and_257_is_refused(pgo, small):
    s, opts, g = small
    ia, ib, meas = candidates(np.random.default_rng(42), s.poses(), 257, lo=1)
    out, joint, rep = s.gate_joint(ia[:256], ib[:256], meas[:256], full=True, **opts)
    assert rep["columns"] == 768 and (joint["status"] == 0).all() and np.isfinite(joint["chi2_cond"]).all()
    assert np.array_equal(blocks(joint["P_full"], 256), out["P"]) and np.array_equal(joint["P_full"], joint["P_full"].T)
    assert joint["n_accepted"] >= 1
    host_agrees(pgo, out, joint)
    with pytest.raises(pgo.PgoError) as e:
        s.gate_joint(ia, ib, meas, **opts)
    assert e.value.status == -8 and "257" in str(e.value)


def test_status_1_constant_endpoints_and_a_duplicate(pgo):
    """the constructions of test_gpu_gate.py: sin delta = -1 exactly (status 1) in the middle of a pass, one and both endpoints
    constant, and the same candidate listed twice"""
    g = subgraph(pgo, load(pgo, "INTEL"), 300)
    N = g.n_poses
    pc = np.zeros(N, bool)
    pc[[200, 201]] = True
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.set_active(None, pc)
    s.solve()
    poses = s.poses()
    poses[[50, 120], 2] = 0.0
    s.set_poses(poses)
    ia, ib, meas = candidates(np.random.default_rng(43), poses, 8, lo=1)
    ia[2], ib[2], meas[2] = 50, 120, [0.1, 0.2, np.pi / 2]      # status 1
    ia[3], ib[3] = 0, 200                                         # both endpoints constant
    ia[4], ib[4] = 200, 77                                        # one endpoint constant
    ia[6], ib[6], meas[6] = ia[1], ib[1], meas[1]                 # a duplicate of candidate 1
    force = np.ones(8, np.int8)
    out, joint, rep = s.gate_joint(ia, ib, meas, force=force, full=True, poses_per_pass=16)
    assert rep["columns"] == 18 and out["status"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    ref, _ = s.gate(ia, ib, meas, poses_per_pass=16)
    same_bits(out, ref, FIELDS + ("status",))
    P = joint["P_full"]
    for k in (2, 3):
        assert not P[3 * k:3 * k + 3, :].any() and not P[:, 3 * k:3 * k + 3].any()
    for f in JFIELDS:
        assert np.isnan(joint[f][2]).all(), f
    assert joint["accepted"].tolist() == [1, 1, 0, 1, 1, 1, 1, 1] and joint["n_accepted"] == 7
    assert np.array_equal(joint["P_cond"][3], np.zeros((3, 3))) and joint["info_gain_cond"][3] == 0.0
    assert abs(joint["chi2_cond"][3] - out["chi2"][3]) <= 16 * EPS * np.sqrt(3.0) * (out["r"][3] @ out["r"][3])
    assert np.array_equal(joint["r_cond"][3], out["r"][3])
    cols = [0, 1, 2, 3, 4, 5, 12, 13, 14, 18, 19, 20]     # the duplicate's rows are the original's (two solves of one column: VARIANT)
    assert np.abs(P[3:6][:, cols] - P[18:21][:, cols]).max() <= VARIANT * np.abs(P).max()
    assert 0 < joint["info_gain_cond"][6] < joint["info_gain_cond"][1]      # the second copy adds less
    host_agrees(pgo, out, joint, force)
    keep = np.array([0, 1, 4, 5, 6, 7])                                     # without the two that change nothing: the same numbers
    _, jk, _ = s.gate_joint(ia[keep], ib[keep], meas[keep], force=force[keep], poses_per_pass=16)
    for f in JFIELDS:
        x, y = joint[f][keep], jk[f]
        assert np.abs(x - y).max() <= VARIANT * np.abs(y).max(), f
    s.close()


def test_pose_ordering_gives_the_same_records(pgo):
    g = load(pgo, "INTEL")
    a = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    a.solve()
    b = pgo.Solver(g, pgo.Options(method=1, max_iters=5, pose_ordering=1))
    assert b.info().pose_ordering == 1
    b.set_poses(a.poses())
    ia, ib, meas = candidates(np.random.default_rng(44), a.poses(), 9)
    force = np.ones(9, np.int8)
    _, ja, _ = a.gate_joint(ia, ib, meas, force=force, full=True, poses_per_pass=16)
    _, jb, _ = b.gate_joint(ia, ib, meas, force=force, full=True, poses_per_pass=16)
    for f in JFIELDS + ("P_full",):
        assert np.abs(ja[f] - jb[f]).max() <= VARIANT * np.abs(ja[f]).max(), f
    a.close(); b.close()


def _records(s):
    return [{k: v for k, v in r.items() if k != "seconds"} for r in s.iter_records()]


@pytest.mark.parametrize("method", [1, 2])
def test_lm_state_is_untouched(pgo, method):
    g = load(pgo, "INTEL", 50)
    o = dict(method=method, max_iters=12)
    ref = pgo.Solver(g, pgo.Options(**o))
    ref.lm_begin()
    ref.lm_step(5)
    ref.lm_step(100)
    s = pgo.Solver(g, pgo.Options(**o))
    s.lm_begin()
    s.lm_step(5)
    ia, ib, meas = candidates(np.random.default_rng(45), s.poses(), 9)
    s.gate_joint(ia, ib, meas, solver=1)
    s.lm_step(100)
    assert np.array_equal(s.poses(), ref.poses())
    assert _records(s) == _records(ref)
    s.close()
    ref.close()


# ------------------------------------------------------------------------------ 5. chain rule and order invariance
@pytest.mark.parametrize("run", ["pcg", "direct"])
def test_chain_rule_and_order_invariance(pgo, case1, run):
    """on the results of case 1: the accepted set's sums against the dense joint forms of the device's own P_full (tolerance 64 eps
    cond relative, as test_gate_joint_host.test_chain_rule), and every candidate forced in, in two orders: the totals agree within
    VARIANT (the two orders solve the same columns in other passes)"""
    c = case1
    s, ia, ib, meas = c["s"], c["ia"], c["ib"], c["meas"]
    out, joint, _ = c[run]
    A = np.nonzero(joint["accepted"])[0]
    assert A.size >= 1
    rows = (3 * A[:, None] + np.arange(3)).reshape(-1)
    PAA, rA = joint["P_full"][np.ix_(rows, rows)], out["r"][A].reshape(-1)
    S = PAA + np.eye(rows.size)
    chi2, gain = rA @ np.linalg.solve(S, rA), 0.5 * np.linalg.slogdet(S)[1]
    assert abs(joint["chi2_joint"] - chi2) <= 64 * EPS * np.linalg.cond(S) * chi2
    assert abs(joint["info_gain_joint"] - gain) <= 64 * EPS * np.linalg.cond(S) * max(1.0, gain)
    assert joint["info_gain_joint"] <= out["info_gain"][A].sum()     # the independent gains count shared information twice
    force = np.ones(50, np.int8)
    p = np.random.default_rng(46).permutation(50)
    _, j1, _ = s.gate_joint(ia, ib, meas, force=force, **c["runs"][run])
    _, j2, _ = s.gate_joint(ia[p], ib[p], meas[p], force=force, **c["runs"][run])
    print(f"{run}: all 50 forced in: chi2_joint {j1['chi2_joint']:.12g} / {j2['chi2_joint']:.12g}, info_gain_joint {j1['info_gain_joint']:.12g} / {j2['info_gain_joint']:.12g}")
    assert abs(j1["chi2_joint"] - j2["chi2_joint"]) <= VARIANT * 50 * j1["chi2_joint"]
    assert abs(j1["info_gain_joint"] - j2["info_gain_joint"]) <= VARIANT * 50 * j1["info_gain_joint"]


# -------------------------------------------------------------------------------------------------------- 6. errors
def test_errors(pgo):
    import ctypes as C
    g = subgraph(pgo, load(pgo, "INTEL"), 300)
    N = g.n_poses
    m = np.array([[0.1, 0.2, 0.3]])
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=1, linear_solver=1))
    assert s.info().linear_solver == 1

    def status(*a, **k):
        with pytest.raises(pgo.PgoError) as e:
            s.gate_joint(*a, **k)
        return e.value.status

    assert status([5], [5], m) == -1                                         # a == b
    assert status([5], [N], m) == -1 and status([-1], [5], m) == -1          # out of range
    assert status([5], [9], m, [[1.0, 2.0, 0, 1.0, 0, 1.0]]) == -1           # not positive definite
    assert status([5], [9], m, force=[2]) == -1 and status([5], [9], m, force=[-2]) == -1
    assert status([5], [9], m, chi2_gate=np.nan) == -1
    assert status([5], [9], m, poses_per_pass=17) == -1
    assert status([5], [9], m, solver=1) == -8                               # a PCG handle: never a fallback
    L = pgo.lib()
    summ = pgo.GateJointSummary()
    assert L.pgo_edge_gate_joint(None, 0, None, None, None, None, None, None, None, None, None, None, C.byref(summ), None) == -1
    assert L.pgo_edge_gate_joint(s._h, 0, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    out, joint, rep = s.gate_joint([], [], np.zeros((0, 3)), full=True)     # n = 0
    assert joint["n_accepted"] == 0 and joint["chi2_joint"] == 0.0 and joint["P_full"].shape == (0, 0) and rep["passes"] == 0
    out, joint, rep = s.gate_joint([5], [9], m)                              # (the handle is still usable)
    assert joint["status"][0] == 0 and rep["columns"] == 3
    s.close()
    for opts in (dict(info_weighting=1), dict(fixed_pose=-1)):
        s = pgo.Solver(g, pgo.Options(method=1, max_iters=1, **opts))
        assert status([5], [9], m) == -8, opts
        s.close()
