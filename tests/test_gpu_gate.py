"""pgo_edge_gate on the GPU: candidate loop edges against the current estimate -- r, J, P = J Sigma_[ab] J', the point and the
innovation chi2 and the exact information gain.

Reference: Sigma by the sparse direct inverse of test_gpu_covariance.py (the helper is copied below), r and J of the
candidate by oracle.edge(dcs=False), P_ref = J Sigma_[ab] J' and the 3x3 algebra in numpy.

Tolerances (none is fitted to the code under test):
  r, J            1e-11 absolute, the tolerance of the K1 parity test
  chi2            16 eps |Omega|_F |r|^2 absolute against the numpy form of the record's own r (a 3-term quadratic form in
                  double precision; r itself is only held to 1e-11)
  P               |P - P_ref|_F <= BLOCK_REL |J|_2^2 |Sigma_[ab]|_F: the suite's per-block bound on Sigma pushed through J . J'
  chi2_marginal   |L'r|^2 |L' dP L|_2 with dP at the P bound: d(v' M^-1 v) = -v' M^-1 dM M^-1 v and |M^-1| <= 1 since M >= I;
                  |L' dP L|_2 <= |Omega|_2 |dP|_F
  info_gain       (sqrt 3 / 2) |L' dP L|_F: d(1/2 logdet M) = 1/2 tr(M^-1 dM) <= 1/2 |M^-1|_F |dM|_F <= (sqrt 3 / 2) |dM|_F;
                  |L' dP L|_F <= |Omega|_2 |dP|_F
  two calls of the library: VARIANT = 1e-9 relative to the largest entry, the suite's bound for two variants of one solve

A batched handle (PGO_ERR_UNSUPPORTED) is not covered: Python reaches a batch only as a pgo_batch_t*, which is not a pgo_t*."""
import os

import numpy as np
import pytest

from conftest import DATA, oracle_graph

pytestmark = pytest.mark.gpu

BLOCK_REL = 1e-7     # test_gpu_covariance.py: per-block relative Frobenius error against the sparse direct inverse
VARIANT = 1e-9       # test_gpu_covariance.py: agreement of two variants of the same solve, relative to the largest entry
EPS = np.finfo(np.float64).eps
FIELDS = ("r", "J", "P", "chi2", "chi2_marginal", "info_gain")


def load(pgo, name, n_out=0, seed=1):
    g = pgo.ReadG2O(os.path.join(DATA, name + ".g2o"))
    if n_out:
        g.add_random_C(n_out, seed)
    return g


def reference_blocks(O, og, poses, idx, method, switches=None, fixed=0, info=False, cross=False):
    """Sigma's blocks at `poses` by a sparse LU of J'J (constant pose removed) -- test_gpu_covariance.reference_blocks"""
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


def full_info(w):
    a, b, c, d, e, f = w
    return np.array([[a, b, c], [b, d, e], [c, e, f]])


def algebra(r, P, W):
    """(chi2, chi2_marginal, info_gain) in numpy"""
    L = np.linalg.cholesky(W)
    M = np.eye(3) + L.T @ P @ L
    v = L.T @ r
    return max(r @ W @ r, 0.0), v @ np.linalg.solve(M, v), 0.5 * np.linalg.slogdet(M)[1]


def sigma_pairs(M, uniq, ia, ib):
    """the 6x6 [a, b] sub-matrices of the cross matrix M over the poses `uniq`"""
    at = {int(p): j for j, p in enumerate(uniq)}
    out = []
    for a, b in zip(ia, ib):
        rows = np.concatenate([3 * at[int(a)] + np.arange(3), 3 * at[int(b)] + np.arange(3)])
        out.append(M[np.ix_(rows, rows)])
    return out


def check_against_reference(O, got, poses, ia, ib, meas, info, sig, label):
    """every candidate's record against oracle.edge and J Sigma_[ab] J'; returns max |dP| / |P|"""
    worst = 0.0
    for k in range(len(ia)):
        r, J = O.edge(poses[ia[k]], poses[ib[k]], meas[k], dcs=False)
        W = np.eye(3) if info is None else full_info(info[k])
        assert got["status"][k] == 0
        assert np.abs(got["r"][k] - r).max() <= 1e-11 and np.abs(got["J"][k] - J).max() <= 1e-11, (label, k)
        P_ref = J @ sig[k] @ J.T
        bound = BLOCK_REL * np.linalg.norm(J, 2) ** 2 * np.linalg.norm(sig[k])
        dP = np.linalg.norm(got["P"][k] - P_ref)
        assert dP <= bound, (label, k, dP, bound, np.linalg.norm(P_ref))
        assert np.array_equal(got["P"][k], got["P"][k].T)
        worst = max(worst, dP / np.linalg.norm(P_ref))
        chi2, cm, ig = algebra(r, P_ref, W)
        w2 = np.linalg.norm(W, 2)
        rg = got["r"][k]    # chi2 is the form of the record's own r (r itself is held to 1e-11 above, not to an ulp)
        assert abs(got["chi2"][k] - max(rg @ W @ rg, 0.0)) <= 16 * EPS * np.linalg.norm(W) * (rg @ rg), (label, k)
        assert abs(got["chi2_marginal"][k] - cm) <= chi2 * w2 * bound, (label, k, got["chi2_marginal"][k], cm)
        assert abs(got["info_gain"][k] - ig) <= np.sqrt(3.0) / 2 * w2 * bound, (label, k, got["info_gain"][k], ig)
    print(f"{label}: max |dP|/|P| = {worst:.3e} over {len(ia)} candidates")
    return worst


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


def agree(a, b, sel_a=slice(None), sel_b=slice(None)):
    """two results of the library within VARIANT, field by field, relative to the field's largest entry"""
    for f in FIELDS:
        x, y = a[f][sel_a], b[f][sel_b]
        assert np.abs(x - y).max() <= VARIANT * np.abs(y).max(), (f, np.abs(x - y).max() / np.abs(y).max())
    assert np.array_equal(a["status"][sel_a], b["status"][sel_b])


# ------------------------------------------------------------------------------------------------------- 1. parity
def test_parity_intel_bogus_loops(pgo, oracle):
    """the 50 loops add_random_C(50, 1) appends to a second copy of INTEL, against a handle on INTEL without them: 4 passes of
    16, 16, 16 and 2 candidates, with the identity and with the candidates' own information"""
    g = load(pgo, "INTEL")
    g2 = load(pgo, "INTEL", 50)
    E = g.n_edges
    ia, ib, meas, info = (np.array(x[E:]) for x in (g2.ia, g2.ib, g2.meas, g2.info))
    assert len(ia) == 50
    og = oracle_graph(oracle, g)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.solve()
    poses = s.poses()
    uniq = np.unique(np.concatenate([ia, ib]))
    sig = sigma_pairs(reference_blocks(oracle, og, poses, uniq, 1, cross=True), uniq, ia, ib)
    for label, w in (("INTEL m1, identity", None), ("INTEL m1, own information", info)):
        got, rep = s.gate(ia, ib, meas, w, poses_per_pass=16)
        assert rep["passes"] == 4 and rep["columns"] == 150 and rep["max_rel_residual"] <= 1e-5, rep
        check_against_reference(oracle, got, poses, ia, ib, meas, w, sig, label)
        assert all(np.linalg.eigvalsh(p).min() > 0 for p in got["P"])
        assert (got["chi2_marginal"] <= got["chi2"]).all() and (got["info_gain"] > 0).all()
    s.close()


def test_parity_m3500(pgo, oracle):
    g = load(pgo, "M3500")
    og = oracle_graph(oracle, g)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=3))
    s.solve()
    poses = s.poses()
    ia, ib, meas = candidates(np.random.default_rng(11), poses, 17)
    uniq = np.unique(np.concatenate([ia, ib]))
    sig = sigma_pairs(reference_blocks(oracle, og, poses, uniq, 1, cross=True), uniq, ia, ib)
    got, rep = s.gate(ia, ib, meas)
    assert rep["passes"] == 3 and rep["columns"] == 51, rep
    check_against_reference(oracle, got, poses, ia, ib, meas, None, sig, "M3500 m1")
    s.close()


def test_parity_method2(pgo, oracle):
    g = load(pgo, "INTEL", 50)
    og = oracle_graph(oracle, g)
    s = pgo.Solver(g, pgo.Options(method=2, max_iters=5))
    s.solve()
    poses = s.poses()
    ia, ib, meas = candidates(np.random.default_rng(12), poses, 8)
    info = np.tile([2.0, 0, 0, 300.0, 0, 300.0], (8, 1))
    uniq = np.unique(np.concatenate([ia, ib]))
    sig = sigma_pairs(reference_blocks(oracle, og, poses, uniq, 2, s.switches(), cross=True), uniq, ia, ib)
    got, rep = s.gate(ia, ib, meas, info)
    assert rep["passes"] == 1 and rep["columns"] == 24, rep
    check_against_reference(oracle, got, poses, ia, ib, meas, info, sig, "INTEL+50 m2")
    s.close()


def test_pose_ordering_gives_the_same_records(pgo):
    g = load(pgo, "INTEL")
    a = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    a.solve()
    b = pgo.Solver(g, pgo.Options(method=1, max_iters=5, pose_ordering=1))
    assert b.info().pose_ordering == 1
    b.set_poses(a.poses())
    ia, ib, meas = candidates(np.random.default_rng(13), a.poses(), 9)
    ra, _ = a.gate(ia, ib, meas)
    rb, rep = b.gate(ia, ib, meas)
    assert rep["passes"] == 2 and rep["columns"] == 27
    agree(rb, ra)
    a.close(); b.close()


# ---------------------------------------------------------------------------------- 2. pass and sweep edges, small graphs
def subgraph(pgo, g, n):
    """the first n poses of g and the edges among them"""
    ia, ib = np.array(g.ia), np.array(g.ib)
    m = (ia < n) & (ib < n)
    return pgo.Graph.from_arrays(np.array(g.poses)[:n], ia[m], ib[m], np.array(g.meas)[m], np.array(g.kind)[m], np.array(g.info)[m])


@pytest.mark.parametrize("n_poses", [300, 600], ids=["300-one-level", "600-coarse"])
def test_every_pass_shape_equals_single_candidate_calls(pgo, n_poses):
    """1, 2, 4, 8 candidates: k_spmm<3 / 6 / 12 / 24>; 9: 24 + 3 columns in two sweeps; 16: two full sweeps; 17: a second pass"""
    g = subgraph(pgo, load(pgo, "INTEL"), n_poses)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.solve()
    ia, ib, meas = candidates(np.random.default_rng(n_poses), s.poses(), 17)
    single = [s.gate(ia[k:k + 1], ib[k:k + 1], meas[k:k + 1])[0] for k in range(17)]
    single = {f: np.concatenate([x[f] for x in single]) for f in FIELDS + ("status",)}
    for n in (1, 2, 4, 8, 9, 16, 17):
        got, rep = s.gate(ia[:n], ib[:n], meas[:n], poses_per_pass=16)
        assert rep["passes"] == (n + 15) // 16 and rep["columns"] == 3 * n, (n, rep)
        agree(got, single, sel_b=slice(0, n))
    s.close()


# ----------------------------------------------------------------------------------------------------- 3. constants
def test_constant_endpoints(pgo):
    g = load(pgo, "INTEL")
    N = g.n_poses
    ia_g, ib_g = np.array(g.ia), np.array(g.ib)
    ea = ~((ia_g == N - 1) | (ib_g == N - 1))        # the last pose keeps no active edge: a resolved constant
    pc = np.zeros(N, bool)
    pc[[300, 301]] = True
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.set_active(ea, pc)
    s.solve()
    poses = s.poses()
    rng = np.random.default_rng(14)
    ia = np.array([0, 300, N - 1, N - 1, 40, 700, 1100], np.int32)
    ib = np.array([300, 500, 301, 600, 900, 20, 350], np.int32)
    _, _, meas = candidates(rng, poses, 7)
    meas[:, :2] += 0.3
    info = np.tile([2.0, 0, 0, 300.0, 0, 300.0], (7, 1))
    info[4] = [5.0, 0.5, 0.1, 40.0, -2.0, 90.0]
    sbb = {k: s.covariance([ib[k]])[0][0] for k in (1, 3)}                       # Sigma_bb of the free endpoint
    s6 = {k: s.covariance([ia[k], ib[k]], cross=True)[0] for k in (4, 5, 6)}     # the six-column route
    for w in (None, info):
        got, rep = s.gate(ia, ib, meas, w, poses_per_pass=16)
        assert rep["passes"] == 1 and rep["columns"] == 3 * 5, rep     # the two candidates between constants take none
        assert (got["status"] == 0).all()
        for k in (0, 2):   # (fixed pose, constant pose), (pose without an active edge, constant pose)
            W = np.eye(3) if w is None else full_info(w[k])
            r = got["r"][k]
            assert np.array_equal(got["P"][k], np.zeros((3, 3))) and got["info_gain"][k] == 0.0
            assert abs(got["chi2_marginal"][k] - got["chi2"][k]) <= 16 * EPS * np.linalg.norm(W) * (r @ r)
        for k in (1, 3):   # (constant, free b): P = J_b Sigma_bb J_b'
            Jb = got["J"][k][:, 3:]
            bound = BLOCK_REL * np.linalg.norm(got["J"][k], 2) ** 2 * np.linalg.norm(sbb[k])
            assert np.linalg.norm(got["P"][k] - Jb @ sbb[k] @ Jb.T) <= bound, k
        for k in (4, 5, 6):   # ordinary candidates of the same pass
            J, M = got["J"][k], s6[k]
            bound = BLOCK_REL * np.linalg.norm(J, 2) ** 2 * np.linalg.norm(M)
            assert np.linalg.norm(got["P"][k] - J @ M @ J.T) <= bound, k
            W = np.eye(3) if w is None else full_info(w[k])
            chi2, cm, ig = algebra(got["r"][k], J @ M @ J.T, W)
            w2 = np.linalg.norm(W, 2)
            assert abs(got["chi2_marginal"][k] - cm) <= chi2 * w2 * bound
            assert abs(got["info_gain"][k] - ig) <= np.sqrt(3.0) / 2 * w2 * bound
    # only candidates between constants: no pass at all
    got, rep = s.gate(ia[[0, 2]], ib[[0, 2]], meas[[0, 2]])
    assert rep["passes"] == 0 and rep["columns"] == 0 and np.array_equal(got["P"], np.zeros((2, 3, 3)))
    s.close()


# ------------------------------------------------------------------------------------- 4. a non-evaluable candidate
def test_non_evaluable_candidate_in_the_middle_of_a_pass(pgo):
    g = subgraph(pgo, load(pgo, "INTEL"), 300)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.solve()
    poses = s.poses()
    poses[[50, 120], 2] = 0.0
    s.set_poses(poses)
    ia, ib, meas = candidates(np.random.default_rng(15), poses, 5, lo=1)
    ia[2], ib[2], meas[2] = 50, 120, [0.1, 0.2, np.pi / 2]      # sin delta = -1 exactly: g = cos delta / 0
    keep = np.array([0, 1, 3, 4])
    got, rep = s.gate(ia, ib, meas)
    ref, rep_ref = s.gate(ia[keep], ib[keep], meas[keep])
    assert rep["columns"] == 12 == rep_ref["columns"] and rep["passes"] == 1
    assert got["status"].tolist() == [0, 0, 1, 0, 0]
    for f in FIELDS:
        assert np.isnan(got[f][2]).all(), f
        assert np.isfinite(got[f][keep]).all(), f
    agree(got, ref, sel_a=keep)
    s.close()


# ------------------------------------------------------------------------------------------------- 5. LM state untouched
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
    idx = [1, 400, 942]
    before, _ = s.covariance(idx)
    ia, ib, meas = candidates(np.random.default_rng(16), s.poses(), 9)
    s.gate(ia, ib, meas)
    after, _ = s.covariance(idx)
    assert np.array_equal(before, after)
    s.lm_step(100)
    assert np.array_equal(s.poses(), ref.poses())
    assert _records(s) == _records(ref)
    s.close()
    ref.close()


# ------------------------------------------------------------------------------------------------------------ 6. repeat
def test_repeat_is_bitwise(pgo):
    g = load(pgo, "INTEL", 50)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=3))
    s.solve()
    ia, ib, meas = candidates(np.random.default_rng(17), s.poses(), 20)
    info = np.tile([2.0, 0, 0, 300.0, 0, 300.0], (20, 1))
    a, ra = s.gate(ia, ib, meas, info)
    b, rb = s.gate(ia, ib, meas, info)
    for f in FIELDS + ("status",):
        assert np.array_equal(a[f], b[f]), f
    assert ra["pcg_iters_total"] == rb["pcg_iters_total"] and ra["passes"] == 3 and ra["columns"] == 60
    s.close()


# ------------------------------------------------------------------------------------------------------------ 7. errors
def test_errors(pgo):
    import ctypes as C
    g = load(pgo, "INTEL", 50)
    N = g.n_poses
    m = np.array([[0.1, 0.2, 0.3]])
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=1))

    def status(*a, **k):
        with pytest.raises(pgo.PgoError) as e:
            s.gate(*a, **k)
        return e.value.status

    assert status([5], [5], m) == -1                                         # a == b
    assert status([5], [N], m) == -1 and status([-1], [5], m) == -1          # out of range
    assert status([5], [9], m, [[1.0, 2.0, 0, 1.0, 0, 1.0]]) == -1           # not positive definite
    assert status([5], [9], m, [[np.nan, 0, 0, 1.0, 0, 1.0]]) == -1
    assert status([5], [9], m, poses_per_pass=17) == -1
    one = np.array([5], np.int32)
    res, rep = (pgo.EdgeGateResult * 1)(), pgo.CovarianceReport()
    assert pgo.lib().pgo_edge_gate(s._h, 1, None, one.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, res, C.byref(rep)) == -1
    assert pgo.lib().pgo_edge_gate(None, 0, None, None, None, None, None, None, None) == -1
    got, rep = s.gate([], [], np.zeros((0, 3)))                              # n = 0
    assert got["P"].shape == (0, 3, 3) and got["status"].size == 0 and rep["columns"] == 0 and rep["passes"] == 0
    assert pgo.lib().pgo_edge_gate(s._h, 0, None, None, None, None, None, None, None) == 0
    got, rep = s.gate([5], [9], m)                                           # (the handle is still usable)
    assert got["status"][0] == 0 and rep["columns"] == 3
    s.close()
    for opts in (dict(info_weighting=1), dict(fixed_pose=-1)):
        s = pgo.Solver(g, pgo.Options(method=1, max_iters=1, **opts))
        assert status([5], [9], m) == -8, opts
        s.close()
    s = pgo.Solver(g, pgo.Options(method=2, max_iters=1))                    # METHOD 2 before lm_begin: no switches yet
    assert status([5], [9], m) == -1
    s.lm_begin()
    got, _ = s.gate([5], [9], m)
    assert got["status"][0] == 0
    s.close()
