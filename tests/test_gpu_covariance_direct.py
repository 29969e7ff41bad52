"""pgo_pose_covariance and pgo_edge_gate with solver = 1: the columns through the handle's direct solve (chain + low rank at
D'D = 0, csrc/solver_covariance.hip Session::pass_direct) instead of PCG.

Chains are built as tests/test_gpu_direct.py builds them (chain_graph: noisy odometry, noisy poses), with linear_solver = 2.
References: the dense inverse of the oracle's J'J with the constant poses removed (chains), the sparse direct inverse of
tests/test_gpu_covariance.py (datasets).  Bounds are the suite's own and none is fitted to this path: BLOCK_REL per block,
RES_MAX on report.max_rel_residual, and for the gate the bounds of tests/test_gpu_gate.py (BLOCK_REL pushed through J . J'
and M >= I: check_against_reference).  Where one system is solved twice by this path (pass widths, repeats, a restored
handle) the outputs must be equal bit for bit.  The CPU restatement of the same algebra: tests/test_covariance_direct_math.py."""
import numpy as np
import pytest

from conftest import oracle_graph
from test_gpu_covariance import BLOCK_REL, RES_MAX, _records, block_errors, load, pick, reference_blocks
from test_gpu_direct import chain_graph, rand_loops
from test_gpu_gate import FIELDS, candidates, check_against_reference, sigma_pairs

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID, NUMERIC = -8, -1, -7


def dense_sigma(O, og, poses, method, const=(0,)):
    """(J'J)^-1 over the free poses by a dense inverse; zero rows and columns on the constant poses"""
    N, E = og.n_poses, og.n_edges
    _, _, J = O.evaluate(og, poses, method=method)
    J = np.asarray(J).reshape(E, 3, 6)
    ia, ib = np.asarray(og.ia), np.asarray(og.ib)
    Jd = np.zeros((3 * E, 3 * N))
    for e in range(E):
        Jd[3 * e:3 * e + 3, 3 * ia[e]:3 * ia[e] + 3] = J[e][:, :3]
        Jd[3 * e:3 * e + 3, 3 * ib[e]:3 * ib[e] + 3] = J[e][:, 3:]
    keep = np.ones(3 * N, bool)
    for c in const:
        keep[3 * c:3 * c + 3] = False
    S = np.zeros((3 * N, 3 * N))
    S[np.ix_(keep, keep)] = np.linalg.inv(Jd[:, keep].T @ Jd[:, keep])
    return 0.5 * (S + S.T)


def check_cross(M, ref, idx, const=(0,)):
    """every block (a, b) of the cross matrix M over the poses idx within BLOCK_REL |Sigma_aa|; returns the largest quotient"""
    assert np.array_equal(M, M.T)
    worst = 0.0
    for a, pa in enumerate(idx):
        Ra = ref[3 * pa:3 * pa + 3]
        if pa in const:
            assert not M[3 * a:3 * a + 3].any()
            continue
        naa = np.linalg.norm(Ra[:, 3 * pa:3 * pa + 3])
        for b, pb in enumerate(idx):
            d = np.linalg.norm(M[3 * a:3 * a + 3, 3 * b:3 * b + 3] - Ra[:, 3 * pb:3 * pb + 3]) / naa
            assert d <= BLOCK_REL, (pa, pb, d)
            worst = max(worst, d)
    return worst


def check_report(rep, columns):
    assert rep["columns"] == columns and rep["passes"] >= 1, rep
    assert rep["pcg_iters_total"] == 0 and rep["pcg_iters_max"] == 0, rep
    assert rep["max_rel_residual"] <= RES_MAX, rep


def chain_solver(pgo, ag, method, fixed=0, iters=2):
    s = pgo.Solver(ag.to_pgo(pgo), pgo.Options(method=method, max_iters=iters, fixed_pose=fixed, linear_solver=2))
    s.solve()
    assert s.info().linear_solver == 2
    return s


# ------------------------------------------------------------------------------------------------- 1. smallest sizes
@pytest.mark.parametrize("loops,fixed", [([], 0), ([(3, 20), (30, 8)], 0), ([(3, 20), (30, 8)], 16)],
                         ids=["N33-K0", "N33-K6", "N33-K6-fixed-middle"])
def test_smallest_sizes(pgo, oracle, loops, fixed):
    """33 poses: 17 sweep segments of 2 poses; no loop at all (K = 0: no capacitance matrix) and two loops (one Cholesky
    block); every pose, with the cross blocks"""
    ag = chain_graph(33, loops, 5, fixed)
    s = chain_solver(pgo, ag, 0, fixed)
    assert s.info().direct_rank == 3 * len(loops)
    idx = np.arange(33)
    M, rep = s.covariance(idx, cross=True, solver=1)
    check_report(rep, 99)
    worst = check_cross(M, dense_sigma(oracle, ag.to_oracle(oracle), s.poses(), 0, (fixed,)), idx, (fixed,))
    print(f"N33, {len(loops)} loops, constant pose {fixed}: largest block error {worst:.2e}, max_rel_residual {rep['max_rel_residual']:.2e}")
    s.close()


# -------------------------------------------------------------------------- 2. separators and several Cholesky blocks
N2 = 300
LOOPS2 = [(75, 110), (74, 120), (151, 190), (0, 33)] + rand_loops(N2, 28, seed=9)   # separators of 300 poses: 75, 150, 225


@pytest.fixture(scope="module")
def case2(pgo):
    ag = chain_graph(N2, LOOPS2, 6)
    s = chain_solver(pgo, ag, 1)
    info = s.info()
    assert info.direct_rank == 96 and info.direct_separators == 3
    yield ag, s
    s.close()


def test_separators_and_three_cholesky_blocks(pgo, oracle, case2):
    ag, s = case2
    idx = pick(N2)
    ref = dense_sigma(oracle, ag.to_oracle(oracle), s.poses(), 1)
    got, rep = s.covariance(idx, solver=1)
    check_report(rep, 3 * idx.size)
    ref_b = np.stack([ref[3 * p:3 * p + 3, 3 * p:3 * p + 3] for p in idx])
    err = block_errors(got[1:], ref_b[1:])
    assert err.max() <= BLOCK_REL, err.max()
    assert not got[0].any()
    M, rep2 = s.covariance(idx, cross=True, solver=1)
    check_report(rep2, 3 * idx.size)
    worst = check_cross(M, ref, idx)
    for a in range(idx.size):   # the diagonal call solves the same columns
        assert np.array_equal(M[3 * a:3 * a + 3, 3 * a:3 * a + 3], got[a])
    pcg, _ = s.covariance(idx, solver=0)
    print(f"N300 K96: diagonal blocks {err.max():.2e}, cross blocks {worst:.2e}, max_rel_residual {rep['max_rel_residual']:.2e}, "
          f"against solver=0 {np.abs(got - pcg).max() / np.abs(pcg).max():.2e}")


# ------------------------------------------------------------------------------------------------------- 3. datasets
def test_intel_method1_blocks_and_gate(pgo, oracle):
    g = load(pgo, "INTEL", 50)
    og = oracle_graph(oracle, g)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.solve()
    assert s.info().linear_solver == 2
    poses = s.poses()
    idx = pick(g.n_poses)
    got, rep = s.covariance(idx, solver=1)
    check_report(rep, 3 * idx.size)
    assert rep["passes"] == 1
    err = block_errors(got[1:], reference_blocks(oracle, og, poses, idx, 1)[1:])
    pcg, rep0 = s.covariance(idx, solver=0)
    print(f"INTEL+50 m1: blocks {err.max():.2e}, max_rel_residual {rep['max_rel_residual']:.2e} (solver=0: {rep0['max_rel_residual']:.2e}), "
          f"against solver=0 {np.abs(got - pcg).max() / np.abs(pcg).max():.2e}")
    assert err.max() <= BLOCK_REL and not got[0].any()
    assert all(np.linalg.eigvalsh(b).min() > 0 for b in got[1:])
    E = g.n_edges - 50
    ia, ib, meas, info = (np.array(x[E:]) for x in (g.ia, g.ib, g.meas, g.info))
    uniq = np.unique(np.concatenate([ia, ib]))
    sig = sigma_pairs(reference_blocks(oracle, og, poses, uniq, 1, cross=True), uniq, ia, ib)
    for label, w in (("INTEL+50 m1 solver=1, identity", None), ("INTEL+50 m1 solver=1, own information", info)):
        res, rep = s.gate(ia, ib, meas, w, solver=1)
        check_report(rep, 150)
        assert rep["passes"] == 1
        check_against_reference(oracle, res, poses, ia, ib, meas, w, sig, label)
        res0, _ = s.gate(ia, ib, meas, w, solver=0, poses_per_pass=16)
        print("  against solver=0:", {f: float(np.abs(res[f] - res0[f]).max() / np.abs(res0[f]).max()) for f in ("P", "chi2_marginal", "info_gain")})
    s.close()


def test_intel_all_loops_in_full_width_passes(pgo, oracle):
    """every loop edge of INTEL + 50 (306 candidates, 918 columns) at the default width: a pass of 256 candidates and one of 50,
    more than 64 candidates in a pass and more than one pass.  Every record against the reference, and bitwise against the same
    candidates gated 16 per pass"""
    g = load(pgo, "INTEL", 50)
    og = oracle_graph(oracle, g)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.solve()
    assert s.info().linear_solver == 2
    poses = s.poses()
    ia_g, ib_g = np.array(g.ia), np.array(g.ib)
    loop = np.nonzero(np.abs(ia_g - ib_g) != 1)[0]
    assert loop.size == 306
    ia, ib, meas, info = ia_g[loop], ib_g[loop], np.array(g.meas)[loop], np.array(g.info)[loop]
    got, rep = s.gate(ia, ib, meas, info, solver=1)
    check_report(rep, 918)
    assert rep["passes"] == 2, rep
    assert (got["status"] == 0).all() and all(np.isfinite(got[f]).all() for f in FIELDS)
    narrow, rep48 = with_width(pgo, 48, lambda: s.gate(ia, ib, meas, info, solver=1))
    assert rep48["passes"] == 20 and rep48["columns"] == 918, rep48
    for f in FIELDS + ("status",):
        assert np.array_equal(got[f], narrow[f]), f
    uniq = np.unique(np.concatenate([ia, ib]))
    sig = sigma_pairs(reference_blocks(oracle, og, poses, uniq, 1, cross=True), uniq, ia, ib)
    check_against_reference(oracle, got, poses, ia, ib, meas, info, sig, "INTEL+50 m1 solver=1, all 306 loops")
    s.close()


def test_intel_method2_gate(pgo, oracle):
    g = load(pgo, "INTEL", 50)
    og = oracle_graph(oracle, g)
    s = pgo.Solver(g, pgo.Options(method=2, max_iters=5))
    s.solve()
    assert s.info().linear_solver == 2
    poses = s.poses()
    ia, ib, meas = candidates(np.random.default_rng(12), poses, 8)
    info = np.tile([2.0, 0, 0, 300.0, 0, 300.0], (8, 1))
    uniq = np.unique(np.concatenate([ia, ib]))
    sig = sigma_pairs(reference_blocks(oracle, og, poses, uniq, 2, s.switches(), cross=True), uniq, ia, ib)
    got, rep = s.gate(ia, ib, meas, info, solver=1)
    check_report(rep, 24)
    check_against_reference(oracle, got, poses, ia, ib, meas, info, sig, "INTEL+50 m2 solver=1")
    got0, _ = s.gate(ia, ib, meas, info, solver=0)
    print("  against solver=0:", float(np.abs(got["P"] - got0["P"]).max() / np.abs(got0["P"]).max()), rep)
    s.close()


def test_mit_method1_closures(pgo, oracle):
    g = load(pgo, "MIT")
    og = oracle_graph(oracle, g)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.solve()
    assert s.info().linear_solver == 2
    poses = s.poses()
    ia_g, ib_g = np.array(g.ia), np.array(g.ib)
    loop = np.nonzero(np.abs(ia_g - ib_g) != 1)[0]
    assert loop.size == 20
    ia, ib, meas = ia_g[loop], ib_g[loop], np.array(g.meas)[loop]
    uniq = np.unique(np.concatenate([ia, ib]))
    sig = sigma_pairs(reference_blocks(oracle, og, poses, uniq, 1, cross=True), uniq, ia, ib)
    got, rep = s.gate(ia, ib, meas, solver=1)
    print("MIT m1 solver=1:", rep)
    check_report(rep, 60)
    check_against_reference(oracle, got, poses, ia, ib, meas, None, sig, "MIT m1 solver=1")
    got0, rep0 = s.gate(ia, ib, meas, solver=0, poses_per_pass=16)
    print("  against solver=0:", float(np.abs(got["P"] - got0["P"]).max() / np.abs(got0["P"]).max()), "solver=0 residual", rep0["max_rel_residual"])
    s.close()


# ---------------------------------------------------------------------------------------------------- 4. pass width
def with_width(pgo, k, call):
    pgo.set_knob("cov_direct_cols", k)
    try:
        return call()
    finally:
        pgo.set_knob("cov_direct_cols", -1)


def test_every_pass_width_gives_the_same_bits(pgo, case2):
    """21 columns in passes of 3 (seven), 6 (three and a partial one), 48 and the default (one): a column's result depends on
    neither the width nor its place in the pass"""
    ag, s = case2
    idx = np.array([1, 40, 75, 76, 150, 224, 299])
    base, rep = s.covariance(idx, cross=True, solver=1)
    assert rep["passes"] == 1
    for k, passes in ((3, 7), (6, 4), (48, 1)):
        M, rep = with_width(pgo, k, lambda: s.covariance(idx, cross=True, solver=1))
        assert rep["passes"] == passes and rep["columns"] == 21, (k, rep)
        assert np.array_equal(M, base), k
    ia, ib, meas = candidates(np.random.default_rng(21), s.poses(), 5, lo=1)
    gbase, rep = s.gate(ia, ib, meas, solver=1)
    assert rep["passes"] == 1 and rep["columns"] == 15
    for k, passes in ((3, 5), (6, 3), (48, 1)):
        got, rep = with_width(pgo, k, lambda: s.gate(ia, ib, meas, solver=1))
        assert rep["passes"] == passes and rep["columns"] == 15, (k, rep)
        for f in FIELDS + ("status",):
            assert np.array_equal(got[f], gbase[f]), (k, f)


# ------------------------------------------------------------------------------------- 5. bitwise repeat and LM state
def test_repeat_is_bitwise(pgo, case2):
    ag, s = case2
    idx = pick(N2, k=9)
    a, ra = s.covariance(idx, solver=1)
    b, rb = s.covariance(idx, solver=1)
    assert np.array_equal(a, b) and ra["max_rel_residual"] == rb["max_rel_residual"]
    ia, ib, meas = candidates(np.random.default_rng(22), s.poses(), 6, lo=1)
    ga, _ = s.gate(ia, ib, meas, solver=1)
    gb, _ = s.gate(ia, ib, meas, solver=1)
    for f in FIELDS + ("status",):
        assert np.array_equal(ga[f], gb[f]), f


@pytest.mark.parametrize("method", [1, 2])
def test_lm_state_is_untouched(pgo, method):
    g = load(pgo, "INTEL", 50)
    o = dict(method=method, max_iters=12)
    ref = pgo.Solver(g, pgo.Options(**o))
    ref.lm_begin()
    ref.lm_step(5)
    ref.lm_step(100)
    s = pgo.Solver(g, pgo.Options(**o))
    assert s.info().linear_solver == 2
    s.lm_begin()
    s.lm_step(5)
    idx = [1, 400, 942]
    before, _ = s.covariance(idx, solver=1)
    ia, ib, meas = candidates(np.random.default_rng(16), s.poses(), 9)
    s.gate(ia, ib, meas, solver=1)
    after, _ = s.covariance(idx, solver=1)
    assert np.array_equal(before, after)
    s.lm_step(100)
    assert np.array_equal(s.poses(), ref.poses())
    assert _records(s) == _records(ref)
    s.close()
    ref.close()


# ------------------------------------------------------------------------------------------------ 6. gate edge cases
def test_gate_edge_cases(pgo, oracle):
    ag = chain_graph(N2, LOOPS2, 6)
    s = chain_solver(pgo, ag, 1)
    poses = s.poses()
    poses[[50, 120], 2] = 0.0
    s.set_poses(poses)
    pc = np.zeros(N2, bool)
    pc[[200, 260]] = True
    s.set_active(None, pc)                      # the chain is whole: the handle stays on the direct solve
    assert s.info().linear_solver == 2
    # 0, 5: ordinary; 1: sin delta = -1 exactly (status 1); 2: both endpoints constant; 3: the constant pose of the options
    # and one of the mask; 4: one constant endpoint
    ia = np.array([10, 50, 200, 0, 260, 130], np.int32)
    ib = np.array([40, 120, 260, 200, 90, 280], np.int32)
    meas = np.array([[0.3, -0.2, 0.1], [0.1, 0.2, np.pi / 2], [1.0, 2.0, 0.2], [0.5, 0.5, -0.3], [2.0, -1.0, 0.4], [-1.0, 0.7, 1.0]])
    dth = poses[ib, 2] - poses[ia, 2] - meas[:, 2]
    assert (np.abs(np.sin(dth[[0, 2, 3, 4, 5]])) < 0.999).all()
    got, rep = s.gate(ia, ib, meas, solver=1)
    check_report(rep, 9)                        # candidates 0, 4, 5
    assert got["status"].tolist() == [0, 1, 0, 0, 0, 0]
    for f in FIELDS:
        assert np.isnan(got[f][1]).all(), f
        assert np.isfinite(got[f][[0, 2, 3, 4, 5]]).all(), f
    for k in (2, 3):
        assert np.array_equal(got["P"][k], np.zeros((3, 3))) and got["info_gain"][k] == 0.0
    ref = dense_sigma(oracle, ag.to_oracle(oracle), poses, 1, (0, 200, 260))
    for k in (0, 4, 5):
        rows = np.concatenate([3 * ia[k] + np.arange(3), 3 * ib[k] + np.arange(3)])
        sig, J = ref[np.ix_(rows, rows)], got["J"][k]
        assert np.linalg.norm(got["P"][k] - J @ sig @ J.T) <= BLOCK_REL * np.linalg.norm(J, 2) ** 2 * np.linalg.norm(sig), k
    Jb = got["J"][4][:, 3:]                     # (constant, free b): P = J_b Sigma_bb J_b'
    sbb = ref[3 * 90:3 * 90 + 3, 3 * 90:3 * 90 + 3]
    assert np.linalg.norm(got["P"][4] - Jb @ sbb @ Jb.T) <= BLOCK_REL * np.linalg.norm(got["J"][4], 2) ** 2 * np.linalg.norm(sbb)
    only, rep = s.gate(ia[[2, 3]], ib[[2, 3]], meas[[2, 3]], solver=1)   # no pass at all
    assert rep["passes"] == 0 and rep["columns"] == 0 and np.array_equal(only["P"], np.zeros((2, 3, 3)))
    none, rep = s.gate([], [], np.zeros((0, 3)), solver=1)
    assert none["status"].size == 0 and rep["columns"] == 0 and rep["passes"] == 0
    c, rep = s.covariance([], solver=1)
    assert c.shape == (0, 3, 3) and rep["columns"] == 0
    s.close()


# ------------------------------------------------------------------------------------- 7. refusals and the report
def status_of(pgo, call):
    with pytest.raises(pgo.PgoError) as e:
        call()
    return e.value.status


def test_refusals_and_report(pgo):
    ag = chain_graph(N2, LOOPS2, 6)
    g = ag.to_pgo(pgo)
    m = np.array([[0.1, 0.2, 0.3]])
    p = pgo.Solver(g, pgo.Options(method=1, max_iters=2, linear_solver=1))
    p.solve()
    assert p.info().linear_solver == 1
    assert status_of(pgo, lambda: p.covariance([5], solver=1)) == UNSUPPORTED     # never a fallback to PCG
    assert status_of(pgo, lambda: p.gate([5], [9], m, solver=1)) == UNSUPPORTED
    p.covariance([5], solver=0)
    p.close()
    s = chain_solver(pgo, ag, 1)
    # pgo_set_active leaves the solve stale: the next call linearises afresh, with Jacobi scales taken at the current poses
    # where the solve's were taken at its first iteration.  "Before" is therefore taken in that state too -- after a
    # pgo_set_active that changes nothing -- so that before and after the cut mask solve the same scaled system.
    s.set_active(None, None)
    idx = [1, 150, 299]
    base, rep = s.covariance(idx, solver=1)
    check_report(rep, 9)
    gbase, grep_ = s.gate([5], [9], m, solver=1)
    check_report(grep_, 3)
    for bad in (2, -1):
        assert status_of(pgo, lambda: s.covariance(idx, solver=bad)) == INVALID
        assert status_of(pgo, lambda: s.gate([5], [9], m, solver=bad)) == INVALID
    assert status_of(pgo, lambda: with_width(pgo, 4, lambda: s.covariance(idx, solver=1))) == INVALID   # not a multiple of 3
    assert status_of(pgo, lambda: with_width(pgo, 771, lambda: s.gate([5], [9], m, solver=1))) == INVALID
    with_width(pgo, 4, lambda: s.covariance(idx, solver=0))                        # (the knob is this path's alone)
    ea = np.ones(ag.n_edges, bool)
    ea[100] = False                                                                # the chain edge 100 -> 101; the loops keep J'J regular
    s.set_active(ea, None)
    assert s.info().linear_solver == 1
    assert status_of(pgo, lambda: s.covariance(idx, solver=1)) == UNSUPPORTED
    assert status_of(pgo, lambda: s.gate([5], [9], m, solver=1)) == UNSUPPORTED
    s.set_active(None, None)
    assert s.info().linear_solver == 2
    again, rep = s.covariance(idx, solver=1)
    assert np.array_equal(again, base)
    gagain, _ = s.gate([5], [9], m, solver=1)
    for f in FIELDS + ("status",):
        assert np.array_equal(gagain[f], gbase[f]), f
    s.close()


# --------------------------------------------------------------------------------- 8. singular chain, regular system
def test_singular_chain_is_named_and_pcg_still_applies(pgo):
    """33 poses, one loop 10 -> 25; the chain edge 16 -> 17 measures 1 m off and has a class of its own with Tukey(0.1): its
    rows are zero, the chain T falls apart although the loop keeps J'J regular"""
    ag = chain_graph(33, [(10, 25)], 7)
    ag.meas[16, 0] += 1.0
    cls = np.zeros(ag.n_edges, np.uint8)
    cls[16] = 1
    s = pgo.Solver(ag.to_pgo(pgo), pgo.Options(method=0, max_iters=2, linear_solver=2),
                   losses=[pgo.Loss("trivial"), pgo.Loss("tukey", 0.1)], edge_class=cls)
    assert s.info().linear_solver == 2
    idx = [5, 20, 30]
    with pytest.raises(pgo.PgoError) as e:
        s.covariance(idx, solver=1)
    assert e.value.status == NUMERIC and "pose " in str(e.value) and "solver = 0" in str(e.value), str(e.value)
    got, rep = s.covariance(idx, solver=0)
    assert rep["max_rel_residual"] <= RES_MAX and all(np.linalg.eigvalsh(b).min() > 0 for b in got)
    s.close()
