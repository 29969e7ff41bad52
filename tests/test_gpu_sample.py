"""pgo_posterior_sample on the GPU against the numpy restatement (tests/_sample_restatement.py): the right-hand side as an
operator (pgo_debug_sample_rhs), the draws against a sparse-LU solve on both solvers, the estimator inside the Wishart cap
on the cases the CPU test has cleared, the bitwise promises (repeats, pass widths, composed draws, with and without the
deltas), an LM state left untouched, and the refusals.  Every handle stands at its graph's INITIAL poses unless said."""

import numpy as np
import pytest

import _active_cases as AC
import _loss_restatement as LR
import _sample_restatement as SR
import _solo_cases as SC
from conftest import oracle_graph

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
DJ = SC.DJ           # 1e-11: |J_device - J_oracle| per entry, the bound of K1's parity test
EPS_TOL = 1e-14      # device triples against the restatement's
RES_MAX = 1e-5       # the largest true residual a column may be accepted with (pgo_pose_covariance's floor)
SEED = 20260410


def check_rhs(s, P, label):
    """eps to 1e-14; b within the propagated bound per entry: DJ sum |eps| over the row's blocks (K1's parity bound on every
    Jacobian entry) + 1e-14 sum |J| (the triples' own tolerance) + (3 deg + 4) ulp of sum |J| |eps| (the fixed-order sums).
    Returns the worst ratio."""
    import scipy.sparse as sp
    worst = 0.0
    for sample in (0, 5):
        eps, b = s.debug_sample_rhs(SEED, sample)
        ref_eps = P.eps(SEED, sample)
        assert np.abs(eps - ref_eps).max() <= EPS_TOL, label
        ref_b, mag = P.rhs(SEED, sample)
        pattern = sp.csr_matrix((np.ones(P.Jm.nnz), P.Jm.indices, P.Jm.indptr), shape=P.Jm.shape)
        deg = np.asarray((pattern.T @ np.ones(3 * P.E))).reshape(P.N, 3) / 3.0
        bound = (DJ * (pattern.T @ np.abs(ref_eps).reshape(-1)) + EPS_TOL * (P.absJm.T @ np.ones(3 * P.E))).reshape(P.N, 3) + (3 * deg + 4) * EPS * mag
        if P.prior_pose is not None:   # the 3x3 Cholesky of rho' Lambda: a few ulp of its entries
            bound[P.prior_pose] += 1e-14 * np.abs(P.prior_R).sum(axis=2) * 10.0
        free = P.free.reshape(P.N, 3)
        assert np.array_equal(b[~free], np.zeros((~free).sum())), label
        ratio = (np.abs(b - ref_b)[free] / bound[free]).max()
        print("%s sample %d: worst |b - b_ref| / bound = %.3f" % (label, sample, ratio))
        assert ratio <= 1.0, (label, sample, ratio)
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("name", ["two", "w255", "w256", "w257", "gaps300", "hub256", "awkward"])
def test_rhs_operator_on_the_shape_cases(pgo, oracle, name):
    """b = J' eps at the row-tile edge (255 / 256 / 257 rows), on a 2-pose graph, with constant poses in the middle of the
    rows, on a row of 256 incidences and with duplicate, reversed and missing chain edges.
    Measured worst |b - b_ref| / bound on the MI355X: 0.024 (w255), 0.018 (w256), 0.007 (awkward), 0.006 (w257), 0.004 (hub256),
    below 0.001 (two, gaps300): the device's Jacobian blocks are far closer to the oracle's than K1's 1e-11."""
    og = SC.oracle_graph(oracle, name)
    s = pgo.Solver(SC.pgo_graph(pgo, name), pgo.Options(method=0))
    constant = [0]
    if name == "gaps300":   # the edge-less poses constant, and one pose of the half that has no constant pose
        mask = np.zeros(300, np.uint8)
        mask[20:281] = 1
        s.set_active(None, mask)
        constant = [0] + list(range(20, 281))
    _, _, J = oracle.evaluate(og, og.poses, method=0)
    P = SR.Problem(og.n_poses, og.ia, og.ib, J, constant=constant)
    check_rhs(s, P, name)
    s.close()


def _intel_variant(pgo, O, variant):
    """(solver, restated Problem) of INTEL + 50 at its initial poses under one variant of the linearisation"""
    g = AC.intel(pgo)
    og = oracle_graph(O, g)
    a = AC.arrays(g)
    E, N = g.n_edges, g.n_poses
    method = 0 if variant == "m0" else 1
    opts = dict(method=method)
    if variant == "ordered":
        opts["pose_ordering"] = 1
    s = pgo.Solver(g, pgo.Options(**opts))
    _, _, J = O.evaluate(og, og.poses, method=method)
    kw = {}
    if variant == "ordered":
        assert s.info().pose_ordering == 1
    elif variant == "cauchy":
        s.set_losses([pgo.Loss("trivial"), pgo.Loss("cauchy", 0.5)])
        losses = [("trivial", 0.0), ("cauchy", 0.5)]
        _, _, J = LR.evaluate(O, og, losses, LR.classes(a["kind"], 2), og.poses, method)
    elif variant == "weights":
        w = np.random.default_rng(3).uniform(0.0, 1.0, E)
        w[::7] = 0.0
        s.set_edge_weights(w)
        J = np.sqrt(w)[:, None] * J
    elif variant == "active":
        m = AC.layer_mask(a["kind"], seed=2)
        s.set_active(m, None)
        J = m[:, None] * J
    elif variant == "priors":
        rng = np.random.default_rng(8)
        B = rng.normal(size=(3, 3))
        pose = np.array([5, 300, 900, 1200])
        info = np.stack([B @ B.T + 0.5 * np.eye(3), np.diag([4.0, 4.0, 0.0]), np.outer(B[0], B[0]), 100.0 * np.eye(3)])
        s.set_priors(pose, a["poses"][pose] + 0.01 * rng.normal(size=(4, 3)), info)
        kw = dict(prior_pose=pose, prior_Lw=info)
    return s, SR.Problem(N, a["ia"], a["ib"], J, **kw)


@pytest.mark.parametrize("variant", ["m0", "m1", "cauchy", "weights", "active", "priors", "ordered"])
def test_rhs_operator_on_intel(pgo, oracle, variant):
    """INTEL + 50 under METHOD 0 and 1 (DCS), with Cauchy on the loops, an edge weight plane (zeros included), an active mask,
    pose priors (positive definite, diag(a, a, 0), rank one) and on the locality ordering: eps is keyed by the caller's edge
    index, J is what the last linearisation left.  Measured worst |b - b_ref| / bound on the MI355X: below 0.0005 in every variant."""
    s, P = _intel_variant(pgo, oracle, variant)
    check_rhs(s, P, "INTEL+50 " + variant)
    s.close()


def delta_bound(P, seed, first, n, ref, rel_residual):
    """per sample, in the maximum norm: 10 x the effect of a DJ disagreement in every Jacobian entry (random signs) on the
    restatement's own solution, plus the accepted true residual times the restatement's condition estimate times |delta|"""
    rng = np.random.default_rng(99)
    Q = SR.Problem(P.N, P.ia, P.ib, P.J + DJ * rng.choice(np.array([-1.0, 1.0]), size=P.J.shape) * (P.J != 0.0),
                   constant=[i for i in range(P.N) if not P.free[3 * i]],
                   prior_pose=P.prior_pose, prior_Lw=None if P.prior_pose is None else np.einsum("nij,nkj->nik", P.prior_R, P.prior_R))
    effect = np.abs(Q.deltas(seed, first, n) - ref).reshape(n, -1).max(axis=1)
    return 10.0 * effect + rel_residual * P.cond_estimate() * np.abs(ref).reshape(n, -1).max(axis=1)


def check_deltas(s, P, label, n=6, **opts):
    d, _, rep = s.sample(n, seed=SEED, want_cov=False, **opts)
    assert rep["columns"] == n and rep["max_rel_residual"] <= RES_MAX, rep
    ref = P.deltas(SEED, 0, n)
    bound = delta_bound(P, SEED, 0, n, ref, rep["max_rel_residual"])
    err = np.abs(d - ref).reshape(n, -1).max(axis=1)
    print("%s %s: worst |delta - ref| / bound = %.3e (|delta| max %.3e, err %.3e, residual %.1e)" % (
        label, opts, (err / bound).max(), np.abs(ref).max(), err.max(), rep["max_rel_residual"]))
    assert (err <= bound).all(), (label, opts, err, bound)
    free = P.free.reshape(P.N, 3)
    assert np.array_equal(d[:, ~free], np.zeros((n, (~free).sum())))
    return rep


@pytest.mark.parametrize("name", ["intel50-m1", "w257"])
def test_deltas_match_the_sparse_lu_solve(pgo, oracle, name):
    """the draws themselves, solver = 0 and, where the handle is on the direct solve, solver = 1"""
    g, method = SR.case_graph(pgo, name)
    P = SR.case_problem(pgo, oracle, name)
    s = pgo.Solver(g, pgo.Options(method=method))
    rep = check_deltas(s, P, name, solver=0, samples_per_pass=4)
    assert rep["passes"] == 2 and rep["pcg_iters_max"] > 0
    if s.info().linear_solver == 2:
        rep = check_deltas(s, P, name, solver=1)
        assert rep["passes"] == 1 and rep["pcg_iters_total"] == 0
    else:
        with pytest.raises(pgo.PgoError) as e:
            s.sample(2, solver=1)
        assert e.value.status == -8
    s.close()


def test_deltas_with_priors_and_ordering(pgo, oracle):
    for variant in ("priors", "ordered"):
        s, P = _intel_variant(pgo, oracle, variant)
        check_deltas(s, P, "INTEL+50 " + variant, n=3, solver=0)
        s.close()


@pytest.mark.parametrize("name", sorted(SR.ESTIMATOR_CASES))
def test_estimator_is_inside_the_wishart_cap(pgo, oracle, name):
    """cov_out of the device within 3 sqrt(12 / S) of the exact blocks in the whitened norm, on the cases and seeds
    tests/test_sample_host.py has cleared for the restatement, and equal to the restatement's estimate within what the delta
    bound allows a product of two deltas (2 |delta| bound + bound^2)"""
    seed, S = SR.ESTIMATOR_CASES[name]
    g, method = SR.case_graph(pgo, name)
    P = SR.case_problem(pgo, oracle, name)
    s = pgo.Solver(g, pgo.Options(method=method))
    solver = 1 if s.info().linear_solver == 2 else 0
    _, cov, rep = s.sample(S, seed=seed, want_deltas=False, solver=solver, samples_per_pass=48)
    assert rep["columns"] == S and rep["max_rel_residual"] <= RES_MAX
    assert np.array_equal(cov[0], np.zeros((3, 3))) and np.array_equal(cov, np.transpose(cov, (0, 2, 1)))
    err = SR.whitened_errors(cov[1:], P.exact_blocks()[1:])
    print("%s: device estimate, worst whitened error %.4f = %.3f sqrt(12 / S)" % (name, err.max(), err.max() / np.sqrt(12.0 / S)))
    assert err.max() <= SR.wishart_cap(S)
    ref = P.deltas(seed, 0, S)
    k = 8   # the delta bound from the first samples (the perturbed restatement is a second factorisation and solve)
    b = (delta_bound(P, seed, 0, k, ref[:k], rep["max_rel_residual"]) / np.abs(ref[:k]).reshape(k, -1).max(axis=1)).max()
    D = np.abs(ref).max()
    tol = 2.0 * D * (b * D) + (b * D) ** 2
    diff = np.abs(cov - SR.second_moment(ref)).max()
    print("%s: |cov - restated estimate| max %.3e, allowed %.3e" % (name, diff, tol))
    assert diff <= tol
    s.close()


def test_bitwise_promises(pgo):
    """repeat calls; samples_per_pass 1 / 3 / 24 / 48 and the direct widths 3 / 48 / default; [0, k) + [k, n) against
    [0, n); cov_out with and without delta_out"""
    g, method = SR.case_graph(pgo, "w257")
    s = pgo.Solver(g, pgo.Options(method=method, linear_solver=1))
    n = 50
    d0, c0, r0 = s.sample(n, seed=3, samples_per_pass=24)
    d1, c1, r1 = s.sample(n, seed=3, samples_per_pass=24)
    assert np.array_equal(d0, d1) and np.array_equal(c0, c1) and r0["pcg_iters_total"] == r1["pcg_iters_total"]
    for spp in (1, 3, 48):
        d, c, rep = s.sample(n, seed=3, samples_per_pass=spp)
        assert np.array_equal(d, d0) and np.array_equal(c, c0), spp
        assert rep["passes"] == (n + spp - 1) // spp
    _, c, _ = s.sample(n, seed=3, samples_per_pass=24, want_deltas=False)
    assert np.array_equal(c, c0)
    da, _, _ = s.sample(17, seed=3, first=0)
    db, _, _ = s.sample(n - 17, seed=3, first=17)
    assert np.array_equal(np.concatenate([da, db]), d0)
    dz, _, _ = s.sample(4, seed=4)
    assert not np.array_equal(dz, d0[:4])   # another seed, other draws
    s.close()
    # the direct solve
    g, method = SR.case_graph(pgo, "intel50-m1")
    s = pgo.Solver(g, pgo.Options(method=method))
    assert s.info().linear_solver == 2
    n = 100
    d0, c0, r0 = s.sample(n, seed=3, solver=1)
    assert r0["passes"] == 1
    try:
        for cols in (3, 48):
            pgo.set_knob("cov_direct_cols", cols)
            d, c, rep = s.sample(n, seed=3, solver=1)
            assert np.array_equal(d, d0) and np.array_equal(c, c0), cols
            assert rep["passes"] == (n + cols - 1) // cols
    finally:
        pgo.set_knob("cov_direct_cols", -1)
    d, c, _ = s.sample(n, seed=3, solver=1)
    assert np.array_equal(d, d0) and np.array_equal(c, c0)
    _, c, _ = s.sample(n, seed=3, solver=1, want_deltas=False)
    assert np.array_equal(c, c0)
    da, _, _ = s.sample(40, seed=3, solver=1)
    db, _, _ = s.sample(60, seed=3, first=40, solver=1)
    assert np.array_equal(np.concatenate([da, db]), d0)
    s.close()


def _records(s):
    return [{k: v for k, v in r.items() if k != "seconds"} for r in s.iter_records()]


@pytest.mark.parametrize("solver,opts", [(0, dict(linear_solver=1)), (1, {})], ids=["pcg", "direct"])
def test_lm_state_is_untouched(pgo, solver, opts):
    g = AC.intel(pgo)
    o = dict(method=1, max_iters=10, **opts)
    ref = pgo.Solver(g, pgo.Options(**o))
    ref.lm_begin()
    ref.lm_step(3)
    ref.lm_step(100)
    s = pgo.Solver(g, pgo.Options(**o))
    s.lm_begin()
    s.lm_step(3)
    s.sample(6, seed=1, solver=solver)
    s.debug_sample_rhs(1, 0)
    s.lm_step(100)
    assert np.array_equal(s.poses(), ref.poses())
    assert _records(s) == _records(ref)
    s.close()
    ref.close()


def test_errors(pgo):
    g = AC.intel(pgo)

    def refused(status, make, call, text=None):
        s = make()
        with pytest.raises(pgo.PgoError) as e:
            call(s)
        assert e.value.status == status, (status, str(e.value))
        if text:
            assert text in str(e.value)
        s.close()

    two = lambda s: s.sample(2)
    refused(-8, lambda: pgo.Solver(g, pgo.Options(method=2)), two, "METHOD 2")
    refused(-8, lambda: pgo.Solver(g, pgo.Options(method=2)), lambda s: s.debug_sample_rhs(0, 0), "METHOD 2")
    refused(-8, lambda: pgo.Solver(g, pgo.Options(method=1, info_weighting=1)), two)
    refused(-8, lambda: pgo.Solver(g, pgo.Options(method=1, fixed_pose=-1)), two)
    refused(-8, lambda: pgo.Solver(g, pgo.Options(method=1, linear_solver=1)), lambda s: s.sample(2, solver=1))
    ok = lambda: pgo.Solver(g, pgo.Options(method=1))
    refused(-1, ok, lambda s: s.sample(0))
    refused(-1, ok, lambda s: s.sample(2, samples_per_pass=0))
    refused(-1, ok, lambda s: s.sample(2, samples_per_pass=49))
    refused(-1, ok, lambda s: s.sample(2, first=-1))
    refused(-1, ok, lambda s: s.sample(2, want_deltas=False, want_cov=False))
    refused(-1, ok, lambda s: s.sample(2, solver=2))
    refused(-1, ok, lambda s: s.debug_sample_rhs(0, -1))

    def nan_pose(s):
        bad = s.poses()
        bad[77, 2] = np.nan
        s.set_poses(bad)
        s.sample(2)
    refused(-7, ok, nan_pose, "pose 77")

    def all_constant(s):
        s.set_active(None, np.ones(g.n_poses, np.uint8))
        s.sample(2)
    refused(-1, ok, all_constant, "constant")
    # a batched handle has no such call: the session's refusal is pgo_pose_covariance's (tests/test_gpu_covariance.py)


def test_cli_sample_cov_flag(pgo, tmp_path):
    """--sample-cov S[:SEED] through the C++ mirror (pgo::SamplePosterior on a handle made at the solved poses): cov_nodes.txt
    holds one line per pose, and its blocks are those of Solver.sample from the same poses -- the same stream, the same
    linearisation, each solve to rtol 1e-10 (compared to 1e-8 of the largest entry)"""
    import os
    import subprocess
    from importlib import import_module
    from conftest import DATA
    exe = import_module("toy_robust_backend_slam_amd._build").build_cli()
    save = str(tmp_path / "save")
    p = subprocess.run([exe, "INTEL", "50", "1", "--seed", "1", "--data", DATA, "--save", save, "--precision", "17", "--sample-cov", "32:5"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sample-cov: 32 samples" in p.stdout
    g = AC.intel(pgo)
    rows = np.loadtxt(os.path.join(save, "cov_nodes.txt"))
    assert rows.shape == (g.n_poses, 7) and np.array_equal(rows[:, 0], np.array(g.pose_ids))
    s = pgo.Solver(g, pgo.Options(method=1))
    s.set_poses(np.loadtxt(os.path.join(save, "opt_nodes.txt"))[:, 1:])
    _, cov, _ = s.sample(32, seed=5, want_deltas=False)
    got = rows[:, 1:]
    ref = cov.reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]]
    assert np.abs(got - ref).max() <= 1e-8 * np.abs(ref).max()
    assert np.array_equal(got[0], np.zeros(6))
    s.close()
    p = subprocess.run([exe, "INTEL", "0", "2", "--data", DATA, "--save", save, "--sample-cov", "8"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--sample-cov" in p.stderr
