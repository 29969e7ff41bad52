"""Absolute pose priors (pgo_set_priors, csrc/prior.h, csrc/prior.hip.h) on the GPU.

References: the numpy restatement tests/_prior_restatement.py (pinned on the CPU by tests/test_prior_host.py), and an
independent route that knows no priors: the same information as edges from one extra constant pose (anchor edges).

Where this departs from a handle "anchored by priors alone" on the direct solve: the plan of a handle is decided at creation,
and it refuses the direct solve without a constant pose (tests/test_gpu_parity.py and tests/test_plan_native.py pin that), so
the direct runs below keep fixed_pose = 0 NEXT to the priors -- which is what shows that k_dlr_setup carries the priors' blocks:
pgo_get_info reports linear_solver 2 with direct_fallbacks == 0, and the refinement step against K3's matrix would fail if T
lacked them."""
import math
import os

import numpy as np
import pytest

import _gnc_restatement as GR
import _loss_restatement as LR
import _mixture_cases as MC
import _prior_restatement as PR
from conftest import DATA, GOLDEN, oracle_graph

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -8, -1
EPS = np.finfo(np.float64).eps
LOSSES = [("trivial", 0.0), ("huber", 0.5), ("softlone", 0.5), ("cauchy", 0.5), ("arctan", 0.5), ("tukey", 2.0)]
COUNTS = (1, 63, 64, 65, 256, 257)   # the wave and workgroup edges of the cost fold
HUBER = ("huber", 0.01)
# the bound tests/test_gpu_loss.py applies to its 50-iteration solves against its restatement (test_lm_matches_restatement)
XY_BOUND, TH_BOUND = 5e-6, 1e-4


def sub(pgo, n, extra_pose=False):
    """poses < n of the synthetic 2000-pose graph; extra_pose: one more pose that no edge touches"""
    z = np.load(os.path.join(GOLDEN, "synth_manhattan_2000_s7.npz"))
    keep = (z["ia"] < n) & (z["ib"] < n)
    poses = z["poses"][:n]
    if extra_pose:
        poses = np.vstack([poses, [[3.0, -2.0, 0.4]]])
    return pgo.Graph.from_arrays(poses, z["ia"][keep], z["ib"][keep], z["meas"][keep], z["kind"][keep])


def history(s):
    return [{k: v for k, v in r.items() if k != "seconds"} for r in s.iter_records()]


def random_priors(N, n, seed, x, forced=(), signed=True):
    """n priors: the forced poses first, then a random choice; means near x; informations SPD, position-only, rank one and zero in
    turn.  signed=False: every entry of every information and every component of every residual is >= 0, so that Lambda d and
    d' Lambda d are sums of terms of one sign -- the inputs at which the operator test's elementwise bound, a few eps of the
    RESULT, is what fp64 can give (with mixed signs Lambda d cancels and its rounding error, a few eps of the TERMS, exceeds any
    bound stated on the result)."""
    rng = np.random.default_rng(seed)
    pose = list(forced[:n])
    rest = np.setdiff1d(np.arange(N), pose)
    pose += rng.choice(rest, n - len(pose), replace=False).tolist()
    pose = np.array(pose)
    noise = rng.normal(size=(n, 3)) * np.array([0.4, 0.4, 0.2])
    mean = x[pose] + (noise if signed else -np.abs(noise) - 1e-3)
    mean[::5, 2] += 2.0 * math.pi if signed else -2.0 * math.pi   # the wrap
    B = rng.normal(size=(n, 3, 3)) if signed else rng.uniform(0.1, 1.0, size=(n, 3, 3))
    info = np.einsum("nij,nkj->nik", B, B) * 4.0
    info[1::4] = np.diag([3.0, 3.0, 0.0])
    info[2::4] = np.einsum("ni,nj->nij", B[2::4, 0], B[2::4, 0])
    if n > 7:
        info[7] = 0.0
    info = 0.5 * (info + np.transpose(info, (0, 2, 1)))
    return PR.make(pose, mean, info)


def apply(pgo, s, pri, loss):
    s.set_priors(pri["pose"], pri["mean"], pri["info"], pgo.Loss(*loss) if loss is not None else None)


# ------------------------------------------------------------------ 3. the operator
def _operator_case(pgo, s, N, x, pri, loss, fixed, what, signed=False):
    """signed: the priors' terms have mixed signs -- the bound then also carries 16 eps of the terms' magnitudes"""
    s.clear_priors()
    s.set_poses(x)
    g0, h0 = s.normal_eq()
    c0 = s.evaluate(want_r=False, want_J=False)[0]
    apply(pgo, s, pri, loss)
    assert s.n_priors == len(pri["pose"])
    g1, h1 = s.normal_eq()
    c1 = s.evaluate(want_r=False, want_J=False)[0]
    scale = np.ones((N, 3))
    if fixed >= 0:
        scale[fixed] = 0.0
    # chi2 first, on its own; the loss is then evaluated at the DEVICE's chi2, so that the elementwise bound below judges the
    # assembly and not the conditioning of rho' near a loss's bend (the loss functions themselves: tests/test_prior_native.py)
    d_ref, chi_ref = PR.residuals(pri, x)
    d, chi2 = s.prior_residuals()
    assert np.all(np.abs(d - d_ref) <= 4 * EPS * np.abs(d_ref)), what
    mag = np.einsum("ni,nij,nj->n", np.abs(d_ref), np.abs(pri["info"]), np.abs(d_ref))
    assert np.all(np.abs(chi2 - chi_ref) <= 8 * EPS * mag), what
    dH, dg, dc = PR.normal_eq_terms(pri, loss or ("trivial", 0.0), x, scale, chi2=chi2)
    ref_h, ref_g = np.zeros((N, 3, 3)), np.zeros((N, 3))
    ref_h[pri["pose"]], ref_g[pri["pose"]] = dH, dg
    got_h, got_g = (h1 - h0).reshape(N, 3, 3), (g1 - g0).reshape(N, 3)
    bound_h = 16 * EPS * (np.abs(h1) + np.abs(h0)).reshape(N, 3, 3)
    bound_g = 16 * EPS * (np.abs(g1) + np.abs(g0)).reshape(N, 3)
    if signed:
        absd = dict(pri, info=np.abs(pri["info"]), mean=x[pri["pose"]] - np.abs(PR.residuals(pri, x)[0]))
        bound_g[pri["pose"]] += 16 * EPS * np.abs(PR.normal_eq_terms(absd, ("trivial", 0.0), x, scale)[1])
    assert np.all(np.abs(got_h - ref_h) <= bound_h), (what, np.abs(got_h - ref_h).max())
    assert np.all(np.abs(got_g - ref_g) <= bound_g), (what, np.abs(got_g - ref_g).max())
    assert abs((c1 - c0) - dc) <= 16 * EPS * (abs(c1) + abs(c0)), (what, c1 - c0, dc)
    # rows without a prior, and the constant pose: exactly nothing
    quiet = np.ones(N, bool)
    quiet[pri["pose"]] = False
    if fixed >= 0:
        quiet[fixed] = True
    assert not got_h[quiet].any() and not got_g[quiet].any(), what
    # repeated calls: bitwise, and k_prior_add does not depend on its grid
    g2, h2 = s.normal_eq()
    assert g2.tobytes() == g1.tobytes() and h2.tobytes() == h1.tobytes(), what
    pgo.set_knob("prior_add_grid", 3)
    try:
        g3, h3 = s.normal_eq()
    finally:
        pgo.set_knob("prior_add_grid", -1)
    assert g3.tobytes() == g1.tobytes() and h3.tobytes() == h1.tobytes(), what
    assert s.evaluate(want_r=False, want_J=False)[0] == c1
    # the residuals, in the caller's order, at given poses too (at the handle's own: above)
    y = x + 0.01
    d_ref, chi_ref = PR.residuals(pri, y)
    d, chi2 = s.prior_residuals(y)
    mag = np.einsum("ni,nij,nj->n", np.abs(d_ref), np.abs(pri["info"]), np.abs(d_ref))
    assert np.all(np.abs(d - d_ref) <= 4 * EPS * np.abs(d_ref)) and np.all(np.abs(chi2 - chi_ref) <= 8 * EPS * mag), what
    return c1 - c0


@pytest.mark.parametrize("iw", [0, 1])
def test_operator_two_poses(pgo, iw):
    """N = 2, one edge: a prior on the constant pose (exactly nothing but the cost), on the free pose, on both"""
    poses = np.array([[0.0, 0.0, 0.1], [1.0, 0.2, 0.3]])
    g = pgo.Graph.from_arrays(poses, [0], [1], [[0.9, 0.1, 0.25]], [0], info=[[2.0, 0.1, 0.0, 3.0, 0.2, 5.0]])
    s = pgo.Solver(g, pgo.Options(method=1, info_weighting=iw))
    for k, loss in enumerate(LOSSES):
        for forced in ((0,), (1,), (1, 0)):
            pri = random_priors(2, len(forced), 10 * k + len(forced), poses, forced, signed=False)
            dc = _operator_case(pgo, s, 2, poses, pri, loss, 0, (iw, loss, forced))
            assert dc > 0.0   # the constant pose's prior still counts in the cost
            _operator_case(pgo, s, 2, poses, random_priors(2, len(forced), k, poses, forced), loss, 0, (iw, loss, forced, "signed"), signed=True)
    s.close()


@pytest.mark.parametrize("iw", [0, 1])
def test_operator_300_poses(pgo, iw):
    """N = 301: the first row (the constant pose), the last row (a pose without edges), rows 255 and 256, every count, every loss"""
    n = 300
    g = sub(pgo, n, extra_pose=True)
    N = n + 1
    s = pgo.Solver(g, pgo.Options(method=1, info_weighting=iw))
    rng = np.random.default_rng(2)
    x = np.array(g.poses) + 0.05 * rng.standard_normal((N, 3))
    for k, count in enumerate(COUNTS):
        for j, loss in enumerate(LOSSES):
            pri = random_priors(N, count, 100 * k + j, x, (255, 0, N - 1, 256, n - 1), signed=False)
            _operator_case(pgo, s, N, x, pri, loss, 0, (iw, count, loss))
    _operator_case(pgo, s, N, x, random_priors(N, 257, 5, x, (255, 0, N - 1, 256, n - 1)), ("cauchy", 0.5), 0, (iw, "signed"), signed=True)
    s.close()


def test_operator_70000_poses(pgo):
    """the internal locality ordering is on: rows are not the caller's poses; several workgroups of k_edge_eval partials in front"""
    N = 70000
    g = pgo.synth_manhattan(N)
    s = pgo.Solver(g, pgo.Options(method=1))
    assert s.info().pose_ordering == 1
    rng = np.random.default_rng(4)
    x = np.array(g.poses) + 0.02 * rng.standard_normal((N, 3))
    for k, count in enumerate(COUNTS + (5000,)):
        loss = LOSSES[k % len(LOSSES)]
        pri = random_priors(N, count, 7 + k, x, (255, 0, N - 1, 256), signed=False)
        _operator_case(pgo, s, N, x, pri, loss, 0, (count, loss))
    _operator_case(pgo, s, N, x, random_priors(N, 257, 5, x, (255, 0, N - 1, 256)), ("huber", 0.5), 0, "signed", signed=True)
    s.close()


# ------------------------------------------------------------------ 4. neutrality
def _handles(pgo, kind):
    if kind == "intel":   # the default K1 instantiation (Huber), the direct solve
        g = pgo.ReadG2O(os.path.join(DATA, "INTEL.g2o"))
        g.add_random_C(50, 1)
        mk = lambda: pgo.Solver(g, pgo.Options(method=1, max_iters=6))
    else:                 # a weight plane: K1's general instantiation
        g = sub(pgo, 300)
        w = np.random.default_rng(3).random(g.n_edges)
        w[np.array(g.kind) == 0] = 1.0

        def mk():
            s = pgo.Solver(g, pgo.Options(method=0, max_iters=6))
            s.set_edge_weights(w)
            return s
    return g, mk


@pytest.mark.parametrize("kind", ["intel", "weights"])
def test_zero_information_and_set_then_clear_are_neutral(pgo, kind):
    g, mk = _handles(pgo, kind)
    x0 = np.array(g.poses)
    a, b, c = mk(), mk(), mk()
    pri = random_priors(g.n_poses, 40, 1, x0, (0, g.n_poses - 1))
    zero = PR.make(pri["pose"], pri["mean"], np.zeros((40, 3, 3)))
    apply(pgo, b, zero, ("cauchy", 0.3))
    apply(pgo, c, pri, HUBER)
    c.lm_begin()
    c.lm_step(2)
    assert np.abs(c.poses() - x0).max() > 1e-3
    c.clear_priors()
    assert c.n_priors == 0
    c.set_poses(x0)
    sa, sb, sc = a.solve(), b.solve(), c.solve()
    for s, t in ((b, sb), (c, sc)):
        assert (sa.final_cost, sa.iterations, sa.termination) == (t.final_cost, t.iterations, t.termination)
        assert history(a) == history(s) and a.poses().tobytes() == s.poses().tobytes()
        assert a.info().linear_solver == s.info().linear_solver and s.info().direct_fallbacks == 0
    for s in (a, b, c):
        s.close()


# ------------------------------------------------------------------ 5. equivalence with anchor edges
@pytest.fixture(scope="module")
def anchor(pgo, oracle):
    """the construction of tests/test_prior_host.py per (method, outliers): graphs, priors, start"""
    out = {}
    for method, n_out in ((0, 0), (1, 50)):
        og = oracle.read_g2o(os.path.join(DATA, "INTEL.g2o"))
        if n_out:
            og = oracle.add_random_C(og, n_out, 1)
        ident = np.tile(PR.info6(np.eye(3)[None]), (og.n_edges, 1))
        og_i = oracle.Graph(np.array(og.pose_id), np.array(og.poses), np.array(og.ia), np.array(og.ib), np.array(og.meas), ident, np.array(og.kind))
        start = LR.lm(oracle, og_i, [HUBER], LR.classes(og_i.kind, 1), method=method, info_weighting=True).poses
        og_a, og_b, pri = PR.anchor_case(oracle, og_i, start)
        out[method] = (og_a, og_b, pri)
    return out


def _pgo_graph(pgo, og):
    return pgo.Graph.from_arrays(np.array(og.poses), np.array(og.ia), np.array(og.ib), np.array(og.meas), np.array(og.kind), info=np.array(og.info))


@pytest.mark.parametrize("method", [0, 1])
def test_priors_equal_anchor_edges_on_the_device(pgo, oracle, anchor, method):
    """METHOD 1: K1 states DCS in two forms -- on chi2 under info_weighting, on the plain residual without -- so the anchor
    route, which needs info mode for the anchor edges' Omega, is the same problem as the prior handle under info_weighting = 1
    only; the direct solve (which refuses info mode) is then compared with a reference that is as independent of the device:
    the numpy restatement on the same graph, priors and start, in the plain mode."""
    og_a, og_b, pri = anchor[method]
    N = og_b.n_poses
    ga, gb = _pgo_graph(pgo, og_a), _pgo_graph(pgo, og_b)
    tight = dict(method=method, pcg_rtol=1e-12, pcg_max_iters=400000)
    # ---- no constant pose: the gauge comes from the priors alone (PCG; see the module docstring)
    a = pgo.Solver(ga, pgo.Options(fixed_pose=N, info_weighting=1, linear_solver=1, **tight))
    sa = a.solve()
    xa, ha = a.poses(), history(a)
    for iw in ((0, 1) if method == 0 else (1,)):
        b = pgo.Solver(gb, pgo.Options(fixed_pose=-1, info_weighting=iw, linear_solver=1, **tight))
        apply(pgo, b, pri, HUBER)
        sb = b.solve()
        xb = b.poses()
        d_xy, d_th = np.abs(xa[:N, :2] - xb[:, :2]).max(), np.abs(xa[:N, 2] - xb[:, 2]).max()
        print(f"METHOD {method} PCG iw {iw}: {sb.iterations} iterations, final cost {sb.final_cost:.9e} / {sa.final_cost:.9e}, "
              f"max |d translation| {d_xy:.2e}, |d heading| {d_th:.2e}")
        assert [r["step_ok"] for r in history(b)] == [r["step_ok"] for r in ha]
        assert (sb.iterations, sb.termination) == (sa.iterations, sa.termination)
        assert d_xy < XY_BOUND and d_th < TH_BOUND
        assert np.abs(PR.residuals(pri, xb)[0][:, 2]).max() < 0.5 * math.pi
        b.close()
    a.close()
    # ---- the direct solve: pose 0 constant in both routes, next to the priors
    if method == 0:
        a = pgo.Solver(ga, pgo.Options(fixed_pose=N, info_weighting=1, linear_solver=1, **tight))
        const = np.zeros(N + 1, np.uint8)
        const[0] = 1
        a.set_active(pose_constant=const)
        sa = a.solve()
        xa, ha, cost_a = a.poses(), history(a), sa.final_cost
        a.close()
    else:
        ref = PR.lm(oracle, og_b, [HUBER], LR.classes(og_b.kind, 1), priors=pri, prior_loss=HUBER, method=1, fixed_pose=0)
        xa, ha, cost_a = ref.poses, ref.records, ref.final_cost
    b = pgo.Solver(gb, pgo.Options(fixed_pose=0, info_weighting=0, linear_solver=2, method=method))
    apply(pgo, b, pri, HUBER)
    sb = b.solve()
    xb = b.poses()
    d_xy, d_th = np.abs(xa[:N, :2] - xb[:, :2]).max(), np.abs(xa[:N, 2] - xb[:, 2]).max()
    print(f"METHOD {method} direct: {sb.iterations} iterations, final cost {sb.final_cost:.9e} / {cost_a:.9e}, "
          f"max |d translation| {d_xy:.2e}, |d heading| {d_th:.2e}, fallbacks {b.info().direct_fallbacks}")
    assert b.info().linear_solver == 2 and b.info().direct_fallbacks == 0
    assert [r["step_ok"] for r in history(b)] == [r["step_ok"] for r in ha]
    assert d_xy < XY_BOUND and d_th < TH_BOUND
    b.close()


# ------------------------------------------------------------------ 6. against the restatement
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("solver", [0, 1])
def test_lm_with_priors_matches_the_restatement(pgo, oracle, method, solver):
    """INTEL + 50, 10 priors under Huber(0.5), from the file's poses, 50 iterations; solver 0 = the library's choice (direct)"""
    g = pgo.ReadG2O(os.path.join(DATA, "INTEL.g2o"))
    g.add_random_C(50, 1)
    og = oracle_graph(oracle, g)
    x0 = np.array(g.poses)
    rng = np.random.default_rng(21)
    pose = np.sort(rng.choice(np.arange(1, g.n_poses), 10, replace=False))
    B = rng.normal(size=(10, 3, 3))
    info = np.einsum("nij,nkj->nik", B, B) * 20.0 + np.eye(3)
    info[3] = np.diag([50.0, 50.0, 0.0])
    pri = PR.make(pose, x0[pose] + rng.normal(size=(10, 3)) * np.array([0.5, 0.5, 0.1]), info)
    loss = ("huber", 0.5)
    ref = PR.lm(oracle, og, [HUBER], LR.classes(og.kind, 1), priors=pri, prior_loss=loss, method=method)
    opt = dict(method=method, pcg_max_iters=400000, linear_solver=solver)
    if solver == 1:
        opt["pcg_rtol"] = 1e-12
    s = pgo.Solver(g, pgo.Options(**opt))
    apply(pgo, s, pri, loss)
    summ = s.solve()
    x = s.poses()
    recs = s.iter_records()
    d_xy, d_th = np.abs(x[:, :2] - ref.poses[:, :2]).max(), np.abs(x[:, 2] - ref.poses[:, 2]).max()
    print(f"METHOD {method} solver {s.info().linear_solver} (fallbacks {s.info().direct_fallbacks}): {summ.iterations} iterations, "
          f"final cost {summ.final_cost:.9e}, max |d translation| {d_xy:.2e}, |d heading| {d_th:.2e}")
    assert summ.termination == ref.termination and summ.iterations == ref.iterations
    assert summ.initial_cost == pytest.approx(ref.initial_cost, rel=1e-12)
    assert [a["step_ok"] for a in recs] == [b["step_ok"] for b in ref.records]
    for a, b in zip(recs, ref.records):
        assert a["cost"] == pytest.approx(b["cost"], rel=1e-6)
    assert recs[0]["gradient_max_norm"] == pytest.approx(ref.records[0]["gradient_max_norm"], rel=1e-10)   # the priors are in the gradient norm
    assert d_xy < XY_BOUND and d_th < TH_BOUND
    if solver == 0:
        assert s.info().linear_solver == 2 and s.info().direct_fallbacks == 0
    s.close()


# ------------------------------------------------------------------ 7. closed form
# cost <= 1e-20 needs the solve to run to the gradient: Ceres' function and parameter tolerances stop a step short of it
TO_THE_END = dict(ftol=0.0, ptol=0.0, gtol=1e-13)


def _compose(z, m):
    c, s_ = math.cos(z[2]), math.sin(z[2])
    return np.array([z[0] + c * m[0] - s_ * m[1], z[1] + s_ * m[0] + c * m[1], z[2] + m[2]])


def _two_poses(pgo, first, m):
    """two poses joined by one edge m, the second exactly where the edge puts it; no constant pose, no loss"""
    x0 = np.array([first, _compose(first, m)])
    g = pgo.Graph.from_arrays(x0, [0], [1], [m], [0])
    return x0, pgo.Solver(g, pgo.Options(method=0, fixed_pose=-1, **TO_THE_END), losses=pgo.Loss("trivial"))


def test_closed_form_two_poses(pgo):
    m = np.array([1.0, 0.5, 0.3])
    x0, s = _two_poses(pgo, [0.2, -0.1, 0.4], m)
    z = np.array([1.5, -0.7, 0.9])
    B = np.array([[2.0, 0.3, 0.1], [0.0, 1.5, -0.2], [0.0, 0.0, 1.1]])
    Lam = B.T @ B
    s.set_priors([0], [z], [Lam])
    summ = s.solve()
    x = s.poses()
    print(f"PD prior: {summ.iterations} iterations, cost {summ.final_cost:.3e}, |x0 - z| {np.abs(x[0] - z).max():.2e}")
    assert summ.final_cost <= 1e-20
    assert np.abs(x[0] - z).max() < 1e-9 and np.abs(x[1] - _compose(z, m)).max() < 1e-9
    cov, rep = s.covariance([0], solver=0, rtol=1e-13)
    ref = np.linalg.inv(Lam)
    assert np.abs(cov[0] - ref).max() <= 1e-9 * np.abs(ref).max()
    # solver = 1 needs a handle on the direct solve, which a handle without a constant pose never is: the status of today
    with pytest.raises(pgo.PgoError) as e:
        s.covariance([0], solver=1)
    assert e.value.status == UNSUPPORTED
    s.close()
    # ---- position only: x, y go to z, the heading is not moved, the edge stays satisfied; no gauge for a covariance.
    # The heading of the pair is a gauge freedom here, and an LM step is orthogonal to it in the metric of its diagonal D, not in
    # the plain one: the heading stays for a displacement ALONG the line that joins the two poses (the pure translation is then
    # D-orthogonal to the rotation about pose 0 whatever D is), which is the case stated here.
    m = np.array([1.0, 0.0, 0.3])
    x0, s = _two_poses(pgo, [0.2, -0.1, 0.0], m)
    z = np.array([1.5, -0.1, 2.0])
    s.set_priors([0], [z], [np.diag([4.0, 4.0, 0.0])])
    summ = s.solve()
    x = s.poses()
    assert summ.final_cost <= 1e-20
    assert np.abs(x[0, :2] - z[:2]).max() < 1e-9 and abs(x[0, 2] - x0[0, 2]) < 1e-9
    assert np.abs(x[1] - _compose(x[0], m)).max() < 1e-9
    with pytest.raises(pgo.PgoError) as e:
        s.covariance([0])
    free = pgo.Solver(pgo.Graph.from_arrays(x0, [0], [1], [m], [0]), pgo.Options(method=0, fixed_pose=-1))
    with pytest.raises(pgo.PgoError) as e0:
        free.covariance([0])
    assert e.value.status == e0.value.status == UNSUPPORTED
    free.close(); s.close()


def test_covariance_and_gate_see_the_priors_on_both_solvers(pgo, oracle):
    """300 poses on the direct solve, pose 0 constant, priors on 20 poses: solver 0 and 1 agree with a dense inverse of
    J'J + the priors' blocks, and the gate's P shrinks where a prior sits"""
    n = 300
    g, og = sub(pgo, n), GR.subgraph(oracle, n)
    s = pgo.Solver(g, pgo.Options(method=0), losses=pgo.Loss("trivial"))
    assert s.info().linear_solver == 2
    x = np.array(g.poses)
    pri = random_priors(n, 20, 6, x, (n - 1, 150))
    _, _, J = LR.evaluate(oracle, og, GR.TRIVIAL, np.zeros(og.n_edges, np.int64), x, 0)
    H = np.zeros((3 * n, 3 * n))
    ia, ib = np.asarray(og.ia), np.asarray(og.ib)
    for e in range(og.n_edges):
        cols = np.r_[3 * ia[e]:3 * ia[e] + 3, 3 * ib[e]:3 * ib[e] + 3]
        Je = J[e].reshape(3, 6)
        H[np.ix_(cols, cols)] += Je.T @ Je
    H0 = H.copy()
    for p, L in zip(pri["pose"], pri["info"]):
        H[3 * p:3 * p + 3, 3 * p:3 * p + 3] += L
    idx = [1, 150, n - 1, int(pri["pose"][5])]
    ref = np.linalg.inv(H[3:, 3:])
    ref0 = np.linalg.inv(H0[3:, 3:])
    apply(pgo, s, pri, None)
    for solver in (0, 1):
        cov, rep = s.covariance(idx, solver=solver)
        for j, i in enumerate(idx):
            blk = ref[3 * i - 3:3 * i, 3 * i - 3:3 * i]
            assert np.abs(cov[j] - blk).max() <= 1e-7 * np.abs(blk).max(), (solver, i)
        i = n - 1
        assert np.abs(cov[2] - ref0[3 * i - 3:3 * i, 3 * i - 3:3 * i]).max() > 0.1 * np.abs(cov[2]).max()   # not the prior-free blocks
    out0, _ = s.gate([10], [n - 1], [[0.0, 0.0, 0.0]], solver=0)
    out1, _ = s.gate([10], [n - 1], [[0.0, 0.0, 0.0]], solver=1)
    assert np.abs(out0["P"] - out1["P"]).max() <= 1e-7 * np.abs(out0["P"]).max()
    s.clear_priors()
    outc, _ = s.gate([10], [n - 1], [[0.0, 0.0, 0.0]], solver=1)
    assert np.trace(outc["P"][0]) > 1.05 * np.trace(out1["P"][0])
    s.close()


def test_a_prior_is_a_gauge_while_its_pose_is_free(pgo):
    """three poses in a chain, no constant pose, a positive definite prior on pose 2 only: switching the edge (1, 2) off makes
    pose 2 constant (no active edge) and takes the gauge away; switching it on again brings it back -- in either call order"""
    x0 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [2.0, 0.1, 0.2]])
    g = pgo.Graph.from_arrays(x0, [0, 1], [1, 2], [[1.0, 0.0, 0.1], [1.0, 0.0, 0.1]], [0, 0])
    off = np.array([1, 0], np.uint8)
    for first in ("priors", "mask"):
        s = pgo.Solver(g, pgo.Options(method=0, fixed_pose=-1), losses=pgo.Loss("trivial"))
        if first == "priors":
            s.set_priors([2], [[2.0, 0.0, 0.2]], [np.diag([4.0, 5.0, 6.0])])
            s.set_active(edge_active=off)
        else:
            s.set_active(edge_active=off)
            s.set_priors([2], [[2.0, 0.0, 0.2]], [np.diag([4.0, 5.0, 6.0])])
        with pytest.raises(pgo.PgoError) as e:
            s.covariance([0])
        assert e.value.status == UNSUPPORTED, first
        s.set_active()
        cov, _ = s.covariance([2], rtol=1e-13)
        assert np.abs(cov[0] - np.diag([1 / 4.0, 1 / 5.0, 1 / 6.0])).max() < 1e-9, first   # pose 2's marginal is the prior's
        s.close()


# ------------------------------------------------------------------ 8. the wrap
def test_heading_wraps_across_the_cut(pgo):
    x0, s = _two_poses(pgo, [0.0, 0.0, -3.1], np.array([1.0, 0.0, 0.0]))
    s.set_priors([0], [[0.0, 0.0, 3.1]], [np.eye(3)])
    d, chi2 = s.prior_residuals()
    assert d[0, 2] == pytest.approx(2.0 * math.pi - 6.2, abs=1e-15) and abs(d[0, 2] - 0.0832) < 1e-4   # not -6.2
    summ = s.solve()
    x = s.poses()
    assert summ.final_cost <= 1e-20
    assert x[0, 2] < -math.pi and abs(x[0, 2] - (3.1 - 2.0 * math.pi)) < 1e-9   # across the cut, by the short way
    s.close()


# ------------------------------------------------------------------ 9. the contract
def test_errors_leave_the_handle_unchanged(pgo):
    g = sub(pgo, 300)
    N = g.n_poses
    x = np.array(g.poses)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=4))
    pri = random_priors(N, 9, 12, x, (0, N - 1))
    apply(pgo, s, pri, ("cauchy", 0.4))
    c_ref, (d_ref, chi_ref) = s.evaluate(want_r=False, want_J=False)[0], s.prior_residuals()
    I = np.tile(np.eye(3), (2, 1, 1))
    z = np.zeros((2, 3))
    bad = [(([1, N], z, I, None), "prior 1: pose %d out of range" % N), (([-1, N], z, I, None), "prior 0: pose -1 out of range"),
           (([5, 5], z, I, None), "prior 1: pose 5 already has a prior"),
           (([1, 2], np.array([[0, 0, 0], [0, np.nan, 0]]), I, None), "prior 1: the mean is not finite"),
           (([1, 2], z, np.array([np.eye(3), np.diag([1.0, np.inf, 1.0])]), None), "prior 1: the information is not finite"),
           (([1, 2], z, np.array([np.eye(3), np.diag([1.0, -1e-6, 1.0])]), None), "prior 1: the information has a negative eigenvalue"),
           (([1, 2], z, I, pgo.Loss("huber", -1.0)), "loss")]
    for args, text in bad:
        with pytest.raises(pgo.PgoError) as e:
            s.set_priors(*args)
        assert e.value.status == INVALID and text in str(e.value), (text, str(e.value))   # (the first offender is named)
    L = pgo.lib()
    import ctypes as C
    one = np.zeros(6)
    ip, dp = np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), one.ctypes.data_as(C.POINTER(C.c_double))
    for args in ((1, None, dp, dp), (1, ip, None, dp), (1, ip, dp, None), (-1, ip, dp, dp)):
        assert L.pgo_set_priors(s._h, *args, None) == INVALID
    assert s.n_priors == 9 and s.evaluate(want_r=False, want_J=False)[0] == c_ref
    d, chi2 = s.prior_residuals()
    assert d.tobytes() == d_ref.tobytes() and chi2.tobytes() == chi_ref.tobytes()
    s.close()
    # the handles priors refuse
    m2 = pgo.Solver(g, pgo.Options(method=2))
    with pytest.raises(pgo.PgoError) as e:
        m2.set_priors([1], [[0, 0, 0]], [np.eye(3)])
    assert e.value.status == UNSUPPORTED and m2.n_priors == 0
    m2.close()


def test_forced_collectives_refuse_priors(pgo, monkeypatch):
    monkeypatch.setenv("PGO_FORCE_COLLECTIVES", "1")
    u = pgo.Solver(sub(pgo, 66), pgo.Options(method=1))
    monkeypatch.delenv("PGO_FORCE_COLLECTIVES")
    with pytest.raises(pgo.PgoError) as e:
        u.set_priors([1], [[0, 0, 0]], [np.eye(3)])
    assert e.value.status == UNSUPPORTED and u.n_priors == 0
    u.close()


def test_stale_rule_and_the_other_setters(pgo):
    g = sub(pgo, 300)
    N = g.n_poses
    x = np.array(g.poses)
    pri = random_priors(N, 12, 8, x, (0, N - 1))
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.lm_begin()
    s.lm_step(1)
    apply(pgo, s, pri, HUBER)
    with pytest.raises(pgo.PgoError) as e:
        s.lm_step(1)
    assert e.value.status == INVALID
    s.lm_begin()
    s.lm_step(1)
    s.clear_priors()
    with pytest.raises(pgo.PgoError) as e:
        s.lm_step(1)
    assert e.value.status == INVALID
    s.close()
    # pgo_set_losses / pgo_set_active / pgo_set_edge_weights leave the priors alone, in either call order
    w = np.random.default_rng(1).random(g.n_edges)
    act = np.ones(g.n_edges, np.uint8)
    act[np.nonzero(np.array(g.kind) != 0)[0][::3]] = 0
    setters = [lambda t: t.set_losses(pgo.Loss("cauchy", 0.2)), lambda t: t.set_active(edge_active=act), lambda t: t.set_edge_weights(w)]
    for k, setter in enumerate(setters):
        a, b = pgo.Solver(g, pgo.Options(method=1, max_iters=4)), pgo.Solver(g, pgo.Options(method=1, max_iters=4))
        apply(pgo, a, pri, HUBER); setter(a)
        setter(b); apply(pgo, b, pri, HUBER)
        assert a.n_priors == b.n_priors == 12
        assert a.prior_residuals()[1].tobytes() == b.prior_residuals()[1].tobytes()
        sa, sb = a.solve(), b.solve()
        assert history(a) == history(b) and a.poses().tobytes() == b.poses().tobytes(), k
        free = pgo.Solver(g, pgo.Options(method=1, max_iters=4))
        setter(free)
        free.solve()
        assert np.abs(free.poses() - a.poses()).max() > 1e-4   # ... and they are in the problem
        for t in (a, b, free):
            t.close()


def test_window_solve_refuses_while_priors_are_set(pgo):
    g = sub(pgo, 300)
    s = pgo.Solver(g, pgo.Options(method=0))
    loops = np.nonzero(np.array(g.kind) != 0)[0]
    win = pgo.window_plan(g.n_poses, np.array(g.ia), np.array(g.ib), np.array(g.kind), [int(loops[0])], 5)
    before = s.window_solve([win])
    s.set_priors([3], [[0.0, 0.0, 0.0]], [np.eye(3)])
    with pytest.raises(pgo.PgoError) as e:
        s.window_solve([win])
    assert e.value.status == UNSUPPORTED
    s.clear_priors()
    after = s.window_solve([win])
    assert np.asarray(before[0]).tobytes() == np.asarray(after[0]).tobytes()
    s.close()


def test_gnc_and_mixture_solves_carry_the_priors(pgo, oracle):
    """the 500-pose worlds of _gnc_restatement / _mixture_cases with 5 priors: both run, the LM solves inside include the priors
    (no accepted step raises the cost), and the mixture objective, priors included, never rises beyond its summation bound"""
    n = 500
    g, og = sub(pgo, n), GR.subgraph(oracle, n)
    x0 = np.array(g.poses)
    truth_like = random_priors(n, 5, 30, x0, (n - 1, 250))
    pri = PR.make(truth_like["pose"], truth_like["mean"], np.tile(np.diag([25.0, 25.0, 0.0]), (5, 1, 1)))

    def lm_costs_fall(s):
        recs = s.iter_records()
        ok = [r["cost"] for r in recs if r["step_ok"] == 1]
        assert len(ok) >= 2 and all(b <= a for a, b in zip(ok, ok[1:]))

    s = pgo.Solver(g, pgo.Options(method=0), losses=pgo.Loss("trivial"))
    apply(pgo, s, pri, None)
    summ, rounds = s.gnc_solve(0.5)
    assert summ["rounds"] >= 1 and len(rounds) == summ["rounds"]
    lm_costs_fall(s)
    with_pri = s.evaluate(want_r=False, want_J=False)[0]
    share = PR.cost(pri, ("trivial", 0.0), s.poses())
    s.clear_priors()
    without = s.evaluate(want_r=False, want_J=False)[0]
    assert share > 0.0 and abs((with_pri - without) - share) <= 1e-12 * with_pri
    s.close()

    (edge, ptr, comps), roles = MC.planted(og)
    s = pgo.Solver(g, pgo.Options(method=0), losses=pgo.Loss("trivial"))
    s.set_mixtures(edge, ptr, comps)
    apply(pgo, s, pri, None)
    summ, rounds = s.mixture_solve()
    F = [r["objective"] for r in rounds] + [summ["objective"]]
    print("mixture objective per round, priors included:", ["%.9e" % f for f in F])
    assert summ["rounds"] >= 1
    for a, b in zip(F, F[1:]):
        assert b <= a + MC.summation_bound(g.n_edges, abs(a))
    lm_costs_fall(s)
    s.clear_priors()
    summ2, _ = s.mixture_solve()
    assert summ2["objective"] < summ["objective"]   # the priors' share is gone
    s.close()
