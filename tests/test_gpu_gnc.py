"""The edge weight plane (pgo_set_edge_weights) and graduated non-convexity (pgo_gnc_update, pgo_gnc_solve) on the GPU.

Inputs: the sub-graphs "poses < N" of tests/golden/synth_manhattan_2000_s7.npz.  Unless a test says otherwise the handle is
METHOD 0 with the Trivial loss (set_losses) on the default linear solver.  The end-to-end reference is the numpy restatement
tests/_gnc_restatement.py, pinned by tests/test_gnc_host.py."""
import math
import os

import numpy as np
import pytest

import _gnc_restatement as GR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -8, -1
CBAR = 0.5


def sub(pgo, n, drop_bogus=False):
    z = np.load(os.path.join(GOLDEN, "synth_manhattan_2000_s7.npz"))
    keep = (z["ia"] < n) & (z["ib"] < n)
    if drop_bogus:
        keep &= z["kind"] != 2
    return pgo.Graph.from_arrays(z["poses"][:n], z["ia"][keep], z["ib"][keep], z["meas"][keep], z["kind"][keep])


def trivial(pgo, g, **opt):
    opt.setdefault("method", 0)
    return pgo.Solver(g, pgo.Options(**opt), losses=pgo.Loss("trivial"))


def history(s):
    return [{k: v for k, v in r.items() if k != "seconds"} for r in s.iter_records()]


def random_weights(E, seed):
    rng = np.random.default_rng(seed)
    w = rng.random(E)
    w[rng.choice(E, E // 8, replace=False)] = 0.0
    w[rng.choice(E, E // 8, replace=False)] = 1.0
    w[0], w[1], w[-1] = 0.0, 1.0, 0.37
    return w


# ------------------------------------------------------------------ 1. K1 with weights
@pytest.mark.parametrize("n", [300, 66])
@pytest.mark.parametrize("kind", ["trivial", "huber", "dcs"])
def test_k1_with_weights(pgo, n, kind):
    """r and J rows = sqrt(w) x the rows without the plane, w = 0 rows exactly zero, cost = sum w cost_e; E = 717 (three
    workgroups, the last one partial) and E = 100 (less than one)"""
    g = sub(pgo, n)
    E = g.n_edges
    assert E == {300: 717, 66: 100}[n]
    if kind == "trivial":
        s = trivial(pgo, g)
    elif kind == "huber":
        s = pgo.Solver(g, pgo.Options(method=0))    # the default Huber(0.01): K1's default instantiation until a plane is set
    else:
        s = pgo.Solver(g, pgo.Options(method=1))
    rng = np.random.default_rng(n)
    x = np.array(g.poses) + 0.05 * rng.standard_normal((n, 3))
    s.set_poses(x)
    w = random_weights(E, 11 + n)
    for apply_loss in (True, False):
        c0, r0, J0 = s.evaluate(apply_loss=apply_loss)
        e0 = s.edge_weights()
        s.set_edge_weights(w)
        assert np.array_equal(s.get_edge_weights(), w)
        c1, r1, J1 = s.evaluate(apply_loss=apply_loss)
        e1 = s.edge_weights()
        q = np.sqrt(w)[:, None]
        assert np.all(np.abs(r1 - q * r0) <= 1e-13 * np.abs(q * r0)), (kind, apply_loss)
        assert np.all(np.abs(J1 - q * J0) <= 1e-13 * np.abs(q * J0)), (kind, apply_loss)
        assert not r1[w == 0.0].any() and not J1[w == 0.0].any() and r0[w == 0.0].any(axis=1).all()
        ref = math.fsum(w * e0["cost"])
        assert abs(c1 - ref) <= 1e-13 * ref, (kind, apply_loss, c1, ref)
        # the scoring call with the plane: weight = w scale^2 rho1, cost = w 1/2 rho, and weight * s_plain = |r|^2
        assert e1["s_plain"].tobytes() == e0["s_plain"].tobytes() and e1["rho1"].tobytes() == e0["rho1"].tobytes()
        assert np.all(np.abs(e1["weight"] - w * e0["weight"]) <= 1e-15 * e0["weight"])
        assert np.all(np.abs(e1["cost"] - w * e0["cost"]) <= 1e-15 * e0["cost"])
        if apply_loss:
            r2 = (r1 * r1).sum(axis=1)
            assert np.all(np.abs(e1["weight"] * e1["s_plain"] - r2) <= 1e-12 * r2 + 1e-300)
        s.set_edge_weights(None)
        assert np.array_equal(s.get_edge_weights(), np.ones(E))
        c2, r2_, J2 = s.evaluate(apply_loss=apply_loss)
        assert c2 == c0 and r2_.tobytes() == r0.tobytes() and J2.tobytes() == J0.tobytes()
    s.close()


@pytest.mark.parametrize("kind", ["trivial", "huber", "dcs"])
def test_null_restores_the_handle_bitwise(pgo, kind):
    g = sub(pgo, 300)
    make = {"trivial": lambda: trivial(pgo, g, max_iters=6), "huber": lambda: pgo.Solver(g, pgo.Options(method=0, max_iters=6)),
            "dcs": lambda: pgo.Solver(g, pgo.Options(method=1, max_iters=6))}[kind]
    a, b = make(), make()
    b.set_edge_weights(random_weights(g.n_edges, 3))
    b.lm_begin()
    b.lm_step(2)
    b.set_edge_weights(None)
    b.set_poses(np.array(g.poses))
    sa, sb = a.solve(), b.solve()
    assert (sa.final_cost, sa.iterations, sa.termination) == (sb.final_cost, sb.iterations, sb.termination)
    assert history(a) == history(b) and a.poses().tobytes() == b.poses().tobytes()
    a.close(); b.close()


# ------------------------------------------------------------------ 2. binary weights = the mask
def test_binary_weights_against_the_mask(pgo):
    from test_gpu_covariance import BLOCK_REL, block_errors
    g = sub(pgo, 300)
    kind = np.array(g.kind)
    rng = np.random.default_rng(5)
    w = np.where((kind != 0) & (rng.random(g.n_edges) < 0.4), 0.0, 1.0)     # the odometry chain stays: every pose keeps an edge
    assert 50 < (w == 0.0).sum() < (kind != 0).sum()
    a, b = trivial(pgo, g, max_iters=10), trivial(pgo, g, max_iters=10)
    a.set_edge_weights(w)
    b.set_active(edge_active=w != 0.0)
    sa, sb = a.solve(), b.solve()
    assert (sa.iterations, sa.termination) == (sb.iterations, sb.termination)
    assert [r["step_ok"] for r in a.iter_records()] == [r["step_ok"] for r in b.iter_records()]
    xa, xb = a.poses(), b.poses()
    print("binary weights vs mask: max pose difference %.3e" % np.abs(xa - xb).max())
    assert np.abs(xa - xb).max() <= 1e-9
    idx = np.array([1, 77, 150, 222, 299])
    b.set_poses(xa)
    ca, _ = a.covariance(idx)
    cb, _ = b.covariance(idx)
    err = block_errors(ca, cb)
    print("covariance blocks, weights vs mask: relative errors", err)
    assert err.max() <= BLOCK_REL
    a.close(); b.close()


def test_zero_weight_odometry_edge_keeps_the_direct_solve(pgo):
    """weights never cut the chain: a zero-weight odometry edge is zero rows on a handle that stays on the direct solve (or
    redoes the iteration by PCG, direct_fallbacks), where the mask takes the handle to PCG; the two solves agree.  Tolerance:
    ten iterations of an exact linear solve against PCG at pcg_rtol 1e-12, on poses of up to ~20 m -- 1e-7 m."""
    g = sub(pgo, 300)
    ia, ib, kind = np.array(g.ia), np.array(g.ib), np.array(g.kind)
    e = int(np.nonzero((kind == 0) & (np.minimum(ia, ib) == 150))[0][0])
    w = np.ones(g.n_edges)
    w[e] = 0.0
    a = trivial(pgo, g, max_iters=10, pcg_rtol=1e-12, pcg_max_iters=400000)
    b = trivial(pgo, g, max_iters=10, pcg_rtol=1e-12, pcg_max_iters=400000)
    assert a.info().linear_solver == 2
    a.set_edge_weights(w)
    b.set_active(edge_active=w != 0.0)
    sa, sb = a.solve(), b.solve()
    assert a.info().linear_solver == 2 and b.info().linear_solver == 1
    assert sa.termination != 6 and [r["step_ok"] for r in a.iter_records()] == [r["step_ok"] for r in b.iter_records()]
    d = np.abs(a.poses() - b.poses()).max()
    print("zero-weight odometry edge: direct (fallbacks %d) against the masked PCG solve, max pose difference %.3e m" % (a.info().direct_fallbacks, d))
    assert d <= 1e-7
    a.close(); b.close()


# ------------------------------------------------------------------ 3. gnc_update against numpy
@pytest.fixture(scope="module")
def update_case(pgo):
    g = sub(pgo, 300)
    s = trivial(pgo, g, max_iters=3)
    s.solve()
    x = s.poses()
    s.close()
    return g, x


@pytest.mark.parametrize("ordering", [0, 1])
def test_gnc_update_against_numpy(pgo, update_case, ordering):
    g, x = update_case
    kind = np.array(g.kind)
    E = g.n_edges
    sel = kind != 0
    mu = 0.05
    s = trivial(pgo, g, pose_ordering=ordering)
    assert s.info().pose_ordering == ordering
    s.set_poses(x)
    sp = s.edge_weights()["s_plain"]
    ref_w = np.ones(E)
    ref_w[sel] = pgo.gnc_weight_eval(CBAR, mu, sp[sel])
    assert (ref_w == 1.0).sum() > sel.size - sel.sum() and ((ref_w > 0) & (ref_w < 1)).sum() > 5 and (ref_w == 0.0).sum() > 2
    seen = []
    try:
        for grid in (1, 2, -1):
            pgo.set_knob("gnc_grid", grid)
            for rep in range(2):
                s.set_edge_weights(None)
                st = s.gnc_update(CBAR, mu)
                w = s.get_edge_weights()
                assert w.tobytes() == ref_w.tobytes(), (grid, rep)
                assert st["n_selected"] == sel.sum() and st["n_nonfinite"] == 0
                assert st["n_nonbinary"] == ((w > 0) & (w < 1) & sel).sum() and st["n_zero"] == ((w == 0.0) & sel).sum()
                assert st["s_max"] == sp[sel].max()
                ref_sum = math.fsum(w[sel] * sp[sel])
                assert abs(st["weighted_sum"] - ref_sum) <= 1e-13 * ref_sum
                seen.append(tuple(st.items()))
    finally:
        pgo.set_knob("gnc_grid", -1)
    assert len(set(seen)) == 1                         # bitwise across grids and repeated calls
    # mu <= 0 measures only
    for m0 in (0.0, -1.0):
        st0 = s.gnc_update(CBAR, m0)
        assert s.get_edge_weights().tobytes() == ref_w.tobytes()
        assert st0 == dict(seen[0])                    # (the same weights at the same poses: the same numbers)
    s.set_edge_weights(None)
    st1 = s.gnc_update(CBAR, 0.0)                      # no plane: every weight reads as 1, and none is created
    assert st1["n_zero"] == 0 and st1["n_nonbinary"] == 0 and np.array_equal(s.get_edge_weights(), np.ones(E))
    assert abs(st1["weighted_sum"] - math.fsum(sp[sel])) <= 1e-13 * math.fsum(sp[sel])
    # select confines the update; by default odometry edges are never touched, nor are inactive edges
    half = np.full(E, 0.5)
    s.set_edge_weights(half)
    s.gnc_update(CBAR, mu)
    w = s.get_edge_weights()
    assert np.all(w[~sel] == 0.5) and w[sel].tobytes() == ref_w[sel].tobytes()
    pick = np.zeros(E, bool)
    pick[::3] = True
    assert (pick & ~sel).any() and (pick & sel).any()
    s.set_edge_weights(half)
    stp = s.gnc_update(CBAR, mu, select=pick)
    w = s.get_edge_weights()
    assert stp["n_selected"] == pick.sum() and np.all(w[~pick] == 0.5)
    assert w[pick].tobytes() == pgo.gnc_weight_eval(CBAR, mu, sp[pick]).tobytes()
    off = np.ones(E, bool)
    off[np.nonzero(sel)[0][:7]] = False
    s.set_active(edge_active=off)
    s.set_edge_weights(half)
    sta = s.gnc_update(CBAR, mu)
    w = s.get_edge_weights()
    assert sta["n_selected"] == sel.sum() - 7 and np.all(w[~off] == 0.5) and w[sel & off].tobytes() == ref_w[sel & off].tobytes()
    s.close()


def test_gnc_update_with_a_pose_that_is_not_finite(pgo, update_case):
    """an edge that cannot be evaluated is an outlier: weight 0, counted in n_nonfinite, and no part of s_max or the sum"""
    g, x = update_case
    sel = np.array(g.kind) != 0
    s = trivial(pgo, g)
    bad = int(np.array(g.ia)[np.nonzero(sel)[0][10]])
    xb = x.copy()
    xb[bad, 0] = np.nan
    s.set_poses(xb)
    hit = sel & ((np.array(g.ia) == bad) | (np.array(g.ib) == bad))
    st = s.gnc_update(CBAR, 0.05)
    w = s.get_edge_weights()
    assert hit.sum() >= 1 and st["n_nonfinite"] == hit.sum() and np.all(w[hit] == 0.0)
    s.set_poses(x)
    sp = s.edge_weights()["s_plain"]
    ok = sel & ~hit
    assert st["s_max"] == sp[ok].max() and w[ok].tobytes() == pgo.gnc_weight_eval(CBAR, 0.05, sp[ok]).tobytes()
    assert abs(st["weighted_sum"] - math.fsum(w[ok] * sp[ok])) <= 1e-13 * math.fsum(w[ok] * sp[ok])
    s.close()


# ------------------------------------------------------------------ 4. end to end
# Final poses against the restatement's: measured on an MI355X, max |x_gpu - x_restatement| = 4.038e-12 m over the 500 poses
# (the handle's linear solves against the restatement's sparse LU over 19 truncated solves and the final one).  The bound is
# 10 times that measurement; independently of it the deviation must stay below 1e-3 m, a fifth of the 0.0047 m that separates
# GNC from the clean solve.
POSE_BOUND = 10 * 4.038e-12


@pytest.fixture(scope="module")
def restated(oracle):
    og = GR.subgraph(oracle, 500)
    return og, GR.gnc(oracle, og, CBAR)


def test_gnc_solve_end_to_end(pgo, restated):
    og, ref = restated
    g = sub(pgo, 500)
    kind = np.array(g.kind)
    assert g.n_edges == 1455 and np.array_equal(kind, og.kind)
    s = trivial(pgo, g)
    summ, rounds = s.gnc_solve(CBAR)
    assert summ["rounds"] == len(rounds) == len(ref.rounds) == 19 and not summ["hit_max_rounds"]
    for a, b in zip(rounds, ref.rounds):
        assert abs(a["mu"] - b["mu"]) <= 1e-12 * b["mu"]
    w = s.get_edge_weights()
    assert np.array_equal(w, ref.weights)               # every one of the 1455 edges
    assert np.all(w[kind == 2] == 0.0) and np.all(w[kind != 2] == 1.0) and summ["n_zero"] == 35 and summ["n_selected"] == 956
    x = s.poses()
    dev = np.abs(x - ref.poses).max()
    print("gnc end to end: max pose deviation from the restatement %.3e m; rounds" % dev,
          [(r["n_nonbinary"], r["n_zero"], r["lm_iterations"], r["lm_termination"]) for r in rounds])
    assert dev < 1e-3
    assert dev <= POSE_BOUND
    # independently of the restatement: closer to the solve without the bogus edges than a default METHOD 1 solve
    clean = trivial(pgo, sub(pgo, 500, drop_bogus=True))
    clean.solve()
    xc = clean.poses()
    dcs = pgo.Solver(g, pgo.Options(method=1))
    dcs.solve()
    rm = lambda p: float(np.sqrt(((p[:, :2] - xc[:, :2]) ** 2).sum(axis=1).mean()))
    print("xy rmse against the clean solve: gnc %.4e m, METHOD 1 %.4e m" % (rm(x), rm(dcs.poses())))
    assert rm(x) < rm(dcs.poses())
    for h in (s, clean, dcs):
        h.close()


# ------------------------------------------------------------------ 5. errors and state
def _unchanged(pgo, s, make):
    """a solve of s is bitwise that of a fresh handle"""
    f = make()
    s.solve(), f.solve()
    assert history(s) == history(f) and s.poses().tobytes() == f.poses().tobytes()
    f.close()


def test_unsupported_handles(pgo, monkeypatch):
    g = sub(pgo, 66)
    E = g.n_edges
    gi = pgo.Graph.from_arrays(g.poses, g.ia, g.ib, g.meas, g.kind, info=np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (E, 1)))
    makers = [lambda: pgo.Solver(g, pgo.Options(method=2, max_iters=3)),
              lambda: pgo.Solver(gi, pgo.Options(method=0, info_weighting=1, max_iters=3))]
    for make in makers:
        s = make()
        for call in (lambda: s.set_edge_weights(np.full(E, 0.5)), lambda: s.get_edge_weights(), lambda: s.gnc_update(CBAR, 0.1),
                     lambda: s.gnc_solve(CBAR)):
            with pytest.raises(pgo.PgoError) as ei:
                call()
            assert ei.value.status == UNSUPPORTED
        _unchanged(pgo, s, make)
        s.close()
    monkeypatch.setenv("PGO_FORCE_COLLECTIVES", "1")
    u = pgo.Solver(g, pgo.Options(method=0))
    monkeypatch.delenv("PGO_FORCE_COLLECTIVES")
    for call in (lambda: u.set_edge_weights(np.full(E, 0.5)), lambda: u.gnc_update(CBAR, 0.1), lambda: u.gnc_solve(CBAR)):
        with pytest.raises(pgo.PgoError) as ei:
            call()
        assert ei.value.status == UNSUPPORTED
    u.close()


def test_invalid_arguments_change_nothing(pgo):
    g = sub(pgo, 66)
    E = g.n_edges
    make = lambda: trivial(pgo, g, max_iters=4)
    s = make()
    for bad in (np.nan, np.inf, -1e-9, 1.0 + 1e-9):
        w = np.full(E, 0.5)
        w[E // 2] = bad
        with pytest.raises(pgo.PgoError) as ei:
            s.set_edge_weights(w)
        assert ei.value.status == INVALID and "edge %d" % (E // 2) in str(ei.value)
    with pytest.raises(ValueError):
        s.set_edge_weights(np.ones(E + 1))
    for cbar, mu in ((0.0, 0.1), (-1.0, 0.1), (np.nan, 0.1), (np.inf, 0.1), (0.5, np.nan), (0.5, np.inf)):
        with pytest.raises(pgo.PgoError) as ei:
            s.gnc_update(cbar, mu)
        assert ei.value.status == INVALID
    for kw in (dict(cbar=0.0), dict(cbar=np.nan), dict(cbar=0.5, mu_factor=1.0), dict(cbar=0.5, mu_factor=np.nan),
               dict(cbar=0.5, inner_iters=0), dict(cbar=0.5, final_iters=0), dict(cbar=0.5, max_rounds=0)):
        with pytest.raises(pgo.PgoError) as ei:
            s.gnc_solve(**kw)
        assert ei.value.status == INVALID
    assert np.array_equal(s.get_edge_weights(), np.ones(E))
    _unchanged(pgo, s, make)
    s.close()
    # pgo_gnc_solve is METHOD 0's: a METHOD 1 handle keeps its weights and its solve
    make1 = lambda: pgo.Solver(g, pgo.Options(method=1, max_iters=4))
    m = make1()
    with pytest.raises(pgo.PgoError) as ei:
        m.gnc_solve(CBAR)
    assert ei.value.status == INVALID
    _unchanged(pgo, m, make1)
    m.close()


def test_state_rules(pgo):
    g = sub(pgo, 300)
    E = g.n_edges
    kind = np.array(g.kind)
    w = random_weights(E, 9)
    s = trivial(pgo, g)
    # a running solve is stale after the weights change, and only then
    s.lm_begin()
    s.lm_step(1)
    s.gnc_update(CBAR, 0.0)
    s.lm_step(1)
    for change in (lambda: s.set_edge_weights(w), lambda: s.gnc_update(CBAR, 0.05), lambda: s.set_edge_weights(None)):
        s.lm_begin()
        change()
        with pytest.raises(pgo.PgoError) as ei:
            s.lm_step(1)
        assert ei.value.status == INVALID
    # pgo_set_losses and pgo_set_active leave the weights alone, in either call order
    mask = np.ones(E, bool)
    mask[np.nonzero(kind != 0)[0][::5]] = False
    a, b = pgo.Solver(g, pgo.Options(method=0)), pgo.Solver(g, pgo.Options(method=0))
    a.set_edge_weights(w)
    a.set_losses(pgo.Loss("cauchy", 0.3))
    a.set_active(edge_active=mask)
    b.set_active(edge_active=mask)
    b.set_losses(pgo.Loss("cauchy", 0.3))
    b.set_edge_weights(w)
    assert np.array_equal(a.get_edge_weights(), w) and np.array_equal(b.get_edge_weights(), w)
    (ca, ra, Ja), (cb, rb, Jb) = a.evaluate(), b.evaluate()
    assert ca == cb and ra.tobytes() == rb.tobytes() and Ja.tobytes() == Jb.tobytes()
    assert not ra[~mask].any() and not ra[w == 0.0].any() and ra[mask & (w > 0.0)].any(axis=1).all()
    a.close(); b.close()
    # pgo_window_solve is refused while a plane is set
    win = pgo.window_plan(g.n_poses, g.ia, g.ib, g.kind, [int(np.nonzero(kind == 1)[0][3])], 4)
    s.set_edge_weights(None)
    p0, r0 = s.window_solve([win])
    s.set_edge_weights(w)
    with pytest.raises(pgo.PgoError) as ei:
        s.window_solve([win])
    assert ei.value.status == UNSUPPORTED
    s.set_edge_weights(None)
    p1, r1 = s.window_solve([win])
    assert p1[0].tobytes() == p0[0].tobytes()
    s.close()


def test_rounds_0_path(pgo):
    """the graph without its bogus edges, after a converged solve, with a generous cbar: nothing to graduate"""
    g = sub(pgo, 300, drop_bogus=True)
    s = trivial(pgo, g)
    assert s.solve().termination in (1, 2, 3)
    x = s.poses()
    summ, rounds = s.gnc_solve(5.0)
    assert summ["rounds"] == 0 and rounds == [] and summ["mu0"] == 0.0 and 2.0 * summ["rmax2"] <= 25.0
    assert summ["n_selected"] == (np.array(g.kind) != 0).sum() and summ["final_solve"]["termination"] in (1, 2, 3)
    assert np.array_equal(s.get_edge_weights(), np.ones(g.n_edges))
    assert np.abs(s.poses() - x).max() < 1e-6
    s.close()


# ------------------------------------------------------------------ 6. the C++ mirror and the CLI
def test_cli_gnc_is_the_librarys(pgo, tmp_path):
    """main DATASET 0 0 --loss trivial --gnc 0.5 (pgo::SolveGnc of host/pgo_problem.h) on the 300-pose sub-graph written as a
    g2o file: the rounds, weights.txt and the written-back poses are those of Solver.gnc_solve on the file's graph"""
    import subprocess
    from importlib import import_module
    exe = import_module("toy_robust_backend_slam_amd._build").build_cli()
    data, save = tmp_path / "data", tmp_path / "save"
    data.mkdir()
    sub(pgo, 300).write_g2o(str(data / "SUB300.g2o"))
    g = pgo.ReadG2O(str(data / "SUB300.g2o"))       # (the loader's own classes: odometry iff |a - b| < 5, everything else closure)
    kind = np.array(g.kind)
    assert g.n_edges == 717 and (kind != 0).sum() > 300
    p = subprocess.run([exe, "SUB300", "0", "0", "--loss", "trivial", "--gnc", str(CBAR), "--data", str(data), "--save", str(save),
                        "--precision", "17"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    s = trivial(pgo, g)
    summ, rounds = s.gnc_solve(CBAR, select=kind != 0)
    assert summ["rounds"] > 5 and "gnc: %d rounds, %d blocks at weight 0" % (summ["rounds"], summ["n_zero"]) in p.stdout
    assert p.stdout.count("gnc round ") == summ["rounds"]
    w = np.loadtxt(str(save / "weights.txt"))
    assert np.array_equal(w, s.get_edge_weights()) and (w == 0.0).sum() == summ["n_zero"] > 0
    nodes = np.loadtxt(str(save / "opt_nodes.txt"))
    assert np.array_equal(nodes[:, 1:4], s.poses())
    s.close()
    # --gnc is METHOD 0's
    assert subprocess.run([exe, "SUB300", "0", "1", "--gnc", "0.5", "--data", str(data), "--save", str(save)], capture_output=True).returncode != 0
