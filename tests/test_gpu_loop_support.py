"""pgo_loop_support on the device (include/pgo.h, "loop support"; csrc/loop_support.hip.h) against the host statement
pgo_loop_support_plan, which tests/test_loop_support_host.py pins to the numpy restatement: equality of the records, bitwise
reproducibility across calls, pose orderings and grids, what apply does to the handle and what its absence leaves alone, the
refusals, and the filter in front of a METHOD 0 solve.
(A batched handle is refused too, but the union handle of a pgo_batch is not reachable as a pgo_t through the C-ABI: that guard
has no test, as for pgo_coarsen and pgo_gnc_update.)"""
import numpy as np
import pytest

import _support_cases as SC

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -8


@pytest.fixture(scope="module")
def cases(pgo):
    """name -> (graph, arrays, select, host records, host stats, restatement info), computed once"""
    out = {}
    for n in SC.PLANTED_N:
        c = SC.planted(n)
        out["planted-%d" % n] = (SC.planted_graph(pgo, c), (c["n"], c["ia"], c["ib"], c["meas"], c["kind"]), c["select"])
    out["fixture-500"] = (SC.fixture_graph(pgo, 500), SC.fixture(500), None)
    for k, (g, arr, select) in list(out.items()):
        rec, stats = pgo.loop_support_plan(*arr, select=select)
        out[k] = (g, arr, select, rec, stats, SC.restate(*arr, select=select)[2])
    return out


def bits(rec, stats):
    return rec.tobytes(), tuple(sorted(stats.items()))


def history(s):
    return [{k: v for k, v in r.items() if k != "seconds"} for r in s.iter_records()]


NAMES = ["planted-%d" % n for n in SC.PLANTED_N] + ["fixture-500"]


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_statement(pgo, cases, name):
    g, arr, select, want, wstats, info = cases[name]
    s = pgo.Solver(g, pgo.Options(method=1))
    got, gstats = s.loop_support(select=select)
    SC.assert_same(got, want, info, name)
    assert gstats == wstats
    if name.startswith("planted"):   # other options, against the plan at the same options (margins from the restatement)
        for kw in (dict(window=1), dict(window=256, min_support=2), dict(tol_xy=0.05, tol_th=0.02)):
            full = dict(SC.DEFAULTS, **kw)
            got, gstats = s.loop_support(select=select, **full)
            want, wstats = pgo.loop_support_plan(*arr, select=select, **full)
            SC.assert_same(got, want, SC.restate(*arr, select=select, **full)[2], "%s %s" % (name, kw))
            assert gstats == wstats
        # another selection on the same handle, and back (the table is rebuilt per selection)
        got, gstats = s.loop_support()
        want, wstats = pgo.loop_support_plan(*arr)
        SC.assert_same(got, want, SC.restate(*arr)[2], name + " default selection")
        assert gstats == wstats
        got, gstats = s.loop_support(select=select)
        assert bits(got, gstats) == bits(*s.loop_support(select=select))
    s.close()


@pytest.mark.parametrize("name", ["planted-1000", "fixture-500", "planted-65"])
def test_bitwise_across_calls_orderings_and_grids(pgo, cases, name):
    g, arr, select, want, wstats, info = cases[name]
    seen = []
    try:
        for ordering in (0, 1):
            for grid in (1, 3, -1):
                pgo.set_knob("support_grid", grid)
                s = pgo.Solver(g, pgo.Options(method=1, pose_ordering=ordering))   # (T is computed at the handle's first call)
                for rep in range(2):
                    seen.append(bits(*s.loop_support(select=select)))
                s.close()
    finally:
        pgo.set_knob("support_grid", -1)
    assert len(seen) == 12 and len(set(seen)) == 1


@pytest.mark.parametrize("opts", [dict(method=1), dict(method=0), dict(method=2)], ids=["m1", "m0", "m2"])
def test_without_apply_the_handle_is_left_alone(pgo, cases, opts):
    g, arr, select, want, wstats, info = cases["fixture-500"]
    a, b = pgo.Solver(g, pgo.Options(max_iters=8, **opts)), pgo.Solver(g, pgo.Options(max_iters=8, **opts))
    for s in (a, b):
        s.lm_begin()
        s.lm_step(2)
    got, gstats = a.loop_support()
    SC.assert_same(got, want, info, "between lm_step slices")
    a.lm_step(3), b.lm_step(3)
    assert history(a) == history(b) and a.poses().tobytes() == b.poses().tobytes()
    if opts["method"] != 2:
        assert np.array_equal(a.get_edge_weights(), np.ones(g.n_edges))
    a.close(), b.close()


def test_apply_writes_the_weight_plane(pgo, cases):
    g, arr, select, want, wstats, info = cases["fixture-500"]
    E = g.n_edges
    kind = arr[4]
    vec = np.where((want["selected"] == 1) & (want["n_consistent"] < 1), 0.0, 1.0)
    assert (vec[kind == 2] == 0.0).all() and (vec == 0.0).sum() == 35 + 2
    make = lambda: pgo.Solver(g, pgo.Options(method=0, max_iters=10), losses=pgo.Loss("trivial"))
    a, b, f = make(), make(), make()
    got, gstats = a.loop_support(apply=True)
    SC.assert_same(got, want, info, "apply")
    assert np.array_equal(a.get_edge_weights(), vec)
    b.set_edge_weights(vec)
    a.solve(), b.solve()
    assert history(a) == history(b) and a.poses().tobytes() == b.poses().tobytes()
    # min_support 2: the verdict follows the option
    a.loop_support(apply=True, min_support=2)
    assert np.array_equal(a.get_edge_weights(), np.where((want["selected"] == 1) & (want["n_consistent"] < 2), 0.0, 1.0))
    # earlier weights of edges that are not selected are kept, those of the selected ones are overwritten
    w = np.random.default_rng(5).random(E)
    a.set_edge_weights(w)
    a.loop_support(apply=True)
    assert np.array_equal(a.get_edge_weights(), np.where(want["selected"] == 1, vec, w))
    sel = np.zeros(E, bool)
    sel[np.nonzero(kind == 2)[0][:10]] = True
    a.set_edge_weights(w)
    rec, st = a.loop_support(select=sel, apply=True)      # ten bogus loops among themselves: unsupported
    assert st["n_selected"] == 10 and st["n_supported"] == 0
    assert np.array_equal(a.get_edge_weights(), np.where(sel, 0.0, w))
    # NULL restores the handle
    a.set_edge_weights(None)
    a.set_poses(np.array(g.poses)), a.solve(), f.solve()
    assert history(a) == history(f) and a.poses().tobytes() == f.poses().tobytes()
    # a running solve is stale after apply, and only then
    a.set_poses(np.array(g.poses))
    a.lm_begin(), a.lm_step(1)
    a.loop_support()
    a.lm_step(1)
    a.loop_support(apply=True)
    with pytest.raises(pgo.PgoError) as ei:
        a.lm_step(1)
    assert ei.value.status == INVALID
    for s in (a, b, f):
        s.close()


def _unchanged(pgo, s, make):
    f = make()
    s.solve(), f.solve()
    assert history(s) == history(f) and s.poses().tobytes() == f.poses().tobytes()
    f.close()


def test_refusals_change_nothing(pgo, cases, monkeypatch):
    g, arr, select, want, wstats, info = cases["planted-65"]
    E = g.n_edges
    gi = pgo.Graph.from_arrays(g.poses, g.ia, g.ib, g.meas, g.kind, info=np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (E, 1)))
    for make in (lambda: pgo.Solver(g, pgo.Options(method=2, max_iters=3)), lambda: pgo.Solver(gi, pgo.Options(method=0, info_weighting=1, max_iters=3))):
        s = make()
        with pytest.raises(pgo.PgoError) as ei:
            s.loop_support(apply=True)
        assert ei.value.status == UNSUPPORTED
        got, gstats = s.loop_support()                    # fine without apply
        SC.assert_same(got, pgo.loop_support_plan(*arr)[0], SC.restate(*arr)[2], "no apply")
        _unchanged(pgo, s, make)
        s.close()
    make = lambda: pgo.Solver(g, pgo.Options(method=0, max_iters=3))
    s = make()
    for kw in (dict(window=0), dict(window=257), dict(tol_xy=0.0), dict(tol_xy=np.nan), dict(tol_th=-1.0), dict(tol_th=np.inf), dict(min_support=0)):
        for apply in (False, True):
            with pytest.raises(pgo.PgoError) as ei:
                s.loop_support(apply=apply, **kw)
            assert ei.value.status == INVALID, kw
    with pytest.raises(ValueError):
        s.loop_support(select=np.ones(E + 1))
    assert pgo.lib().pgo_loop_support(s._h, None, None, None, None) == INVALID
    assert pgo.lib().pgo_loop_support(None, None, None, None, None) == INVALID
    assert np.array_equal(s.get_edge_weights(), np.ones(E))
    _unchanged(pgo, s, make)
    s.close()
    # no outputs asked for: the call still runs (and applies)
    s = make()
    o = pgo.LoopSupportOptions(apply=1)
    assert pgo.lib().pgo_loop_support(s._h, o, None, None, None) == 0
    d = pgo.loop_support_plan(*arr)[0]
    assert np.array_equal(s.get_edge_weights(), np.where((d["selected"] == 1) & (d["n_consistent"] < 1), 0.0, 1.0))
    s.close()
    monkeypatch.setenv("PGO_FORCE_COLLECTIVES", "1")
    u = pgo.Solver(g, pgo.Options(method=0))
    monkeypatch.delenv("PGO_FORCE_COLLECTIVES")
    for apply in (False, True):
        with pytest.raises(pgo.PgoError) as ei:
            u.loop_support(apply=apply)
        assert ei.value.status == UNSUPPORTED
    u.close()


# METHOD 0 from dead reckoning after the filter against the same solve on a handle whose bogus and unsupported edges were
# removed with pgo_set_active: two routes to the same problem -- zero rows against absent rows -- that differ in the order of the
# sums over the edges at most.  Measured on an MI355X: E2E_MEASURED -- the two are bitwise equal, a zero-weight edge adds exact
# zeros to every sum it enters and this graph stays on one linear solver either way; the bound is ten times the measured value
# (DESIGN.md section 4i).
E2E_MEASURED = 0.0
E2E_BOUND = 10 * E2E_MEASURED


def test_filter_then_solve_end_to_end(pgo, cases):
    g, arr, select, want, wstats, info = cases["fixture-500"]
    kind = arr[4]
    drop = (kind == 2) | ((want["selected"] == 1) & (want["n_consistent"] < 1))
    make = lambda: pgo.Solver(g, pgo.Options(method=0), losses=pgo.Loss("trivial"))
    a, b = make(), make()
    rec, st = a.loop_support(apply=True)
    assert st["n_supported"] == 921 - 2 and np.array_equal(a.get_edge_weights() == 0.0, drop)
    b.set_active(edge_active=~drop)
    sa, sb = a.solve(), b.solve()
    assert sa.termination in (1, 2, 3) and sb.termination in (1, 2, 3)
    d = np.abs(a.poses() - b.poses()).max()
    ate = a.trajectory_error(pgo.synth_manhattan_truth(2000, 7)[:500])["ate_rmse"]
    print("filter + METHOD 0 against set_active: max pose difference %.3e (bound %.3e), iterations %d / %d, ATE %.3e"
          % (d, E2E_BOUND, sa.iterations, sb.iterations, ate))
    assert d <= E2E_BOUND, (d, E2E_BOUND)
    a.close(), b.close()


def test_cli_loop_support_is_the_librarys(pgo, tmp_path):
    """main DATASET 0 0 --loss trivial --loop-support 1 (pgo::LoopSupport of host/pgo_problem.h) on the 500-pose sub-graph
    written as a g2o file: the counts it prints, weights.txt and the written-back poses are those of Solver.loop_support with
    apply and Solver.solve on the file's graph; with --init-stride the coarse solve runs without the dropped blocks"""
    import subprocess
    from importlib import import_module
    exe = import_module("toy_robust_backend_slam_amd._build").build_cli()
    data, save = tmp_path / "data", tmp_path / "save"
    data.mkdir()
    SC.fixture_graph(pgo, 500).write_g2o(str(data / "SUB500.g2o"))
    g = pgo.ReadG2O(str(data / "SUB500.g2o"))       # (the loader's own classes: odometry iff |a - b| < 5, everything else closure)
    kind = np.array(g.kind)
    run = lambda *extra: subprocess.run([exe, "SUB500", "0", "0", "--loss", "trivial", "--data", str(data), "--save", str(save), "--precision", "17",
                                         *extra], capture_output=True, text=True, timeout=300)
    p = run("--loop-support", "1")
    assert p.returncode == 0, p.stdout + p.stderr
    s = pgo.Solver(g, pgo.Options(method=0), losses=pgo.Loss("trivial"))
    rec, st = s.loop_support(select=kind != 0, apply=True)
    assert st["n_selected"] > st["n_supported"] > 800
    assert "%d selected blocks, %d supported" % (st["n_selected"], st["n_supported"]) in p.stdout
    w = np.loadtxt(str(save / "weights.txt"))
    assert np.array_equal(w, s.get_edge_weights()) and (w == 0.0).sum() == st["n_selected"] - st["n_supported"]
    s.solve()
    assert np.array_equal(np.loadtxt(str(save / "opt_nodes.txt"))[:, 1:4], s.poses())
    # other options reach the library; with the hierarchical start the coarse graph loses the dropped blocks too
    p = run("--loop-support", "2:16:0.05:0.02", "--init-stride", "16")
    assert p.returncode == 0, p.stdout + p.stderr
    rec2, st2 = s.loop_support(select=kind != 0, window=16, tol_xy=0.05, tol_th=0.02, min_support=2, apply=True)
    assert "min 2 window 16 tol_xy 0.05 tol_th 0.02: %d selected blocks, %d supported" % (st2["n_selected"], st2["n_supported"]) in p.stdout
    s.set_poses(np.array(g.poses))
    s.initialize_hierarchical(16, carry_weights=True)
    s.solve()
    assert np.array_equal(np.loadtxt(str(save / "opt_nodes.txt"))[:, 1:4], s.poses())
    s.close()
    # METHOD 2 has no weight plane
    assert subprocess.run([exe, "SUB500", "0", "2", "--loop-support", "1", "--data", str(data), "--save", str(save)], capture_output=True).returncode != 0
