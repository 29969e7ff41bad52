"""pgo_chordal_init on the device (include/pgo.h, "chordal initialisation"; csrc/chordal.hip.h) against the host statement
pgo_chordal_plan, which tests/test_chordal_host.py pins to the numpy / scipy restatement: the same iteration counts and results
that differ by rounding alone (_chordal_cases.rounding_bounds), besides agreement within what two solves to rtol imply
(_chordal_cases.bounds; both derived from the restatement's eigenvalues and printed beside the measured difference), the truth
of noise-free graphs to 1e-9 m,
bitwise reproducibility across calls, pose orderings and grids, what commit and apply_weights do to the handle and what their
absence leaves alone, the refusals, and the start in front of a METHOD 1 solve.
(A batched handle is refused too, but the union handle of a pgo_batch is not reachable as a pgo_t through the C-ABI: that guard
has no test, as for pgo_loop_support.)"""
import numpy as np
import pytest

import _chordal_cases as CC
from _coarsen_cases import wrap

pytestmark = pytest.mark.gpu

INVALID, NUMERIC, UNSUPPORTED = -1, -7, -8
RTOL = 1e-8

MAKE = {"planted-65-two": lambda: CC.planted_case(65, "two"), "planted-257-weights": lambda: CC.planted_case(257, "weights"),
        "planted-513-const": lambda: CC.planted_case(513, "const"), "planted-1000-plain": lambda: CC.planted_case(1000),
        "planted-1000-weights": lambda: CC.planted_case(1000, "weights"), "fixture-2000": lambda: CC.fixture_case()}


@pytest.fixture(scope="module")
def cases(pgo):
    """name -> (case, graph, plan result, restatement info), computed once"""
    out = {}
    for k, make in MAKE.items():
        c = make()
        out[k] = (c, CC.graph_of(pgo, c), pgo.chordal_plan(*CC.plan_args(c), w=c["w"], constant=c["constant"]),
                  CC.restate(*CC.plan_args(c), w=c["w"], constant=c["constant"])[3])
    return out


def solver(pgo, c, g, **opts):
    """a handle that holds the case: its weights in the plane (zero-weight edges of the `weights` variant inactive instead, so
    that the mask is exercised), its constant poses through fixed_pose or pose_constant"""
    const = c["constant"]
    fixed = 0
    if const is not None:
        idx = np.nonzero(const)[0]
        fixed = int(idx[0]) if len(idx) == 1 else -1
    s = pgo.Solver(g, pgo.Options(method=opts.pop("method", 1), fixed_pose=fixed, **opts))
    w = c["w"].copy()
    inactive = None
    if (w > 0).any() and ((w > 0) & (w < 1)).any():      # the fractional plane: its zeros go through the mask
        inactive = w == 0.0
        w[inactive] = 0.5
    if inactive is not None or (const is not None and fixed < 0):
        s.set_active(edge_active=None if inactive is None else ~inactive, pose_constant=const if fixed < 0 else None)
    if not (w == 1.0).all():
        s.set_edge_weights(w)
    return s


def history(s):
    return [{k: v for k, v in r.items() if k != "seconds"} for r in s.iter_records()]


def bits(out):
    poses, res, summ = out
    return poses.tobytes(), res.tobytes(), str({k: v for k, v in summ.items() if k != "seconds"})


@pytest.mark.parametrize("name", sorted(MAKE))
def test_device_equals_the_plan(pgo, cases, name):
    c, g, (want, wres, _, wsumm), info = cases[name]
    s = solver(pgo, c, g)
    got, res, summ = s.chordal_init()
    a, b = summ["solves"][0], wsumm["solves"][0]
    print("%s: iterations %s (plan %s), relative residuals %s" % (name, a["iters"], b["iters"], a["rel_residual"]))
    assert a["converged"] == [1, 1] and max(a["rel_residual"]) <= RTOL
    assert a["iters"] == b["iters"]                       # one recurrence: the same number of iterations in both stages ...
    CC.compare_rounding(got, want, info, c, name)         # ... and results that differ by rounding alone
    CC.compare(got, want, info, RTOL, name, solves=2)
    const = np.arange(c["n"]) == 0 if c["constant"] is None else np.asarray(c["constant"], bool)
    assert got[const].tobytes() == np.ascontiguousarray(c["poses"][const]).tobytes()
    assert summ["n_degenerate"] == 0 and abs(summ["min_mag"] - wsumm["min_mag"]) <= CC.bounds(info, RTOL, 2)[0]
    b_th, b_xy = CC.bounds(info, RTOL, 2)
    lever = np.hypot(c["meas"][:, 0], c["meas"][:, 1]).max()
    assert np.abs(res[:, 0] - wres[:, 0]).max() <= 2 * b_xy + lever * 2 * b_th and np.abs(res[:, 1] - wres[:, 1]).max() <= 2 * b_th
    # the report is the definition at the device's own poses (zh = exp(i theta): nothing is degenerate); 1e-12: the rounding of
    # a difference of positions of up to some hundred metres
    t, th, m = got[:, 0] + 1j * got[:, 1], got[:, 2], c["meas"]
    ia, ib = c["ia"], c["ib"]
    assert np.abs(res[:, 0] - np.abs(t[ib] - t[ia] - np.exp(1j * th[ia]) * (m[:, 0] + 1j * m[:, 1]))).max() <= 1e-12 * max(1.0, np.abs(t).max())
    assert np.abs(res[:, 1] - np.abs(wrap(th[ib] - th[ia] - m[:, 2]))).max() <= 1e-12
    # the handle is as it was: its poses are the graph's
    assert s.poses().tobytes() == np.ascontiguousarray(c["poses"]).tobytes()
    s.close()


@pytest.mark.parametrize("n,variant", [(65, "two"), (257, "weights"), (513, "const"), (1000, "plain"), (1000, "weights")])
def test_device_returns_the_truth_of_a_noise_free_graph(pgo, n, variant):
    """_chordal_cases.exact_case: every positive-weight measurement comes from the true poses, the start (a noisy chain at
    weight 0) does not.  The truth comes back to 1e-9 m and 1e-9 rad -- the bound test_chordal_host sets for the plan -- once
    rtol asks for it (1e-14; the restatement's direct solve is 2e-12 to 2e-11 m from the truth on these graphs).  This pins the
    device's positions at every size: a wavefront and a row, two tiles and a row, four, and a tail of 232 rows."""
    c = CC.exact_case(n, variant)
    const = c["constant"]
    fixed = 0 if const is None else (int(np.nonzero(const)[0][0]) if const.sum() == 1 else -1)
    s = pgo.Solver(CC.graph_of(pgo, c), pgo.Options(method=0, fixed_pose=fixed))
    if fixed < 0:
        s.set_active(edge_active=None, pose_constant=const)
    s.set_edge_weights(c["w"])
    start = s.chordal_init(max_iters=1)[0]
    got, res, summ = s.chordal_init(rtol=1e-14)
    d_xy, d_th = CC.from_truth(got, c)
    a = summ["solves"][0]
    print("noise-free %d-%s: %.3e m, %.3e rad from the truth after %s iterations, relative residuals %s (one iteration from the start: %.3e m)"
          % (n, variant, d_xy, d_th, a["iters"], a["rel_residual"], CC.from_truth(start, c)[0]))
    assert CC.from_truth(start, c)[0] > 1e-3               # the start is not the answer
    assert a["converged"] == [1, 1] and min(a["iters"]) > 0
    assert d_xy <= 1e-9 and d_th <= 1e-9
    assert res[c["w"] > 0].max() <= 1e-9
    s.close()


@pytest.mark.parametrize("name", ["planted-1000-weights", "planted-65-two", "fixture-2000"])
def test_bitwise_across_calls_orderings_and_grids(pgo, cases, name):
    c, g, _, _ = cases[name]
    seen = []
    try:
        for ordering in (0, 1):
            for grid in (1, 3, -1):
                pgo.set_knob("chordal_grid", grid)
                s = solver(pgo, c, g, pose_ordering=ordering)
                for rep in range(2 if grid == 3 else 1):
                    seen.append(bits(s.chordal_init(check_every=7 if grid == 1 else 50)))   # (the slice length plays no part either)
                s.close()
    finally:
        pgo.set_knob("chordal_grid", -1)
    assert len(seen) == 8 and len(set(seen)) == 1


def test_degenerate_and_reject_rounds_follow_the_plan(pgo):
    c = CC.degenerate_case(65)
    g = CC.graph_of(pgo, c)
    s = solver(pgo, c, g)
    want, _, _, wsumm = pgo.chordal_plan(*CC.plan_args(c), w=c["w"])
    got, _, summ = s.chordal_init()
    h = c["half"]
    assert summ["n_degenerate"] == wsumm["n_degenerate"] == c["n"] - h and summ["min_mag"] < 1e-3
    assert np.abs(got[h:, 2] - want[h:, 2]).max() <= 1e-12 and np.abs(wrap(got[:h, 2] - want[:h, 2])).max() <= 1e-6
    s.close()
    c = CC.reject_case(257)
    g = CC.graph_of(pgo, c)
    want, wres, w_out, wsumm = pgo.chordal_plan(*CC.plan_args(c), w=c["w"], rounds=3)
    info = CC.restate(*CC.plan_args(c), w=c["w"], rounds=3)[3]
    s = solver(pgo, c, g, method=0)
    got, res, summ = s.chordal_init(rounds=3)
    assert summ["n_solves"] == 2 and [x["n_rejected"] for x in summ["solves"]] == [len(c["bad"]), 0]
    assert [x["iters"] for x in summ["solves"]] == [x["iters"] for x in wsumm["solves"]]
    CC.compare_rounding(got, want, info, c, "reject-257")
    CC.compare(got, want, info, RTOL, "reject-257", solves=2)
    assert np.array_equal(s.get_edge_weights(), c["w"])                   # without apply_weights the plane is as it was
    # apply_weights round-trips through pgo_get_edge_weights: 0 on the rejected edges, every other weight kept
    got2, _, summ2 = s.chordal_init(rounds=3, apply_weights=True)
    assert got2.tobytes() == got.tobytes() and np.array_equal(s.get_edge_weights(), w_out)
    assert np.array_equal(np.nonzero(s.get_edge_weights() == 0.0)[0], c["bad"])
    again = s.chordal_init(rounds=3)[2]                                    # the plane now holds the verdict: nothing left to reject
    assert again["n_solves"] == 1 and again["n_rejected"] == 0
    s.close()
    # a fresh plane is created at all ones
    t = pgo.Solver(g, pgo.Options(method=0))
    t.set_edge_weights(c["w"])
    t.set_edge_weights(None)
    ones = np.ones(len(c["w"]))
    summ3 = t.chordal_init(rounds=1, apply_weights=True, reject_xy=30.0, reject_th=3.0)[2]
    dropped = t.get_edge_weights() == 0.0
    assert summ3["n_rejected"] == dropped.sum() > 0 and np.array_equal(t.get_edge_weights(), np.where(dropped, 0.0, ones))
    t.close()


@pytest.mark.parametrize("method", [0, 1, 2])
def test_without_commit_the_handle_is_left_alone(pgo, cases, method):
    c, g, _, _ = cases["fixture-2000"]
    sub = CC.fixture_case(500)
    g = CC.graph_of(pgo, sub)
    a, b = pgo.Solver(g, pgo.Options(method=method, max_iters=8)), pgo.Solver(g, pgo.Options(method=method, max_iters=8))
    for s in (a, b):
        s.lm_begin()
        s.lm_step(2)
    a.chordal_init(rounds=1)
    a.lm_step(3), b.lm_step(3)
    assert history(a) == history(b) and a.poses().tobytes() == b.poses().tobytes()
    if method != 2:
        assert np.array_equal(a.get_edge_weights(), np.ones(g.n_edges))
    a.close(), b.close()


def test_commit_writes_the_poses_and_keeps_the_constant_ones(pgo, cases):
    for name in ("planted-65-two", "planted-513-const"):
        c, g, _, _ = cases[name]
        for ordering in (0, 1):
            s = solver(pgo, c, g, pose_ordering=ordering, max_iters=5)
            before = s.poses()
            s.lm_begin(), s.lm_step(1)
            moved = s.poses()
            got, _, _ = s.chordal_init(commit=True)
            const = np.asarray(c["constant"], bool)
            now = s.poses()
            assert now[const].tobytes() == moved[const].tobytes() == before[const].tobytes()   # bitwise as they were
            assert now.tobytes() == got.tobytes()
            with pytest.raises(pgo.PgoError) as ei:                                              # the running solve is stale
                s.lm_step(1)
            assert ei.value.status == INVALID
            s.lm_begin(), s.lm_step(1)
            s.close()


def test_refusals_and_errors_change_nothing(pgo, cases, monkeypatch):
    c, g, _, _ = cases["planted-65-two"]
    plain = CC.planted_case(65)
    gp = CC.graph_of(pgo, plain)
    s = pgo.Solver(gp, pgo.Options(method=2, max_iters=3))
    with pytest.raises(pgo.PgoError) as ei:
        s.chordal_init(apply_weights=True)
    assert ei.value.status == UNSUPPORTED
    assert np.isfinite(s.chordal_init()[0]).all()                # fine without apply_weights
    s.close()
    s = pgo.Solver(gp, pgo.Options(method=0, max_iters=3))
    for kw in (dict(rtol=0.0), dict(max_iters=0), dict(check_every=0), dict(mag_min=-1.0), dict(rounds=9), dict(reject_xy=0.0)):
        with pytest.raises(pgo.PgoError) as ei:
            s.chordal_init(commit=True, apply_weights=True, **kw)
        assert ei.value.status == INVALID, kw
    assert pgo.lib().pgo_chordal_init(s._h, None, None, None, None) == INVALID
    assert pgo.lib().pgo_chordal_init(None, None, None, None, None) == INVALID
    o = pgo.ChordalOptions()
    assert pgo.lib().pgo_chordal_init(s._h, o, None, None, None) == 0     # no outputs asked for: the call still runs
    # a component the mask cuts off from the constant pose, named; nothing changes
    h = 32
    ia, ib = plain["ia"], plain["ib"]
    cut = (np.minimum(ia, ib) < h) & (np.maximum(ia, ib) >= h)
    s.set_edge_weights(np.where(cut, 0.0, 1.0))
    with pytest.raises(pgo.PgoError) as ei:
        s.chordal_init(commit=True, apply_weights=True)
    assert ei.value.status == UNSUPPORTED and "pose %d " % h in str(ei.value)
    assert s.poses().tobytes() == np.ascontiguousarray(plain["poses"]).tobytes()
    assert np.array_equal(s.get_edge_weights(), np.where(cut, 0.0, 1.0))
    s.close()
    s = pgo.Solver(gp, pgo.Options(method=0, fixed_pose=-1))     # no constant pose at all
    with pytest.raises(pgo.PgoError) as ei:
        s.chordal_init()
    assert ei.value.status == UNSUPPORTED
    s.close()
    # a measurement that is not finite on a positive-weight edge: named; at weight 0 it is not looked at
    m = plain["meas"].copy()
    fam = int(plain["planted"]["families"][2])
    m[fam, 1] = np.nan
    gn = pgo.Graph.from_arrays(plain["poses"], ia, ib, m, plain["kind"])
    s = pgo.Solver(gn, pgo.Options(method=0))
    with pytest.raises(pgo.PgoError) as ei:
        s.chordal_init()
    assert ei.value.status == NUMERIC and "edge %d " % fam in str(ei.value)
    w = np.ones(len(ia))
    w[fam] = 0.0
    s.set_edge_weights(w)
    assert np.isfinite(s.chordal_init()[0]).all()
    s.close()
    monkeypatch.setenv("PGO_FORCE_COLLECTIVES", "1")
    u = pgo.Solver(gp, pgo.Options(method=0))
    monkeypatch.delenv("PGO_FORCE_COLLECTIVES")
    with pytest.raises(pgo.PgoError) as ei:
        u.chordal_init()
    assert ei.value.status == UNSUPPORTED
    u.close()


def test_filter_chordal_start_then_method_1(pgo, cases):
    """On the 2000-pose fixture: loop_support(apply) -> chordal_init(commit) -> METHOD 1 against the path of DESIGN.md section
    4i, loop_support(apply) -> initialize_hierarchical(16, carry_weights) -> METHOD 1 (0.055 m on that section's graph), both
    run here.  Both are LM solves of one problem from two starts; how far two such routes may end from each other is taken from
    a third, the restatement's own run -- the same METHOD 1 solve started from the poses the direct solves of
    _chordal_cases.restate give for the filtered weights: margin = |ATE(restatement's start) - ATE(hierarchical start)|, and the
    chordal path must end no worse than the hierarchical one by more than that."""
    c, g, _, _ = cases["fixture-2000"]
    truth = pgo.synth_manhattan_truth(2000, 7)
    ate = lambda s: s.trajectory_error(truth)["ate_rmse"]
    make = lambda: pgo.Solver(g, pgo.Options(method=1))
    hier, chord, ref = make(), make(), make()
    for s in (hier, chord, ref):
        s.loop_support(apply=True)
    w = chord.get_edge_weights()
    hier.initialize_hierarchical(16, carry_weights=True)
    a_hier0 = ate(hier)
    hier.solve()
    start, _, summ = chord.chordal_init(commit=True)
    a_chord0 = ate(chord)
    sc = chord.solve()
    ref.set_poses(CC.restate(*CC.plan_args(c), w=w)[0])
    a_ref0 = ate(ref)
    ref.solve()
    a_hier, a_chord, a_ref = ate(hier), ate(chord), ate(ref)
    margin = abs(a_ref - a_hier)
    print("fixture: dead reckoning %.3f m; hierarchical start %.4f -> %.4f m; chordal start %.4f -> %.4f m (%s iterations of the stages, min |z| %.3f, "
          "%d LM iterations); restatement's start %.4f -> %.4f m; margin %.3e m"
          % (pgo.trajectory_error(c["poses"], truth)["ate_rmse"], a_hier0, a_hier, a_chord0, a_chord, summ["solves"][0]["iters"], summ["min_mag"],
             sc.iterations, a_ref0, a_ref, margin))
    assert sc.termination in (1, 2, 3)
    assert a_chord <= a_hier + margin, (a_chord, a_hier, margin)
    for s in (hier, chord, ref):
        s.close()


def test_cli_chordal_init_is_the_librarys(pgo, tmp_path):
    """main DATASET 0 1 --loop-support 1 --chordal-init [ROUNDS...] (pgo::ChordalInit of host/pgo_problem.h) on the 500-pose
    sub-graph written as a g2o file: the line it prints and the written-back poses are those of Solver.loop_support with apply,
    Solver.chordal_init with commit and Solver.solve on the file's graph"""
    import subprocess
    from importlib import import_module
    import _support_cases as SC
    exe = import_module("toy_robust_backend_slam_amd._build").build_cli()
    data, save = tmp_path / "data", tmp_path / "save"
    data.mkdir()
    SC.fixture_graph(pgo, 500).write_g2o(str(data / "SUB500.g2o"))
    g = pgo.ReadG2O(str(data / "SUB500.g2o"))
    kind = np.array(g.kind)
    run = lambda *extra: subprocess.run([exe, "SUB500", "0", "1", "--data", str(data), "--save", str(save), "--precision", "17", *extra],
                                        capture_output=True, text=True, timeout=300)
    for extra, kw in ((("--chordal-init",), {}), (("--chordal-init", "2:1.5:0.3"), dict(rounds=2, reject_xy=1.5, reject_th=0.3, apply_weights=True))):
        p = run("--loop-support", "1", *extra)
        assert p.returncode == 0, p.stdout + p.stderr
        s = pgo.Solver(g, pgo.Options(method=1))
        s.loop_support(select=kind != 0, apply=True)
        _, _, summ = s.chordal_init(commit=True, **kw)
        last = summ["solves"][-1]
        assert "%d solves, %d blocks rejected, %d + %d iterations" % (summ["n_solves"], summ["n_rejected"], last["iters"][0], last["iters"][1]) in p.stdout
        s.solve()
        assert np.array_equal(np.loadtxt(str(save / "opt_nodes.txt"))[:, 1:4], s.poses())
        s.close()
    assert run("--chordal-init", "9").returncode != 0          # more rounds than PGO_CHORDAL_MAX_ROUNDS
