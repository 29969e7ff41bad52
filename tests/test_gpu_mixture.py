"""Max-mixture edges (pgo_set_mixtures, pgo_mixture_select, pgo_mixture_solve) on the GPU.

Inputs: the 500-pose sub-graph of tests/golden/synth_manhattan_2000_s7.npz (smaller ones where a test says so).  Unless a test
says otherwise the handle is METHOD 0 with the Trivial loss (set_losses).  The select is compared with pgo_mixture_plan (the
serial host statement, pinned to numpy by tests/test_mixture_host.py), the loop with the numpy restatement of
tests/_mixture_cases.py on the planted world."""
import os

import numpy as np
import pytest

import _gnc_restatement as GR
import _mixture_cases as MC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -8, -1
# Final poses against the restatement's: the bound of tests/test_gpu_gnc.py's end-to-end test, which runs the same restated LM
# machinery against the same handle (10 times the 4.038e-12 m measured there)
POSE_BOUND = 10 * 4.038e-12


def sub(pgo, n):
    z = np.load(os.path.join(GOLDEN, "synth_manhattan_2000_s7.npz"))
    keep = (z["ia"] < n) & (z["ib"] < n)
    return pgo.Graph.from_arrays(z["poses"][:n], z["ia"][keep], z["ib"][keep], z["meas"][keep], z["kind"][keep])


def trivial(pgo, g, **opt):
    opt.setdefault("method", 0)
    return pgo.Solver(g, pgo.Options(**opt), losses=pgo.Loss("trivial"))


def history(s):
    return [{k: v for k, v in r.items() if k != "seconds"} for r in s.iter_records()]


def cost(s):
    return s.evaluate(want_r=False, want_J=False)[0]


@pytest.fixture(scope="module")
def og(oracle):
    return GR.subgraph(oracle, 500)


@pytest.fixture(scope="module")
def g500(pgo):
    return sub(pgo, 500)


def same(a, b):
    """two select results, bitwise: chosen, q, stats"""
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ------------------------------------------------------------------ 1. the select against the plan
@pytest.mark.parametrize("n", MC.SELECT_SIZES)
def test_select_against_the_plan(pgo, og, g500, n):
    (edge, ptr, comps), x = MC.select_case(og, n)
    K = np.diff(ptr)
    pc, pq, ps = pgo.mixture_plan(x, og.ia, og.ib, edge, ptr, comps)
    ok = MC.decided(pq)
    assert ps["n_nonfinite"] == 0 and (~ok).sum() <= 0.01 * n
    if n >= 255:
        assert all(c > 0 for c in ps["count"])      # every component index is chosen somewhere
    win = pgo.window_plan(g500.n_poses, g500.ia, g500.ib, g500.kind, [int(edge[0])], 4)
    results = []
    try:
        for po in (0, 1):
            for grid in (1, -1):
                pgo.set_knob("mix_grid", grid)
                s = trivial(pgo, g500, pose_ordering=po)
                s.set_poses(x)
                s.set_mixtures(edge, ptr, comps)
                c0 = cost(s)
                a, b = s.mixture_select(), s.mixture_select()
                assert same(a, b)
                # apply = 0 wrote nothing and made no plane: the cost is bitwise, the window solve (refused under a plane) runs
                assert cost(s) == c0 and np.all(s.mixture_selection() == -1)
                s.window_solve([win])
                assert np.array_equal(s.get_edge_weights(), np.ones(g500.n_edges))
                chosen, q, st = a
                assert np.array_equal(chosen[ok], pc[ok])
                assert np.all(np.abs(q[:, 0] - pq[:, 0]) <= MC.Q_REL * np.abs(pq[:, 0]))
                fin = np.isfinite(pq[:, 1])
                assert np.array_equal(np.isinf(q[:, 1]), ~fin) and np.all(q[~fin, 1] > 0) and np.array_equal(~fin, K == 1)
                # (the margin is q_second - q_best: each q is good to Q_REL of itself, so their difference to Q_REL (q_best + q_second))
                assert np.all(np.abs(q[fin, 1] - pq[fin, 1]) <= MC.Q_REL * (2.0 * np.abs(pq[fin, 0]) + pq[fin, 1]))
                assert (st["n_mix"], st["n_changed"], st["n_nonfinite"], st["n_inactive"]) == (n, n, 0, 0)
                assert st["count"] == np.bincount(chosen, minlength=8).tolist()      # exact, whatever the undecided edges did
                if ok.all():   # (an undecided edge may sit on another component: its c_k* and its count then differ by right)
                    assert st["count"] == ps["count"]
                    assert abs(st["offset"] - ps["offset"]) <= 1e-12 * abs(ps["offset"])
                assert abs(st["mix_cost"] - ps["mix_cost"]) <= 1e-12 * abs(ps["mix_cost"])
                # apply: the same selection, now in the planes
                ap = s.mixture_select(apply=True)
                assert same(ap, a) and np.array_equal(s.mixture_selection(), chosen)
                rows = comps[ptr[:-1] + chosen]
                w = s.get_edge_weights()
                ref_w = np.ones(g500.n_edges)
                ref_w[edge] = rows[:, 4]
                assert np.array_equal(w, ref_w)                                      # w_k*, and 1 everywhere else
                one = rows.copy()
                one[:, 3:] = 1.0                                                     # (pi = w = 1: q = 1/2 s exactly)
                _, q1, _ = pgo.mixture_plan(x, og.ia, og.ib, edge, np.arange(n + 1, dtype=np.int32), one)
                sp = s.edge_weights()["s_plain"][edge]
                assert np.all(np.abs(sp - 2.0 * q1[:, 0]) <= MC.Q_REL * 2.0 * q1[:, 0])      # s_plain is s_k*
                with pytest.raises(pgo.PgoError) as ei:
                    s.window_solve([win])
                assert ei.value.status == UNSUPPORTED
                again = s.mixture_select(apply=True)
                assert again[2]["n_changed"] == 0 and np.array_equal(again[0], chosen) and again[1].tobytes() == q.tobytes()
                results.append(a)
                s.close()
    finally:
        pgo.set_knob("mix_grid", -1)
    for r in results[1:]:
        assert same(r, results[0])          # both orderings and both grids: bitwise


# ------------------------------------------------------------------ 2. edges that cannot be evaluated
def test_nonfinite_pose(pgo, og, g500):
    """one NaN pose: its mixture edges are counted, keep their selection and their planes; the others are unaffected"""
    (edge, ptr, comps), x = MC.select_case(og, 257)
    bad_pose = int(og.ib[edge[100]])
    touched = (og.ia[edge] == bad_pose) | (og.ib[edge] == bad_pose)
    assert 0 < touched.sum() < 20
    s = trivial(pgo, g500)
    s.set_mixtures(edge, ptr, comps)
    first = s.mixture_select(apply=True)          # at the file's poses
    w0, sp0 = s.get_edge_weights(), s.edge_weights()["s_plain"]
    xn = x.copy()
    xn[bad_pose] = np.nan
    s.set_poses(xn)
    chosen, q, st = s.mixture_select(apply=True)
    assert st["n_nonfinite"] == int(touched.sum()) and st["n_inactive"] == 0
    assert np.array_equal(chosen[touched], first[0][touched]) and np.all(np.isnan(q[touched]))
    # the others: what a handle at the finite poses x selects
    t = trivial(pgo, g500)
    t.set_poses(x)
    t.set_mixtures(edge, ptr, comps)
    ref = t.mixture_select(apply=True)
    assert np.array_equal(chosen[~touched], ref[0][~touched]) and q[~touched].tobytes() == ref[1][~touched].tobytes()
    assert sum(st["count"]) == int((~touched).sum())
    # the planes of the touched edges: as the first select left them
    w1 = s.get_edge_weights()
    assert np.array_equal(w1[edge[touched]], w0[edge[touched]]) and np.array_equal(w1[edge[~touched]], t.get_edge_weights()[edge[~touched]])
    s.set_poses(np.array(g500.poses))
    sp1 = s.edge_weights()["s_plain"]
    assert np.array_equal(sp1[edge[touched]], sp0[edge[touched]])
    # every component non-finite on every edge of a pose: nothing is selected there on a fresh table either
    t.set_mixtures(edge, ptr, comps)
    t.set_poses(xn)
    c2, _, st2 = t.mixture_select(apply=True)
    assert np.all(c2[touched] == -1) and st2["n_changed"] == int((~touched).sum())
    s.close(); t.close()


def test_inactive_edges(pgo, og, g500):
    (edge, ptr, comps), x = MC.select_case(og, 257)
    mask = np.ones(g500.n_edges, bool)
    off = np.zeros(len(edge), bool)
    off[::7] = True
    mask[edge[off]] = False
    s = trivial(pgo, g500)
    s.set_poses(x)
    s.set_mixtures(edge, ptr, comps)
    s.set_active(edge_active=mask)                # (leaves the table alone)
    chosen, q, st = s.mixture_select(apply=True)
    assert st["n_inactive"] == int(off.sum()) and st["n_changed"] == int((~off).sum()) and st["n_nonfinite"] == 0
    assert np.all(chosen[off] == -1) and np.all(np.isnan(q[off])) and np.all(chosen[~off] >= 0)
    assert np.all(s.get_edge_weights()[edge[off]] == 1.0)
    t = trivial(pgo, g500)
    t.set_poses(x)
    t.set_mixtures(edge, ptr, comps)
    ref = t.mixture_select(apply=True)
    assert np.array_equal(chosen[~off], ref[0][~off]) and q[~off].tobytes() == ref[1][~off].tobytes()
    # their measurements too: active again, they evaluate as a handle that never had mixtures does
    s.set_active()
    u = trivial(pgo, g500)
    u.set_poses(x)
    assert np.array_equal(s.edge_weights()["s_plain"][edge[off]], u.edge_weights()["s_plain"][edge[off]])
    for h in (s, t, u):
        h.close()


# ------------------------------------------------------------------ 3. clearing restores the handle
@pytest.mark.parametrize("n_poses,linear_solver", [(300, 2), (500, 1)])
def test_clear_restores_the_handle(pgo, oracle, n_poses, linear_solver):
    """set, select + apply, solve, clear, drop the plane: pgo_solve is bitwise a fresh handle's -- on a direct-solve handle (the
    300-pose sub-graph, linear_solver 2: the chain factorisation and the capacitance matrix are formed from what K1 gives
    them) and on a PCG handle (the 500-pose sub-graph, linear_solver 1); which solver is in force is asserted"""
    g, ogn = sub(pgo, n_poses), GR.subgraph(oracle, n_poses)
    loops = np.nonzero(np.asarray(ogn.kind) != 0)[0]
    edge, ptr, comps = MC.cycling_table(ogn, loops, 17)
    x = MC.perturbed(ogn, 17, sigma=0.05)
    make = lambda: pgo.Solver(g, pgo.Options(method=0, max_iters=4, linear_solver=linear_solver, pose_ordering=0))
    s, f = make(), make()
    assert s.info().linear_solver == f.info().linear_solver == linear_solver
    s.set_poses(x)
    s.set_mixtures(edge, ptr, comps)
    st = s.mixture_select(apply=True)[2]
    assert st["n_changed"] == len(edge) > 256
    assert s.solve().iterations > 0               # a solve on the selected problem in between
    assert s.info().linear_solver == linear_solver
    s.set_mixtures()
    assert np.array_equal(s.get_edge_weights(), np.ones(g.n_edges))
    s.set_edge_weights(None)
    with pytest.raises(pgo.PgoError) as ei:
        s.mixture_select()
    assert ei.value.status == INVALID
    s.set_poses(np.array(g.poses))
    s.solve(), f.solve()
    assert s.info().linear_solver == f.info().linear_solver == linear_solver
    assert history(s) == history(f) and s.poses().tobytes() == f.poses().tobytes()
    s.close(); f.close()


def test_set_mixture_null_is_the_table(pgo, g500):
    kind = np.array(g500.kind)
    loops = np.nonzero(kind != 0)[0].astype(np.int32)
    meas = np.array(g500.meas)
    comps = np.zeros((2 * len(loops), 5))
    comps[0::2, :3] = comps[1::2, :3] = meas[loops]
    comps[0::2, 3:] = 1.0
    comps[1::2, 3:] = (MC.PI_NULL, MC.SCALE_NULL)
    a, b = trivial(pgo, g500), trivial(pgo, g500)
    a.set_mixture_null(MC.PI_NULL, MC.SCALE_NULL)
    b.set_mixtures(loops, 2 * np.arange(len(loops) + 1), comps)
    assert same(a.mixture_select(), b.mixture_select())
    (sa, ra), (sb, rb) = a.mixture_solve(max_rounds=3, final_iters=3), b.mixture_solve(max_rounds=3, final_iters=3)
    strip = lambda rr: [{k: v for k, v in r.items() if k != "seconds"} for r in rr]
    assert strip(ra) == strip(rb) and sa["objective"] == sb["objective"] and sa["n_mix"] == sb["n_mix"] == 956
    assert a.poses().tobytes() == b.poses().tobytes() and np.array_equal(a.mixture_selection(), b.mixture_selection())
    # a mask: the selected edges only
    sel = np.zeros(g500.n_edges, bool)
    sel[loops[::3]] = True
    a.set_mixture_null(0.5, 0.25, select=sel)
    assert a.mixture_select()[2]["n_mix"] == int(sel.sum())
    a.close(); b.close()


# ------------------------------------------------------------------ 4. end to end
@pytest.fixture(scope="module")
def planted(oracle, og):
    table, roles = MC.planted(og)
    return table, roles, MC.solve(oracle, og, table)


def test_mixture_solve_end_to_end(pgo, og, g500, planted):
    """Measured on an MI355X: see DESIGN.md section 4k for the pose deviation this test prints."""
    (edge, ptr, comps), roles, ref = planted
    E = g500.n_edges
    s = trivial(pgo, g500)
    s.set_mixtures(edge, ptr, comps)
    summ, rounds = s.mixture_solve()
    print("restatement: smallest margin per round", ["%.3e" % r["min_margin"] for r in ref.rounds])
    print("device: F per round", ["%.12e" % r["objective"] for r in rounds], "restated", ["%.12e" % r["objective"] for r in ref.rounds])
    assert summ["rounds"] == len(rounds) == len(ref.rounds) and not summ["hit_max_rounds"] and summ["n_mix"] == len(edge)
    for a, b in zip(rounds, ref.rounds):
        assert a["n_changed"] == b["n_changed"] and a["count"] == b["count"]
        assert abs(a["objective"] - b["objective"]) <= 1e-9 * abs(b["objective"])
    F = [r["objective"] for r in rounds]
    for a, b in zip(F, F[1:]):
        assert b <= a + MC.summation_bound(E, a)
    assert summ["objective"] <= F[-1] + MC.summation_bound(E, F[-1])
    assert abs(summ["objective"] - ref.objective) <= 1e-9 * abs(ref.objective) and abs(summ["offset"] - ref.offset) <= 1e-12 * abs(ref.offset)
    assert summ["n_would_change"] == ref.n_would_change == 0 and summ["final_solve"]["termination"] in (1, 2, 3)
    sel = s.mixture_selection()
    assert np.array_equal(sel, ref.selection)
    assert np.all(sel[roles == "bimodal"] == 1) and np.all(sel[roles == "slip"] == 0) and np.all(sel[roles == "bogus"] == 1)
    assert np.array_equal(s.get_edge_weights(), ref.weights)
    x = s.poses()
    dev = np.abs(x - ref.poses).max()
    print("mixture end to end: max pose deviation from the restatement %.3e m" % dev)
    assert dev < 1e-3
    assert dev <= POSE_BOUND
    # the rounds driven through the public calls: the selection after EVERY round is the restatement's (where its margin
    # decides), and the poses end where pgo_mixture_solve's do
    t = trivial(pgo, g500)
    t.set_mixtures(edge, ptr, comps)
    for k, r in enumerate(ref.rounds):
        chosen, q, st = t.mixture_select(apply=True)
        ok = r["margin"] > MC.MARGIN_REL * (1.0 + np.abs(r["q_best"]))
        assert ok.sum() >= 0.99 * len(edge) and np.array_equal(chosen[ok], r["chosen"][ok]), k
        if k > 0 and st["n_changed"] == 0:
            break
        t.lm_begin()
        t.lm_step(2)
    assert k == len(ref.rounds) - 1
    t.solve()
    assert np.array_equal(t.mixture_selection(), sel) and np.abs(t.poses() - x).max() <= 1e-9
    s.close(); t.close()


def test_objective_never_rises_under_cauchy(pgo, og, g500, planted):
    """the monotone property alone, with Cauchy(1.0) on the loop class (q is stated with the handle's own loss)"""
    (edge, ptr, comps), roles, _ = planted
    s = pgo.Solver(g500, pgo.Options(method=0), losses=[pgo.Loss("trivial"), pgo.Loss("cauchy", 1.0)])
    s.set_mixtures(edge, ptr, comps)
    summ, rounds = s.mixture_solve()
    F = [r["objective"] for r in rounds]
    print("cauchy: F per round", ["%.9e" % f for f in F], "final", summ["objective"])
    assert len(F) >= 2 and rounds[0]["n_changed"] == len(edge)
    for a, b in zip(F, F[1:]):
        assert b <= a + MC.summation_bound(g500.n_edges, a)
    assert summ["objective"] <= F[-1] + MC.summation_bound(g500.n_edges, F[-1])
    s.close()


# ------------------------------------------------------------------ 5. refusals and state
def _unchanged(s, make):
    f = make()
    s.solve(), f.solve()
    assert history(s) == history(f) and s.poses().tobytes() == f.poses().tobytes()
    f.close()


def _calls(s, edge, ptr, comps):
    return (lambda: s.set_mixtures(edge, ptr, comps), lambda: s.set_mixtures(), lambda: s.set_mixture_null(0.1, 0.1),
            lambda: s.mixture_select(), lambda: s.mixture_selection(), lambda: s.mixture_solve())


def test_unsupported_handles(pgo, monkeypatch):
    """(A batched handle is refused too -- requires(NOT_BATCH) -- but the union handle of a batch is not reachable through
    the C-ABI.)"""
    g = sub(pgo, 66)
    E = g.n_edges
    loops = np.nonzero(np.array(g.kind) != 0)[0][:5]
    edge, ptr = loops.astype(np.int32), 2 * np.arange(6, dtype=np.int32)
    comps = np.repeat(np.concatenate([np.array(g.meas)[loops], np.ones((5, 2))], axis=1), 2, axis=0)
    gi = pgo.Graph.from_arrays(g.poses, g.ia, g.ib, g.meas, g.kind, info=np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (E, 1)))
    makers = [lambda: pgo.Solver(g, pgo.Options(method=1, max_iters=3)), lambda: pgo.Solver(g, pgo.Options(method=2, max_iters=3)),
              lambda: pgo.Solver(gi, pgo.Options(method=0, info_weighting=1, max_iters=3))]
    for make in makers:
        s = make()
        for call in _calls(s, edge, ptr, comps):
            with pytest.raises(pgo.PgoError) as ei:
                call()
            assert ei.value.status == UNSUPPORTED
        _unchanged(s, make)
        s.close()
    monkeypatch.setenv("PGO_FORCE_COLLECTIVES", "1")
    u = pgo.Solver(g, pgo.Options(method=0))
    monkeypatch.delenv("PGO_FORCE_COLLECTIVES")
    for call in _calls(u, edge, ptr, comps):
        with pytest.raises(pgo.PgoError) as ei:
            call()
        assert ei.value.status == UNSUPPORTED
    u.close()


def test_invalid_arguments_change_nothing(pgo, og, g500):
    (edge, ptr, comps), x = MC.select_case(og, 257)
    n = len(edge)
    make = lambda: trivial(pgo, g500, max_iters=4)
    s = make()
    for call in (lambda: s.mixture_select(), lambda: s.mixture_selection(), lambda: s.mixture_solve()):     # no table yet
        with pytest.raises(pgo.PgoError) as ei:
            call()
        assert ei.value.status == INVALID
    s.set_mixtures(edge, ptr, comps)
    before = s.mixture_select()

    def refused(e=edge, p=ptr, c=comps, text=None):
        with pytest.raises(pgo.PgoError) as ei:
            s.set_mixtures(e, p, c)
        assert ei.value.status == INVALID and (text is None or text in str(ei.value)), str(ei.value)
        assert same(s.mixture_select(), before)          # the table in force is the old one

    e2 = edge.copy(); e2[5] = e2[4]
    refused(e=e2, text="mixture 5 (edge %d)" % e2[5])
    e2 = edge.copy(); e2[-1] = g500.n_edges
    refused(e=e2, text="out of range")
    p2 = ptr.copy(); p2[3] = p2[2]
    refused(p=p2, text="mixture 2")
    p9 = np.concatenate([[0], [9], 9 + np.arange(1, n)]).astype(np.int32)
    refused(p=p9, c=np.tile([0.0, 0.0, 0.0, 1.0, 1.0], (9 + n, 1)), text="mixture 0")
    for col, bad in ((1, np.nan), (2, np.inf), (3, 0.0), (3, np.nan), (4, 0.0), (4, 1.5), (4, np.inf)):
        c2 = comps.copy()
        c2[ptr[7], col] = bad
        refused(c=c2, text="mixture 7 (edge %d)" % edge[7])
    L = pgo.lib()
    assert L.pgo_set_mixtures(s._h, n, None, None, None) == INVALID
    assert L.pgo_get_mixture_selection(s._h, None) == INVALID
    for pi, sc in ((0.0, 0.5), (np.nan, 0.5), (1.0, 0.0), (1.0, 1.5), (1.0, np.nan)):
        with pytest.raises(pgo.PgoError) as ei:
            s.set_mixture_null(pi, sc)
        assert ei.value.status == INVALID
    for kw in (dict(inner_iters=0), dict(final_iters=0), dict(max_rounds=0)):
        with pytest.raises(pgo.PgoError) as ei:
            s.mixture_solve(**kw)
        assert ei.value.status == INVALID
    assert same(s.mixture_select(), before) and np.all(s.mixture_selection() == -1)
    assert np.array_equal(s.get_edge_weights(), np.ones(g500.n_edges))
    _unchanged(s, make)                                  # nothing was applied: the solve is a fresh handle's
    s.close()


def test_state_rules(pgo, og, g500):
    (edge, ptr, comps), x = MC.select_case(og, 257)
    s = trivial(pgo, g500)
    s.set_mixtures(edge, ptr, comps)
    # a measuring select leaves a running solve alone; an applying one, setting and clearing make it stale
    s.lm_begin()
    s.lm_step(1)
    s.mixture_select()
    s.lm_step(1)
    for change in (lambda: s.mixture_select(apply=True), lambda: s.set_mixtures(), lambda: s.set_mixtures(edge, ptr, comps) or s.mixture_select(apply=True)):
        s.lm_begin()
        change()
        with pytest.raises(pgo.PgoError) as ei:
            s.lm_step(1)
        assert ei.value.status == INVALID
    # last writer wins on a mixture edge's weight; pgo_set_losses and pgo_set_active leave table and selection alone
    sel = s.mixture_selection()
    w = s.get_edge_weights()
    s.set_edge_weights(np.full(g500.n_edges, 0.5))
    assert np.all(s.get_edge_weights() == 0.5)
    s.set_losses(pgo.Loss("cauchy", 0.3))
    s.set_active(edge_active=np.ones(g500.n_edges, bool))
    s.set_losses(pgo.Loss("trivial"))
    assert np.array_equal(s.mixture_selection(), sel)
    st = s.mixture_select(apply=True)[2]
    w2 = s.get_edge_weights()
    assert st["n_changed"] == 0 and np.array_equal(w2[edge], w[edge]) and np.all(np.delete(w2, edge) == 0.5)
    # the consumers of the planes see the selected problem: the cost is the sum of the selected components' costs
    ew = s.edge_weights()
    assert abs(cost(s) - ew["cost"].sum()) <= 1e-12 * cost(s)
    s.close()


# ------------------------------------------------------------------ 6. the C++ mirror and the CLI
def test_cli_mixture_null_is_the_librarys(pgo, tmp_path):
    """main DATASET 0 0 --mixture-null PI:SCALE (pgo::SolveMixture of host/pgo_problem.h) on the 300-pose sub-graph written as
    a g2o file: the rounds, weights.txt and the written-back poses are those of Solver.mixture_solve on the file's graph with
    the Trivial loss on the loop class"""
    import subprocess
    from importlib import import_module
    exe = import_module("toy_robust_backend_slam_amd._build").build_cli()
    data, save = tmp_path / "data", tmp_path / "save"
    data.mkdir()
    sub(pgo, 300).write_g2o(str(data / "SUB300.g2o"))
    g = pgo.ReadG2O(str(data / "SUB300.g2o"))       # (the loader's own classes: odometry iff |a - b| < 5, everything else closure)
    kind = np.array(g.kind)
    spec = "%g:%g" % (MC.PI_NULL, MC.SCALE_NULL)
    p = subprocess.run([exe, "SUB300", "0", "0", "--mixture-null", spec, "--data", str(data), "--save", str(save), "--precision", "17"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    s = pgo.Solver(g, pgo.Options(method=0), losses=[pgo.Loss("huber", 0.01), pgo.Loss("trivial")])
    s.set_mixture_null(MC.PI_NULL, MC.SCALE_NULL, select=kind != 0)
    summ, rounds = s.mixture_solve()
    n_null = int((s.mixture_selection() == 1).sum())
    assert summ["rounds"] >= 2 and n_null > 0
    assert "mixture: %d rounds, %d mixture blocks, %d on the null hypothesis, %d would change" % (
        summ["rounds"], summ["n_mix"], n_null, summ["n_would_change"]) in p.stdout
    assert p.stdout.count("mixture round ") == summ["rounds"]
    w = np.loadtxt(str(save / "weights.txt"))
    assert np.array_equal(w, s.get_edge_weights()) and (w == MC.SCALE_NULL).sum() == n_null
    nodes = np.loadtxt(str(save / "opt_nodes.txt"))
    assert np.array_equal(nodes[:, 1:4], s.poses())
    s.close()
    # --mixture-null is METHOD 0's
    assert subprocess.run([exe, "SUB300", "0", "1", "--mixture-null", spec, "--data", str(data), "--save", str(save)], capture_output=True).returncode != 0
