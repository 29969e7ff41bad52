"""pgo_window_solve / pgo_batch_window_solve on the GPU: many small windows of a live handle's graph, one workgroup each, the
whole LM loop on the device.

Yardsticks: the CPU oracle (oracle.lm_direct, _active_cases.lm_direct_const, _loss_restatement.lm) on the EXTRACTED window --
the listed poses numbered by list position, the listed edges in list order -- and the product's older path (set_active +
solve).  The window kernel is never compared with itself, except where the claim IS bitwise self-consistency (two calls,
pose_ordering, batch against solo, one call against several).  Input: INTEL + 50 bogus loops, seed 1; its loop and bogus edges
are 1227..1532."""
import ctypes as C

import numpy as np
import pytest

import _active_cases as AC
import _loss_restatement as LR
import _window_cases as WC

pytestmark = pytest.mark.gpu

HANDFUL = [1227, 1300, 1381, 1501, 1521, 1532]


@pytest.fixture(scope="module")
def case(pgo):
    g, a = WC.graph(pgo)
    return dict(g=g, a=a, n=len(a["poses"]), E=len(a["ia"]))


def _win(pgo, case, e, radius=10):
    return WC.plan(pgo, case["a"], [e], radius)


# ---------------------------------------------------------------------------------------------------------- 1. sweep
@pytest.mark.parametrize("method", [0, 1])
def test_sweep_all_loop_windows_in_one_call(pgo, oracle, case, method):
    """All 306 windows window_plan([e], 10) in ONE call (more windows than CUs), max_iters 4, against the oracle on each
    extracted window: every accept / reject decision, the termination and the counts equal; initial cost 1e-12, poses 1e-6,
    final cost 1e-7 relative (floor 1e-9 x initial cost: several windows converge to 1e-11 .. 1e-15).
    302 windows have 42 poses and 41 edges; 1460 (26 / 26), 1482 (38 / 38) and 1501 (33 / 33) have overlapping ranges, 1521
    (38 / 37) is clipped at the last pose.  Measured on MI355X: max |d pose| 1.4e-10 (METHOD 0) / 3.9e-11
    (METHOD 1); |d final cost| at most 1.1e-3 / 3.1e-3 of its bound."""
    wins, refs = WC.sweep(pgo, oracle, method)
    assert len(wins) == 306
    sizes = {e: (len(w[0]), len(w[1])) for e, w in zip(WC.LOOP_EDGES, wins)}
    assert sizes[1501] == (33, 33) and sum(1 for v in sizes.values() if v == (42, 41)) == 302
    assert (sizes[1460], sizes[1482], sizes[1521]) == ((26, 26), (38, 38), (38, 37))
    # the premise: the oracle's histories cover every branch (checked on the CPU when the cases were chosen)
    hist = {e: tuple(r["hist"]) for e, r in zip(WC.LOOP_EDGES, refs)}
    count = lambda h: sum(1 for v in hist.values() if v == h)
    if method == 0:
        assert (count((1, 1, 1, 1, 1)), count((1, 1, 1, 1, 0)), count((1, 1, 1, 0, 1))) == (257, 39, 5)
        assert [e for e, v in hist.items() if v == (1, 1, 0, 1, 1)] == [1381, 1394, 1509, 1520] and hist[1505] == (1, 1, 1, 0, 0)
        assert all(r["termination"] == 4 for r in refs)
    else:
        assert count((1, 0)) == 21 and hist[1501] == (1, 1, 1, 0) and refs[1501 - 1227]["termination"] == 1
        assert sum(1 for r in refs if r["termination"] == 1) == 22 and sum(1 for r in refs if r["termination"] == 4) == 284
    s = pgo.Solver(case["g"], pgo.Options(method=method))
    before = s.poses()
    poses, res, recs = s.window_solve(wins, max_iters=WC.SWEEP_ITERS, want_records=True)
    assert s.poses().tobytes() == before.tobytes()
    worst_p = worst_c = 0.0
    for e, x, r, rc, ref in zip(WC.LOOP_EDGES, poses, res, recs, refs):
        dp, dc = WC.check_against_oracle(x, r, rc, ref, f"edge {e} METHOD {method}")
        worst_p, worst_c = max(worst_p, dp), max(worst_c, dc)
        assert [q["iter"] for q in rc] == list(range(len(rc))) and all(q["pcg_iters"] == 0 and q["seconds"] == 0.0 for q in rc)
        if ref["records"] is not None:      # the rows themselves, loosely: they are the oracle's rows
            for q, o in zip(rc, ref["records"]):
                assert q["radius"] == pytest.approx(o["radius"], rel=1e-6)
                assert q["cost"] == pytest.approx(o["cost"], rel=1e-6, abs=1e-9 * ref["initial_cost"])
    print(f"sweep METHOD {method}: 306 windows, max |d pose| vs oracle {worst_p:.2e}, max |d final cost| / bound {worst_c:.2e}")
    s.close()


# ------------------------------------------------------------------------------- 2. against the product's older path
@pytest.mark.parametrize("method", [0, 1])
def test_against_set_active_and_solve(pgo, case, method):
    """the same windows through pgo_set_active + pgo_solve (PCG to 1e-12): poses within 1e-9, the suite's bound between two
    product paths"""
    a, n = case["a"], case["n"]
    wins = [_win(pgo, case, e) for e in HANDFUL]
    w = pgo.Solver(case["g"], pgo.Options(method=method))
    poses, res = w.window_solve(wins, max_iters=4)
    w.close()
    s = pgo.Solver(case["g"], pgo.Options(method=method, max_iters=4, linear_solver=1, pcg_rtol=1e-12, pcg_max_iters=400000))
    for e, (pidx, eidx, anchor), x, r in zip(HANDFUL, wins, poses, res):
        m = np.zeros(case["E"], bool)
        m[eidx] = True
        pc = np.zeros(n, bool)
        pc[anchor] = True
        s.set_poses(a["poses"])
        s.set_active(m, pc)
        summ = s.solve()
        d = np.abs(s.poses()[pidx] - x).max()
        print(f"edge {e} METHOD {method}: window kernel vs set_active + solve: max |d pose| {d:.2e}; costs {r.final_cost!r} / {summ.final_cost!r}")
        assert (summ.termination, summ.iterations, summ.successful_steps) == (r.termination, r.iterations, r.successful_steps)
        assert d < 1e-9
    s.close()


# ------------------------------------------------------------------------------------------------------ 3. size edges
def _edge_between(a, i, j):
    k = np.nonzero((a["ia"] == i) & (a["ib"] == j))[0]
    return int(k[0])


def _size_cases(pgo, case):
    a = case["a"]
    run = lambda lo, cnt: (np.arange(lo, lo + cnt), np.array([_edge_between(a, i, i + 1) for i in range(lo, lo + cnt - 1)]))
    p42, e42, an42 = _win(pgo, case, 1300)
    cap = pgo.WINDOW_MAX_POSES
    pc, ec = run(300, cap)
    p2, e2 = run(100, 2)
    p3, e3 = run(100, 3)
    return {
        "2 poses, 1 edge": (p2, e2, 100),
        "3 poses": (p3, e3, 101),
        "anchor in the middle": (p42, e42, int(p42[20])),
        "anchor last": (p42, e42, int(p42[-1])),
        "descending pose list": (p42[::-1].copy(), e42, an42),
        "shuffled lists": (np.random.default_rng(5).permutation(p42), np.random.default_rng(6).permutation(e42), an42),
        "an edge listed twice": (p42, np.concatenate([e42, e42[-1:]]), an42),
        "two edges listed twice": (p3, np.array([e3[0], e3[1], e3[0], e3[1]]), 100),
        "a listed pose without an edge": (np.concatenate([p42, [5, 900]]), e42, an42),
        "exactly the cap": (pc, ec, 300),
    }


@pytest.mark.parametrize("method", [0, 1])
def test_size_edges(pgo, oracle, case, method):
    """the smallest and the largest windows, every place an anchor can be, lists in any order, repeated edges, unused poses; the
    handle's poses are INTEL's plus N(0, 0.01) noise, so that chains of odometry edges have something to do"""
    a = case["a"]
    cases = _size_cases(pgo, case)
    s = pgo.Solver(case["g"], pgo.Options(method=method))
    s.set_poses(a["poses"] + np.random.default_rng(11).normal(0, 0.01, a["poses"].shape))
    x0 = s.poses()
    names = list(cases)
    poses, res, recs = s.window_solve([cases[k] for k in names], max_iters=4, want_records=True)
    for name, x, r, rc in zip(names, poses, res, recs):
        w = cases[name]
        ref = WC.oracle_window(oracle, a, w, method, 4, poses=x0)
        dp, dc = WC.check_against_oracle(x, r, rc, ref, name)
        print(f"{name} METHOD {method}: hist {ref['hist']} term {r.termination}; max |d pose| {dp:.2e}, |d cost| / bound {dc:.2e}")
        g, const = WC.extracted(oracle, a, w)
        assert x[const].tobytes() == x0[np.asarray(w[0])][const].tobytes(), name     # constant poses: bitwise
        assert r.successful_steps >= 1 and not np.array_equal(x[~const], x0[np.asarray(w[0])][~const]), name
    x = poses[names.index("a listed pose without an edge")]
    assert x[-2:].tobytes() == x0[[5, 900]].tobytes()
    assert len(cases["exactly the cap"][0]) == pgo.WINDOW_MAX_POSES
    assert s.poses().tobytes() == x0.tobytes()
    s.close()


def test_window_above_the_cap_is_unsupported(pgo, case):
    a = case["a"]
    big = WC.plan(pgo, a, [1500, 1501], 10)
    assert len(big[0]) == 75 > pgo.WINDOW_MAX_POSES
    s = pgo.Solver(case["g"], pgo.Options(method=1))
    ok = _win(pgo, case, 1300)
    for commit in (False, True):
        with pytest.raises(pgo.PgoError) as ei:
            s.window_solve([ok, big], commit=commit)
        assert ei.value.status == -8 and "window 1" in str(ei.value)
        assert s.poses().tobytes() == a["poses"].tobytes()
    many = (np.arange(0, 4), np.array([0, 1, 2] * 86), 0)          # 258 edges on 4 poses
    assert len(many[1]) > pgo.WINDOW_MAX_EDGES
    with pytest.raises(pgo.PgoError) as ei:
        s.window_solve([many])
    assert ei.value.status == -8
    s.window_solve([(np.arange(0, 4), np.array(([0, 1, 2] * 86)[:pgo.WINDOW_MAX_EDGES]), 0)])     # exactly the edge cap runs
    s.close()


def test_edge_cap_against_the_oracle(pgo, oracle, case):
    """WINDOW_MAX_EDGES residual blocks on 4 poses (every lane an edge, 86 contributions per block)"""
    a = case["a"]
    w = (np.arange(0, 4), np.array(([0, 1, 2] * 86)[:pgo.WINDOW_MAX_EDGES]), 0)
    s = pgo.Solver(case["g"], pgo.Options(method=0))
    s.set_poses(a["poses"] + np.random.default_rng(2).normal(0, 0.01, a["poses"].shape))
    x0 = s.poses()
    poses, res, recs = s.window_solve([w], max_iters=3, want_records=True)
    WC.check_against_oracle(poses[0], res[0], recs[0], WC.oracle_window(oracle, a, w, 0, 3, poses=x0), "edge cap")
    s.close()


# ---------------------------------------------------------------------------------------------------------- 4. losses
@pytest.mark.parametrize("method", [0, 1])
def test_losses_follow_the_handle(pgo, oracle, case, method):
    """Cauchy(0.1) on the loop class after set_losses: the window kernel follows the handle's classes"""
    a = case["a"]
    losses = [("huber", 0.01), ("cauchy", 0.1)]
    s = pgo.Solver(case["g"], pgo.Options(method=method))
    wins = [_win(pgo, case, e) for e in (1300, 1505, 1512)]
    plain = s.window_solve(wins, max_iters=4)[1]
    s.set_losses([pgo.Loss(n, v) for n, v in losses])
    poses, res, recs = s.window_solve(wins, max_iters=4, want_records=True)
    for w, x, r, rc, r0 in zip(wins, poses, res, recs, plain):
        og, const = WC.extracted(oracle, a, w)
        ref = LR.lm(oracle, og, losses, LR.classes(og.kind, 2), method=method, max_iters=4, fixed_pose=int(np.nonzero(const)[0][0]))
        refd = dict(poses=ref.poses, termination=ref.termination, iterations=ref.iterations, successful_steps=ref.successful_steps,
                    initial_cost=ref.initial_cost, final_cost=ref.final_cost, hist=[q["step_ok"] for q in ref.records])
        dp, dc = WC.check_against_oracle(x, r, rc, refd, "cauchy")
        print(f"cauchy METHOD {method}: initial cost {r.initial_cost!r} (huber: {r0.initial_cost!r}), max |d pose| {dp:.2e}")
        assert r.initial_cost != r0.initial_cost
    s.close()


# ----------------------------------------------------------------------------------------------- 5. failure isolation
def _singular_graph(pgo):
    """12 poses on a line, noisy; pose 7 turned by pi / 2 and joined to pose 4 by a loop with heading 0: sin(delta) = 1.0"""
    rng = np.random.default_rng(3)
    poses = np.zeros((12, 3))
    poses[:, 0] = np.arange(12)
    poses += rng.normal(0, 0.02, poses.shape)
    poses[4] = [4, 0, 0]
    poses[7] = [7, 0, np.pi / 2]
    ia = [0, 1, 2, 4, 5, 8, 9, 10, 4]
    ib = [1, 2, 3, 5, 6, 9, 10, 11, 7]
    meas = [[1, 0, 0]] * 8 + [[3, 0, 0]]
    return pgo.Graph.from_arrays(poses, ia, ib, meas, [0] * 8 + [1]), poses


@pytest.mark.parametrize("method", [0, 1])
def test_a_failing_window_is_isolated(pgo, method):
    g, poses0 = _singular_graph(pgo)
    wins = [(np.arange(0, 4), np.array([0, 1, 2]), 0), (np.arange(4, 8), np.array([3, 4, 8]), 4), (np.arange(8, 12), np.array([5, 6, 7]), 8)]
    s = pgo.Solver(g, pgo.Options(method=method))
    with pytest.raises(pgo.PgoError) as e:      # the premise: d asin is +-inf on edge 8
        s.evaluate()
    assert e.value.status == -7
    poses, res, recs = s.window_solve(wins, max_iters=3, want_records=True)
    assert res[1].termination == 6 and res[1].iterations == 0 and res[1].n_records == 1
    assert poses[1].tobytes() == poses0[4:8].tobytes()
    for k in (0, 2):
        assert res[k].termination in (1, 2, 3, 4) and res[k].successful_steps >= 1 and np.isfinite(res[k].final_cost)
        assert res[k].final_cost < res[k].initial_cost
        alone = s.window_solve([wins[k]], max_iters=3, want_records=True)
        assert alone[0][0].tobytes() == poses[k].tobytes() and bytes(alone[1][0]) == bytes(res[k]) and alone[2][0] == recs[k]
    s.window_solve(wins, max_iters=3, commit=True)
    x = s.poses()
    assert x[4:8].tobytes() == poses0[4:8].tobytes() and x[0:4].tobytes() == poses[0].tobytes() and x[8:12].tobytes() == poses[2].tobytes()
    s.close()


# ----------------------------------------------------------------------------------------------------------- 6. state
def test_without_commit_the_handle_is_untouched(pgo, case):
    wins = [_win(pgo, case, e) for e in HANDFUL]
    out = []
    for call in (False, True):
        s = pgo.Solver(case["g"], pgo.Options(method=1, max_iters=10))
        s.lm_begin()
        s.lm_step(2)
        if call:
            s.window_solve(wins, max_iters=4, commit=False, want_records=True)
        s.lm_step(2)
        out.append((s.poses().tobytes(), s.iter_records()))
        s.close()
    strip = lambda recs: [{k: v for k, v in r.items() if k != "seconds"} for r in recs]
    assert out[0][0] == out[1][0] and strip(out[0][1]) == strip(out[1][1]) and len(out[0][1]) == 5


def test_commit_writes_exactly_the_listed_poses(pgo, case):
    a = case["a"]
    wins = [_win(pgo, case, e) for e in (1227, 1300, 1532)]
    listed = np.concatenate([w[0] for w in wins])
    assert len(np.unique(listed)) == len(listed)
    s = pgo.Solver(case["g"], pgo.Options(method=1))
    s.lm_begin()
    poses, res = s.window_solve(wins, max_iters=2, commit=True)
    x = s.poses()
    rest = np.ones(case["n"], bool)
    rest[listed] = False
    assert x[rest].tobytes() == a["poses"][rest].tobytes()
    for w, p in zip(wins, poses):
        assert x[w[0]].tobytes() == p.tobytes() and not np.array_equal(p, a["poses"][w[0]])
    with pytest.raises(pgo.PgoError) as ei:      # as after pgo_set_poses: the running solve is stale
        s.lm_step(1)
    assert ei.value.status == -1
    # overlapping lists under commit: refused before anything is launched; fine without commit
    before = s.poses()
    over = [wins[0], _win(pgo, case, 1228)]
    assert set(over[0][0]) & set(over[1][0])
    with pytest.raises(pgo.PgoError) as ei:
        s.window_solve(over, commit=True)
    assert ei.value.status == -1 and s.poses().tobytes() == before.tobytes()
    s.window_solve(over, commit=False)
    assert s.poses().tobytes() == before.tobytes()
    s.window_solve(wins, commit=True)             # (and the host-side marks of the refused call are gone)
    s.close()


def _blob(out):
    return b"".join(p.tobytes() for p in out[0]) + b"".join(bytes(r) for r in out[1]) + repr(out[2]).encode()


def test_two_calls_and_pose_ordering_are_bitwise_equal(pgo, case):
    wins = [_win(pgo, case, e) for e in WC.LOOP_EDGES[::7]]
    blobs = []
    for ordering in (0, 0, 1):
        s = pgo.Solver(case["g"], pgo.Options(method=1, pose_ordering=ordering))
        assert s.info().pose_ordering == ordering
        blobs.append(_blob(s.window_solve(wins, max_iters=4, want_records=True)))
        blobs.append(_blob(s.window_solve(wins, max_iters=4, want_records=True)))
        half = s.window_solve(wins[:5], max_iters=4, want_records=True)     # windows are independent of their company
        assert _blob(half) == _blob(tuple(x[:5] for x in s.window_solve(wins, max_iters=4, want_records=True)))
        s.close()
    assert all(b == blobs[0] for b in blobs)


def test_commit_with_pose_ordering(pgo, case):
    a = case["a"]
    wins = [_win(pgo, case, e) for e in (1227, 1300, 1532)]
    xs = []
    for ordering in (0, 1):
        s = pgo.Solver(case["g"], pgo.Options(method=1, pose_ordering=ordering))
        poses, _ = s.window_solve(wins, max_iters=2, commit=True)
        x = s.poses()
        for w, p in zip(wins, poses):
            assert x[w[0]].tobytes() == p.tobytes()
        xs.append(x.tobytes())
        s.close()
    assert xs[0] == xs[1]


def test_errors(pgo, case, monkeypatch):
    a = case["a"]
    ok = _win(pgo, case, 1300)
    p, e, an = ok
    s = pgo.Solver(case["g"], pgo.Options(method=1))

    def refused(status, wins, **kw):
        with pytest.raises(pgo.PgoError) as ei:
            s.window_solve(wins, **kw)
        assert ei.value.status == status, str(ei.value)
        assert s.poses().tobytes() == a["poses"].tobytes()

    assert s.window_solve([]) == ([], [])                                   # n_windows == 0
    refused(-1, [ok], max_iters=0)
    refused(-1, [ok], max_iters=pgo.WINDOW_MAX_ITERS + 1)
    s.window_solve([ok], max_iters=pgo.WINDOW_MAX_ITERS)
    refused(-1, [(np.concatenate([p, [case["n"]]]), e, an)])                # pose index out of range
    refused(-1, [(np.concatenate([p, [-1]]), e, an)])
    refused(-1, [(p, np.concatenate([e, [case["E"]]]), an)])                # edge index out of range
    refused(-1, [(p, np.concatenate([e, [-1]]), an)])
    refused(-1, [(np.concatenate([p, p[:1]]), e, an)])                      # a duplicate pose
    refused(-1, [(p[1:], e, int(p[1]))])                                    # an endpoint not in the list
    refused(-1, [(p, e, 5)])                                                # an anchor not in the list
    refused(-1, [(p, e, -1)])
    refused(-1, [ok, (p[1:], e, int(p[1]))], commit=True)                   # the second window is bad: nothing launched
    s.window_solve([ok, ok], commit=False)                                  # (no marks left behind by the refused calls)
    # null pointers at the C-ABI
    L = pgo.lib()
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    pp, ep, pi, ei_, av = i32([0, len(p)]), i32([0, len(e)]), i32(p), i32(e), i32([an])
    res = (pgo.WindowResult * 1)()
    assert L.pgo_window_solve(s._h, 1, ip(pp), ip(pi), ip(ep), ip(ei_), ip(av), 2, 0, None, None, None) == -1
    assert L.pgo_window_solve(s._h, 1, ip(pp), None, ip(ep), ip(ei_), ip(av), 2, 0, None, res, None) == -1
    assert L.pgo_window_solve(None, 1, ip(pp), ip(pi), ip(ep), ip(ei_), ip(av), 2, 0, None, res, None) == -1
    assert L.pgo_window_solve(s._h, 1, ip(pp), ip(pi), ip(ep), ip(ei_), ip(av), 2, 0, None, res, None) == 0     # poses_out may be NULL
    assert res[0].termination == 4 and res[0].iterations == 2
    s.close()
    for kw in (dict(method=2), dict(method=1, info_weighting=1)):
        u = pgo.Solver(case["g"], pgo.Options(**kw))
        with pytest.raises(pgo.PgoError) as ei:
            u.window_solve([ok])
        assert ei.value.status == -8
        u.close()
    monkeypatch.setenv("PGO_FORCE_COLLECTIVES", "1")
    u = pgo.Solver(case["g"], pgo.Options(method=1))
    monkeypatch.delenv("PGO_FORCE_COLLECTIVES")
    with pytest.raises(pgo.PgoError) as ei:
        u.window_solve([ok])
    assert ei.value.status == -8
    u.close()


# ----------------------------------------------------------------------------------------------------------- 7. batch
def test_batch_is_bitwise_the_solo_handles(pgo, case):
    """3 copies of the graph, copy k at the poses after k LM iterations; two windows on each in ONE call"""
    a = case["a"]
    s = pgo.Solver(case["g"], pgo.Options(method=1, max_iters=10))
    s.lm_begin()
    xs = [s.poses()]
    for _ in range(2):
        s.lm_step(1)
        xs.append(s.poses())
    s.close()
    assert not np.array_equal(xs[0], xs[1]) and not np.array_equal(xs[1], xs[2])
    graphs = [pgo.Graph.from_arrays(x, a["ia"], a["ib"], a["meas"], a["kind"], a["info"]) for x in xs]
    w1, w2 = _win(pgo, case, 1300), _win(pgo, case, 1505)
    order = [(2, w2), (0, w1), (1, w1), (2, w1), (1, w2), (0, w2)]
    b = pgo.Batch(graphs, pgo.Options(method=1))
    got = b.window_solve([(k,) + w for k, w in order], max_iters=4, want_records=True)
    assert all(b.poses(k).tobytes() == xs[k].tobytes() for k in range(3))
    solo = []
    for k in range(3):
        h = pgo.Solver(graphs[k], pgo.Options(method=1))
        solo.append(h)
    for i, (k, w) in enumerate(order):
        ref = solo[k].window_solve([w], max_iters=4, want_records=True)
        assert got[0][i].tobytes() == ref[0][0].tobytes() and bytes(got[1][i]) == bytes(ref[1][0]) and got[2][i] == ref[2][0]
    assert len({got[0][i].tobytes() for i in (1, 2, 3)}) == 3            # the three copies really differ
    # the commit lands in the right problem
    b.window_solve([(k,) + w for k, w in order], max_iters=4, commit=True)
    for k in range(3):
        x = b.poses(k)
        rest = np.ones(case["n"], bool)
        for i, (kk, w) in enumerate(order):
            if kk == k:
                assert x[w[0]].tobytes() == got[0][i].tobytes()
                rest[w[0]] = False
        assert x[rest].tobytes() == xs[k][rest].tobytes()
    # errors name the problem's own numbering
    for bad in ([(3,) + w1], [(-1,) + w1], [(0, np.concatenate([w1[0], [case["n"]]]), w1[1], w1[2])], [(0, w1[0], np.concatenate([w1[1], [case["E"]]]), w1[2])]):
        with pytest.raises(pgo.PgoError) as ei:
            b.window_solve(bad)
        assert ei.value.status == -1
    # a NULL `problem` (or any other list) at the C-ABI, with commit: refused, nothing written, no problem solved in its place
    L = pgo.lib()
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    pr, pp, ep, pi, ei_, av = i32([1]), i32([0, len(w1[0])]), i32([0, len(w1[1])]), i32(w1[0]), i32(w1[1]), i32([w1[2]])
    res = (pgo.WindowResult * 1)()
    res[0].termination = -7
    before = [b.poses(k).tobytes() for k in range(3)]
    assert L.pgo_batch_window_solve(b._h, 1, None, ip(pp), ip(pi), ip(ep), ip(ei_), ip(av), 2, 1, None, res, None) == -1
    assert L.pgo_batch_window_solve(b._h, 1, ip(pr), ip(pp), None, ip(ep), ip(ei_), ip(av), 2, 1, None, res, None) == -1
    assert L.pgo_batch_window_solve(b._h, 1, ip(pr), ip(pp), ip(pi), ip(ep), ip(ei_), ip(av), 2, 1, None, None, None) == -1
    assert L.pgo_batch_window_solve(None, 1, ip(pr), ip(pp), ip(pi), ip(ep), ip(ei_), ip(av), 2, 1, None, res, None) == -1
    assert res[0].termination == -7 and [b.poses(k).tobytes() for k in range(3)] == before
    assert L.pgo_batch_window_solve(b._h, 0, None, None, None, None, None, None, 2, 1, None, None, None) == 0
    with pytest.raises(pgo.PgoError) as ei:      # the error names the caller's own index
        b.window_solve([(1, np.concatenate([w1[0], [case["n"] + 3]]), w1[1], w1[2])])
    assert f"pose index {case['n'] + 3}" in str(ei.value) and "problem 1" in str(ei.value)
    assert L.pgo_batch_window_solve(b._h, 1, ip(pr), ip(pp), ip(pi), ip(ep), ip(ei_), ip(av), 2, 1, None, res, None) == 0
    assert res[0].termination in (1, 2, 3, 4) and b.poses(0).tobytes() == before[0] and b.poses(2).tobytes() == before[2]
    with pytest.raises(pgo.PgoError) as ei:      # the same poses twice in ONE problem overlap; in two problems they do not
        b.window_solve([(0,) + w1, (0,) + w1], commit=True)
    assert ei.value.status == -1
    b.window_solve([(0,) + w1, (1,) + w1], commit=True)
    for h in solo:
        h.close()
    b.close()
