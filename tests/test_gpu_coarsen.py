"""pgo_coarsen and pgo_prolong on the device (include/pgo.h, "hierarchical initialisation") against the host statement
pgo_coarsen_plan / pgo_prolong_eval -- structure exactly, numbers to the bounds derived in tests/_coarsen_cases.py -- and what
the calls promise about the handle: reproducible bits, an untouched LM state, constant poses that stay."""
import numpy as np
import pytest

import _coarsen_cases as CC

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -8
GPU_STRIDES = (2, 7, 64, 65, 256)     # one pose per lane up to 64, then 2 .. 4 per lane
PARITY = 5e-6   # the pose-parity bound of the golden LM tests (test_gpu_parity.py)


def graph_of(pgo, name):
    if name in ("synth600", "intel50"):
        return getattr(CC, name)(pgo)
    if name.startswith("exact"):
        P, ia, ib, meas, kind = CC.exact_graph(int(name[5:]), 12, seed=5)
        return pgo.Graph.from_arrays(P + np.random.default_rng(1).normal(0, 0.1, P.shape), ia, ib, meas, kind)
    return CC.dataset(pgo, name)


def coarse_dict(graph, origin):
    return {"n_poses": graph.n_poses, "ia": np.array(graph.ia), "ib": np.array(graph.ib), "meas": np.array(graph.meas),
            "kind": np.array(graph.kind), "origin": origin, "poses": np.array(graph.poses)}


def bits(d):
    return b"".join(np.ascontiguousarray(d[k]).tobytes() for k in ("ia", "ib", "meas", "kind", "origin", "poses"))


# ------------------------------------------------------------------------------------------------ 1. the device against the host statement
@pytest.mark.parametrize("name,strides", [("synth600", GPU_STRIDES), ("intel50", GPU_STRIDES), ("MIT", GPU_STRIDES),
                                           ("exact65", (64,)), ("exact129", (64,)), ("exact130", (2, 64, 65))])
def test_device_is_the_host_statement(pgo, name, strides):
    g = graph_of(pgo, name)
    n, ia, ib, meas, kind = CC.arrays(g)
    p0 = np.array(g.poses)
    s = pgo.Solver(g, pgo.Options(method=1))
    for S in strides:
        if n <= S:
            continue
        s.set_poses(p0)
        want = pgo.coarsen_plan(n, ia, ib, meas, kind, S)
        graph, origin = s.coarsen(S)
        got = coarse_dict(graph, origin)
        CC.assert_same_structure(got, want)
        assert got["poses"].tobytes() == np.ascontiguousarray(p0[::S]).tobytes()      # the current poses at the key poses
        assert np.array_equal(np.array(graph.info), np.tile([1.0, 0, 0, 1, 0, 1], (len(origin), 1)))
        tol_xy, tol_th = CC.bounds(n, ia, ib, meas, S)
        CC.assert_close_poses(got["meas"], want["meas"], tol_xy, tol_th, "%s S=%d coarse measurements" % (name, S))
        assert np.abs(got["meas"][:, 2]).max() <= np.pi
        X = p0[::S] + np.random.default_rng(S).normal(0, 2, (want["n_poses"], 3))
        s.prolong(S, X)
        P = s.poses()
        ref = pgo.prolong_eval(n, S, want["C"], want["Cend"], X)
        ref[0] = p0[0]                                                                  # fixed_pose = 0 is not moved
        tol_xy, tol_th = CC.bounds(n, ia, ib, meas, S, X)
        CC.assert_close_poses(P, ref, tol_xy, tol_th, "%s S=%d prolongation" % (name, S))
        assert P[0].tobytes() == p0[0].tobytes() and P[S::S].tobytes() == np.ascontiguousarray(X[1:]).tobytes()   # key poses bitwise
    s.close()


# ------------------------------------------------------------------------------------------------ 2. the same bits every time
def test_bitwise_across_calls_orderings_and_grids(pgo):
    g = CC.synth600(pgo)
    n = g.n_poses
    runs = {}
    for tag, ordering, grid in (("plain", 0, -1), ("reordered", 1, -1), ("grid1", 0, 1), ("grid3", 1, 3)):
        pgo.set_knob("coarsen_grid", grid)
        try:
            s = pgo.Solver(g, pgo.Options(method=1, pose_ordering=ordering))
            out = []
            for S in (7, 65):
                X = np.array(g.poses)[::S] + np.random.default_rng(S).normal(0, 2, (-(-n // S), 3))
                a, b = coarse_dict(*s.coarsen(S)), coarse_dict(*s.coarsen(S))
                assert bits(a) == bits(b), (tag, S)
                s.prolong(S, X)
                pa = s.poses()
                s.set_poses(np.array(g.poses))
                s.prolong(S, X)
                assert pa.tobytes() == s.poses().tobytes(), (tag, S)
                s.set_poses(np.array(g.poses))
                out.append(bits(a) + pa.tobytes())
            runs[tag] = out
            s.close()
        finally:
            pgo.set_knob("coarsen_grid", -1)
    for tag in ("reordered", "grid1", "grid3"):
        assert runs[tag] == runs["plain"], tag


# ------------------------------------------------------------------------------------------------ 3. the handle is left as it was
def test_coarsen_leaves_the_solve_alone_and_prolong_makes_it_stale(pgo):
    g = CC.synth600(pgo)
    runs = []
    for call in (False, True):
        s = pgo.Solver(g, pgo.Options(method=1))
        s.lm_begin()
        s.lm_step(2)
        if call:
            before = s.info().device_bytes
            s.coarsen(16)
            s.coarsen(64)
            grown = s.info().device_bytes
            s.coarsen(16)
            assert grown > before and s.info().device_bytes == grown      # repeated calls of one size allocate nothing
        s.lm_step(2)
        runs.append((s.iter_records(), s.poses()))
        if call:
            s.prolong(16, s.poses()[::16])
            with pytest.raises(pgo.PgoError) as ei:
                s.lm_step(1)
            assert ei.value.status == INVALID_ARG
            s.lm_begin()
            s.lm_step(1)
        s.close()
    (ra, pa), (rb, pb) = runs
    assert len(ra) == len(rb) == 5
    for x, y in zip(ra, rb):
        for k in x:
            if k != "seconds":
                assert np.float64(x[k]).tobytes() == np.float64(y[k]).tobytes(), k
    assert pa.tobytes() == pb.tobytes()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals(pgo, monkeypatch):
    g = CC.synth600(pgo)
    s = pgo.Solver(g, pgo.Options(method=1))
    p0 = s.poses()
    with pytest.raises(pgo.PgoError) as ei:                       # no composites yet
        s.prolong(16, p0[::16])
    assert ei.value.status == INVALID_ARG
    s.coarsen(16)
    with pytest.raises(pgo.PgoError) as ei:                       # composites of another stride
        s.prolong(8, p0[::8])
    assert ei.value.status == INVALID_ARG
    for S in (1, 257, 600):
        with pytest.raises(pgo.PgoError) as ei:
            s.coarsen(S)
        assert ei.value.status == INVALID_ARG
    assert s.poses().tobytes() == p0.tobytes()
    s.prolong(16, p0[::16])                                       # the composites of stride 16 survived the refused calls
    s.close()
    for kw in (dict(method=2), dict(method=0, info_weighting=1)):  # graph operations: any METHOD, info weighting
        u = pgo.Solver(g, pgo.Options(**kw))
        graph, origin = u.coarsen(16)
        assert graph.n_poses == 38 and len(origin) == graph.n_edges
        u.close()
    monkeypatch.setenv("PGO_FORCE_COLLECTIVES", "1")
    u = pgo.Solver(g, pgo.Options(method=1))
    monkeypatch.delenv("PGO_FORCE_COLLECTIVES")
    for call in (lambda: u.coarsen(16), lambda: u.prolong(16, p0[::16])):
        with pytest.raises(pgo.PgoError) as ei:
            call()
        assert ei.value.status == UNSUPPORTED
    u.close()
    n, ia, ib, meas, kind = CC.arrays(g)
    cut = np.ones(len(ia), bool)
    cut[np.nonzero((np.minimum(ia, ib) == 41) & (np.maximum(ia, ib) == 42))[0]] = False
    u = pgo.Solver(pgo.Graph.from_arrays(np.array(g.poses), ia[cut], ib[cut], meas[cut], kind[cut]), pgo.Options(method=1))
    with pytest.raises(pgo.PgoError) as ei:                       # a missing chain pair, named
        u.coarsen(16)
    assert ei.value.status == UNSUPPORTED and "poses 41 and 42" in str(ei.value)
    u.close()


# ------------------------------------------------------------------------------------------------ 5. constant poses stay
@pytest.mark.parametrize("ordering", [0, 1])
def test_constant_poses_are_not_moved(pgo, ordering):
    g = CC.synth600(pgo)
    n, S = g.n_poses, 7
    p0 = np.array(g.poses)
    X = p0[::S] + np.random.default_rng(2).normal(0, 2, (-(-n // S), 3))
    free = pgo.Solver(g, pgo.Options(method=1, fixed_pose=-1, pose_ordering=ordering))
    free.coarsen(S)
    free.prolong(S, X)
    moved = free.poses()
    free.close()
    assert (moved != p0).any(axis=1).all()
    s = pgo.Solver(g, pgo.Options(method=1, fixed_pose=75, pose_ordering=ordering))
    s.coarsen(S)
    s.prolong(S, X)
    want = moved.copy()
    want[75] = p0[75]
    assert s.poses().tobytes() == want.tobytes()
    const = np.zeros(n, bool)
    const[[0, 14, 15, 300, 599]] = True
    s.set_poses(p0)
    s.set_active(pose_constant=const)
    s.prolong(S, X)
    want[const] = p0[const]
    assert s.poses().tobytes() == want.tobytes()
    s.close()


# ------------------------------------------------------------------------------------------------ 6. the command line
def test_cli_starts_from_the_coarse_solution(pgo, tmp_path):
    """--init-stride S: the solve starts at the cost of the Python route's prolonged poses (printed with seven digits); a stride
    out of range is exit status 2"""
    import subprocess
    from importlib import import_module
    from conftest import DATA
    exe = import_module("toy_robust_backend_slam_amd._build").build_cli()
    g = CC.intel50(pgo)
    s = pgo.Solver(g, pgo.Options(method=1))
    plain = s.evaluate(want_r=False, want_J=False)[0]
    summ = s.initialize_hierarchical(16)
    cost = s.evaluate(want_r=False, want_J=False)[0]
    s.close()
    base = [exe, "INTEL", "50", "1", "--seed", "1", "--data", DATA, "--save", str(tmp_path / "save")]
    p = subprocess.run(base + ["--init-stride", "16"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    line = [l for l in p.stdout.splitlines() if l.startswith("init-stride 16: ")]
    assert len(line) == 1 and "coarse graph of 77 poses" in line[0] and ("in %d iterations" % summ.iterations) in line[0]
    first = [float(l.split()[1]) for l in p.stdout.splitlines() if l.startswith("Initial ")]
    assert len(first) == 1 and abs(first[0] - cost) <= 1e-6 * cost and abs(first[0] - plain) > 1e-3 * plain
    p = subprocess.run(base + ["--init-stride", "1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "stride must be 2..256" in p.stderr


# ------------------------------------------------------------------------------------------------ 7. the point of it
def test_hierarchical_start_is_the_oracles(pgo, oracle):
    """synth_manhattan(2000, 4.0, 0.1, seed 3), METHOD 1, stride 16 (125 key poses).  On the CPU, against synth_manhattan_truth:
    the dead-reckoned poses have an ATE rmse of 4.837007 m; the restatement's coarse graph solved by the oracle (lm_direct, 50
    iterations allowed, 23 taken) and prolonged by the restatement has 0.267958 m -- a factor of 18.05.  The device route
    (initialize_hierarchical) must reach half that factor, and its ATE must lie within PARITY (1 + L) of the oracle route's: the
    pose-parity bound of the exact-mode solves on the coarse poses, whose angle part turns composites no longer than the
    longest segment path L."""
    n, seed, S = 2000, 3, 16
    g = pgo.synth_manhattan(n, 4.0, 0.1, seed)
    truth = pgo.synth_manhattan_truth(n, seed)
    n_, ia, ib, meas, kind = CC.arrays(g)
    dead = pgo.trajectory_error(np.array(g.poses), truth)["ate_rmse"]
    co = CC.restate_coarsen(n, ia, ib, meas, kind, S)
    og = oracle.Graph(np.arange(co["n_poses"], dtype=np.int32), np.array(g.poses)[::S].copy(), co["ia"], co["ib"], co["meas"],
                      np.tile([1.0, 0, 0, 1, 0, 1], (len(co["ia"]), 1)), co["kind"])
    ores = oracle.lm_direct(og, oracle.Options(method=1, max_iters=50))
    want = pgo.trajectory_error(CC.restate_prolong(n, S, co["C"], co["Cend"], ores.poses), truth)["ate_rmse"]
    chain, _ = CC.chain_edges(n, ia, ib)
    step = np.hypot(meas[chain[:n - 1], 0], meas[chain[:n - 1], 1])
    L = max(step[k * S:(k + 1) * S].sum() for k in range(co["n_poses"]))
    s = pgo.Solver(g, pgo.Options(method=1))
    summ = s.initialize_hierarchical(S)
    got = s.trajectory_error(truth)["ate_rmse"]
    s.close()
    print("dead reckoning %.6f, oracle route %.6f (factor %.2f), device route %.6f (coarse solve: %d iterations, termination %d), "
          "distance %.3e (bound %.3e)" % (dead, want, dead / want, got, summ.iterations, summ.termination, abs(got - want), PARITY * (1 + L)))
    assert abs(dead - 4.837007) < 1e-6 and abs(want - 0.267958) < 1e-6      # the recorded numbers are these
    assert got * (18.05 / 2) < dead
    assert abs(got - want) <= PARITY * (1 + L)
