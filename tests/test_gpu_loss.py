"""The robust loss family (pgo_set_losses: Trivial, Huber, SoftLOne, Cauchy, Arctan, Tukey; up to 4 classes) on the GPU,
against the numpy restatement of tests/_loss_restatement.py (Ceres' losses and corrector on the oracle's plain residual
blocks, Ceres' LM loop with a sparse LU), and the properties the C-ABI promises: the default path bitwise unchanged, the
batched and sharded handles, covariances, the stale-solve rule, the errors and the C++ / CLI drop-in surface."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _loss_restatement as LR
from conftest import DATA, ROOT, oracle_graph

pytestmark = pytest.mark.gpu

EDGE_TOL = 1e-11     # K1 against the restatement (the edge-kernel bound of test_edge_kernel_parity)
NAMES = list(LR.TYPES)


def load(pgo, name, n_out=0, seed=1):
    g = pgo.ReadG2O(os.path.join(DATA, name + ".g2o"))
    if n_out:
        g.add_random_C(n_out, seed)
    return g


def records_equal(ra, rb):
    for a, b in zip(ra, rb):
        assert {k: v for k, v in a.items() if k != "seconds"} == {k: v for k, v in b.items() if k != "seconds"}
    assert len(ra) == len(rb)


# ------------------------------------------------------------------ 1. the default path
@pytest.mark.parametrize("name,n_out,ls", [("INTEL", 50, 0), ("M3500", 0, 1)])
def test_default_losses_leave_the_solve_bitwise_unchanged(pgo, name, n_out, ls):
    """one explicit Huber(0.01) class = a handle without the call (K1's default instantiation), bitwise; three classes all
    Huber(0.01) (the general instantiation) agree to 1e-14"""
    g = load(pgo, name, n_out)
    opts = dict(method=1, pcg_max_iters=200000, linear_solver=ls)
    a = pgo.Solver(g, pgo.Options(**opts))
    assert a.info().linear_solver == (2 if ls == 0 else 1)
    sa = a.solve()
    b = pgo.Solver(g, pgo.Options(**opts), losses=pgo.Loss("huber", 0.01))
    sb = b.solve()
    assert (sa.final_cost, sa.iterations, sa.total_pcg_iters) == (sb.final_cost, sb.iterations, sb.total_pcg_iters)
    records_equal(a.iter_records(), b.iter_records())
    np.testing.assert_array_equal(a.poses(), b.poses())
    c = pgo.Solver(g, pgo.Options(**opts), losses=[pgo.Loss("huber", 0.01)] * 3)
    sc = c.solve()
    assert sc.iterations == sa.iterations and sc.termination == sa.termination
    for x, y in zip(a.iter_records(), c.iter_records()):
        assert x["step_ok"] == y["step_ok"] and abs(x["cost"] - y["cost"]) <= 1e-14 * abs(x["cost"])
    xa, xc = a.poses(), c.poses()
    assert np.abs(xa - xc).max() <= 1e-14 * np.abs(xa).max()
    # Trivial (one class) = huber_delta <= 0
    d = pgo.Solver(g, pgo.Options(max_iters=3, huber_delta=0.0, **opts))
    e = pgo.Solver(g, pgo.Options(max_iters=3, **opts), losses=pgo.Loss("trivial"))
    d.solve(), e.solve()
    records_equal(d.iter_records(), e.iter_records())
    np.testing.assert_array_equal(d.poses(), e.poses())
    for s in (a, b, c, d, e):
        s.close()


# ------------------------------------------------------------------ 2. K1 against the restatement
def _scale(name, s_plain):
    """a scale with blocks on both sides of every loss's bend: a^2 = the median of the blocks' |e|^2"""
    return 0.0 if name == "trivial" else float(np.sqrt(np.median(s_plain)))


def _check_against_restatement(oracle, og, losses, cls, poses, sw, method, iw, plain, corrected, what):
    """K1's plain and corrected blocks against the oracle's plain blocks and the restated corrector on them.

    Plain blocks: EDGE_TOL, plus eps / cos^2 d per edge -- d asin(u) / d u is formed as cos d / sqrt(1 - sin^2 d) by kernel
    and oracle alike, so a bogus loop with cos^2 d ~ 1e-7 carries ~eps / cos^2 d in that entry (Huber used to scale it away,
    Trivial does not).  Whitened blocks: relative to the largest entry (Omega reaches 2.7e12 on INTEL).
    Corrected blocks: each side takes sqrt(rho') at its OWN |e|^2.  The two |e|^2 differ by the plain blocks' difference,
    which is small absolutely but not relatively on blocks with |e| ~ 1e-5 (odometry), and a loss whose bend sits there
    (a^2 = the median |e|^2) turns that into |J| |d sqrt(rho') / ds| |ds|: that first-order term (x2) is added per edge."""
    c0, r0, J0 = plain
    c, r, J = corrected
    if method == 2:
        oc0, or0, oJ0, _, _ = LR.evaluate_sc(oracle, og, losses, cls, poses, sw, 1.0, False)
        oc, orr, oJ, _, _ = LR.evaluate_sc(oracle, og, losses, cls, poses, sw, 1.0, True)
    else:
        oc0, or0, oJ0 = LR.evaluate(oracle, og, losses, cls, poses, method, False, iw)
        oc, orr, oJ = LR.evaluate(oracle, og, losses, cls, poses, method, True, iw)
    tol = 1e-10 * max(1.0, np.abs(oJ0).max()) if iw else EDGE_TOL
    dth = poses[og.ib, 2] - poses[og.ia, 2] - og.meas[:, 2]
    cond = (1e-15 / np.maximum(np.cos(dth) ** 2, 1e-300))[:, None]

    def check(got, ref, bound, label):
        excess = np.abs(got - ref) - bound
        k = np.unravel_index(np.argmax(excess), excess.shape)
        assert excess[k] <= 0.0, (what, label, "edge %d entry %d: got %r ref %r bound %r" % (k[0], k[1], got[k], ref[k], bound[k]))

    rel_cost = 1e-10 if iw else 1e-12
    assert c0 == pytest.approx(oc0, rel=rel_cost) and c == pytest.approx(oc, rel=rel_cost), what
    check(r0, or0, np.broadcast_to(tol + cond, r0.shape), "plain r")
    check(J0, oJ0, np.broadcast_to(tol + cond, J0.shape), "plain J")
    so, sg = (or0 * or0).sum(axis=1), (r0 * r0).sum(axis=1)

    def sens(sv):   # |d sqrt(rho') / ds|; 0 where rho' = 0 (beyond Tukey's bend)
        _, p1, p2 = LR.block_rho(losses, cls, sv)
        live = p1 > 0.0
        return np.where(live, np.abs(p2) / (2.0 * np.sqrt(np.where(live, p1, 1.0))), 0.0)

    # (taken on both sides: at a bend -- Huber's kink, Tukey's end -- the two |e|^2 may fall on different sides)
    prop = (2.0 * np.maximum(sens(so), sens(sg)) * np.abs(sg - so))[:, None]
    check(r, orr, tol + cond + prop * np.abs(or0), "corrected r")
    check(J, oJ, tol + cond + prop * np.abs(oJ0), "corrected J")


@pytest.mark.parametrize("method,iw", [(0, False), (1, False), (0, True), (1, True), (2, False)])
def test_edge_kernel_matches_restatement(pgo, oracle, method, iw):
    g = load(pgo, "INTEL", 50)
    og = oracle_graph(oracle, g)
    rng = np.random.default_rng(7)
    x0 = np.array(g.poses)
    x1 = x0 + 0.05 * rng.standard_normal(x0.shape)
    configs = [("one", 1, None), ("kind", 3, None), ("edge", 3, rng.integers(0, 3, g.n_edges).astype(np.uint8))]
    seen_sides = set()
    for poses in (x0, x1):
        sw = None
        if method == 2:
            sw = np.ones(g.n_edges)
            sw[og.kind != 0] = rng.uniform(0.3, 1.0, int((og.kind != 0).sum()))
            s_plain = (oracle.evaluate_sc(og, poses, sw, 1.0, 0.0, False)[1] ** 2).sum(axis=1)
        else:
            s_plain = (oracle.evaluate(og, poses, method, 0.5, 0.0, False, True, False, 1, iw)[1] ** 2).sum(axis=1)
        for i, name in enumerate(NAMES):
            for tag, n, ec in configs:
                names = [name] if n == 1 else [name, NAMES[(i + 2) % 6], NAMES[(i + 4) % 6]]
                losses = [(nm, _scale(nm, s_plain)) for nm in names]
                cls = LR.classes(og.kind, n, ec)
                for k, (nm, a) in enumerate(losses):
                    if nm in ("huber", "tukey") and (cls == k).any():
                        seen_sides.update((nm, bool(v)) for v in s_plain[cls == k] > a * a)
                s = pgo.Solver(g, pgo.Options(method=method, info_weighting=int(iw)), losses=[pgo.Loss(nm, a) for nm, a in losses],
                               edge_class=ec)
                if method == 2:   # the handle's switches: those of an LM iteration, set through a solve state
                    s.lm_begin()
                    s.lm_step(1)
                    sw = s.switches()
                # (a) the loss itself: the corrected blocks = sqrt(rho') x the kernel's own plain blocks (apply_loss = 0),
                #     the cost = 1/2 sum rho of their |e|^2 -- at both pose sets
                c, r, J = s.evaluate(poses, apply_loss=True)
                c0, r0, J0 = s.evaluate(poses, apply_loss=False)
                q0, q1, _ = LR.block_rho(losses, cls, (r0 * r0).sum(axis=1))
                sq = np.sqrt(q1)[:, None]
                prior = 0.5 * ((1.0 - sw[og.kind != 0]) ** 2).sum() if method == 2 else 0.0   # (the switch prior: no loss)
                assert c == c0 and c == pytest.approx(0.5 * q0.sum() + prior, rel=1e-13), (name, tag)
                # (relative to the plain entry: near Tukey's bend sqrt(rho') = v is tiny and only absolutely accurate)
                assert (np.abs(r - sq * r0) <= 1e-13 * np.abs(r0)).all() and (np.abs(J - sq * J0) <= 1e-13 * np.abs(J0)).all()
                c2, _, _ = s.evaluate(poses, want_r=False, want_J=False)   # the cost-only launch
                assert c2 == pytest.approx(c, rel=1e-14)
                # (b) against the restatement on the oracle's blocks, at the file poses
                if poses is x0:
                    _check_against_restatement(oracle, og, losses, cls, poses, sw, method, iw, (c0, r0, J0), (c, r, J),
                                               (name, tag))
                s.close()
    assert seen_sides >= {("huber", True), ("huber", False), ("tukey", True), ("tukey", False)}


# ------------------------------------------------------------------ 3. LM against the restatement
# (graph, outliers, METHOD, losses (name, a) per class, classes: None = by kind).  Scales chosen so that both regions of
# each loss occur on the trajectory: the INTEL / MIT loops start at |e|^2 up to ~10, the odometry blocks at ~1e-4.
LM_CASES = [("INTEL", 50, 0, [("cauchy", 0.1)]),
            ("INTEL", 50, 1, [("trivial", 0.0), ("softlone", 0.1)]),
            ("INTEL", 50, 2, [("cauchy", 0.1)]),
            ("MIT", 0, 0, [("arctan", 2.0)]),   # (converges by the function tolerance in 43 iterations; at 0.5 the 50-iteration
                                                  # cap stops a slow crawl whose end point moves by 1e-4 with rounding)
            ("M3500", 0, 0, [("trivial", 0.0), ("tukey", 1.0)])]


@pytest.mark.parametrize("name,n_out,method,losses,solver",
                         [c + (ls,) for c in LM_CASES for ls in ((1,) if c[0] == "M3500" else (0, 1))])
def test_lm_matches_restatement(pgo, oracle, name, n_out, method, losses, solver):
    """solver 0: the library's choice (the direct solve on INTEL / MIT), 1: PCG to 1e-12; M3500 is PCG only"""
    g = load(pgo, name, n_out)
    og = oracle_graph(oracle, g)
    cls = LR.classes(og.kind, len(losses))
    ref = LR.lm(oracle, og, losses, cls, method=method)
    opt = dict(method=method, pcg_max_iters=400000, linear_solver=solver)
    if solver == 1:
        opt["pcg_rtol"] = 1e-12
    s = pgo.Solver(g, pgo.Options(**opt), losses=[pgo.Loss(n, a) for n, a in losses])
    summ = s.solve()
    x = s.poses()
    assert summ.termination == ref.termination and summ.iterations == ref.iterations
    assert summ.initial_cost == pytest.approx(ref.initial_cost, rel=1e-12)
    assert summ.final_cost == pytest.approx(ref.final_cost, rel=1e-7)
    recs = s.iter_records()
    assert len(recs) == len(ref.records)
    for a, b in zip(recs, ref.records):
        assert a["step_ok"] == b["step_ok"]
        assert a["radius"] == pytest.approx(b["radius"], rel=1e-4)
        assert a["cost"] == pytest.approx(b["cost"], rel=1e-6)
    d_xy = np.abs(x[:, :2] - ref.poses[:, :2]).max()
    print(f"{name}+{n_out} m{method} {losses} solver {s.info().linear_solver} (fallbacks {s.info().direct_fallbacks}): "
          f"{summ.iterations} iterations, final cost {summ.final_cost:.9e}, max |d translation| {d_xy:.2e}")
    assert d_xy < 5e-6 and np.abs(x[:, 2] - ref.poses[:, 2]).max() < 1e-4
    if method == 2:
        assert np.abs(s.switches() - ref.switches).max() < 1e-6
    s.close()


# ------------------------------------------------------------------ 4. batched handle
def test_batch_with_per_kind_losses_equals_individual_solves(pgo):
    from test_gpu_parity import _layer_problems
    graphs = _layer_problems(pgo, 8)
    losses = [pgo.Loss("trivial"), pgo.Loss("cauchy", 0.3), pgo.Loss("tukey", 1.0)]
    opt = dict(method=0, max_iters=2, fixed_pose=0)   # (the layer managers' local_iters, as test_batch_handle_equals_individual_solves)
    b = pgo.Batch(graphs, pgo.Options(**opt), losses=losses)
    s_b = b.solve()
    worst = 0.0
    for k, g in enumerate(graphs):
        s = pgo.Solver(g, pgo.Options(linear_solver=1, **opt), losses=losses)
        sa = s.solve()
        assert sa.iterations == s_b[k].iterations and sa.termination == s_b[k].termination
        assert s_b[k].final_cost == pytest.approx(sa.final_cost, rel=1e-10)
        assert [r["step_ok"] for r in s.iter_records()] == [r["step_ok"] for r in b.iter_records(k)]
        worst = max(worst, np.abs(s.poses() - b.poses(k)).max())
        s.close()
    print(f"8 layer problems, losses by kind: worst pose difference batch vs own solve {worst:.2e}")
    assert worst < 2e-9, worst   # (measured 9.3e-10: the summation order differs, and Cauchy / Tukey are less convex than Huber)
    # the batch's classes follow the problems' edges concatenated; a class table that differs from the default changes it
    ec = np.concatenate([np.minimum(np.array(g.kind), 2) for g in graphs]).astype(np.uint8)
    b2 = pgo.Batch(graphs, pgo.Options(**opt), losses=losses, edge_class=ec)
    for k, x in enumerate(b2.solve()):
        assert x.final_cost == s_b[k].final_cost
    with pytest.raises(ValueError):
        b2.set_losses(losses, ec[:-1])
    b.close(), b2.close()


# ------------------------------------------------------------------ 5. sharded
def _run_sharded(world, cfg, tmp):
    out = os.path.join(str(tmp), "w%d" % world)
    os.makedirs(out, exist_ok=True)
    name = "pgo_loss_%d_%d" % (os.getpid(), world)
    worker = os.path.join(ROOT, "tests", "_loss_shard_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, json.dumps(dict(cfg, rank=r, world=world, name=name, out=out))],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    if any(p.returncode != 0 for p in procs):
        raise AssertionError("\n".join("rank %d exit %s:\n%s" % (r, p.returncode, logs[r][-3000:]) for r, p in enumerate(procs)))
    res = [json.load(open(os.path.join(out, "out_%d.json" % r))) for r in range(world)]
    return res, [np.load(os.path.join(out, "poses_%d.npy" % r)) for r in range(world)]


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_per_edge_classes_match_one_rank(tmp_path, world):
    """every rank maps the caller-order classes onto its local edges: the one-rank history and PCG counts (the
    configuration of test_gpu_sharded_coarse: PCG with the same ordering and preconditioner levels at every world size)"""
    cfg = dict(graph="INTEL", outliers=50, losses=[["huber", 0.05], ["cauchy", 0.2], ["tukey", 0.5]],
               options=dict(method=1, max_iters=5, linear_solver=1, pcg_rtol=1e-11, pcg_max_iters=400000,
                            pcg_coarse_poses=16, pose_ordering=1))
    ref, ref_poses = _run_sharded(1, cfg, tmp_path)
    res, poses = _run_sharded(world, cfg, tmp_path)
    for r in range(world):
        np.testing.assert_array_equal(poses[r], poses[0])
        assert res[r]["cost0"] == pytest.approx(ref[0]["cost0"], rel=1e-12)
        assert [x["pcg_iters"] for x in res[r]["records"]] == [x["pcg_iters"] for x in res[0]["records"]]
    for a, b in zip(res[0]["records"], ref[0]["records"]):
        assert a["step_ok"] == b["step_ok"] and a["cost"] == pytest.approx(b["cost"], rel=1e-9)
        assert abs(a["pcg_iters"] - b["pcg_iters"]) <= 1
    d = np.abs(poses[0] - ref_poses[0]).max()
    print(f"world {world}: PCG {[x['pcg_iters'] for x in res[0]['records']]} (one rank {[x['pcg_iters'] for x in ref[0]['records']]}), "
          f"max |d pose| {d:.2e}")
    assert d < 1e-10   # (measured 2.7e-12 / 6.9e-12 at 2 / 3 ranks)


# ------------------------------------------------------------------ 6. covariances
def test_covariance_after_cauchy_solve_matches_sparse_lu(pgo, oracle):
    g = load(pgo, "INTEL")
    og = oracle_graph(oracle, g)
    losses = [("cauchy", 0.05)]
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=20), losses=pgo.Loss("cauchy", 0.05))
    s.solve()
    idx = np.concatenate([[0], np.unique(np.linspace(1, g.n_poses - 1, 23).astype(np.int64))])
    got, rep = s.covariance(idx)
    ref = LR.covariance_blocks(oracle, og, losses, LR.classes(og.kind, 1), s.poses(), idx, method=1)
    err = max(np.linalg.norm(a - b) / np.linalg.norm(b) for a, b in zip(got[1:], ref[1:]))
    assert np.all(got[0] == 0.0) and err < 1e-7, err
    s.close()


# ------------------------------------------------------------------ 7. rules and errors
def test_stale_solve_rule_and_errors(pgo):
    import ctypes
    g = load(pgo, "INTEL", 50)
    s = pgo.Solver(g, pgo.Options(method=1, max_iters=5))
    s.lm_begin()
    s.lm_step(1)
    s.set_losses(pgo.Loss("cauchy", 0.1))
    with pytest.raises(pgo.PgoError) as e:
        s.lm_step(1)                                    # the solve begun before the change is stale
    assert e.value.status == -1
    s.set_poses(np.array(g.poses))                      # (pgo_lm_begin starts from the handle's current poses)
    s.lm_begin()
    s.lm_step(2)
    t = pgo.Solver(g, pgo.Options(method=1, max_iters=5), losses=pgo.Loss("cauchy", 0.1))
    t.lm_begin()
    t.lm_step(2)
    np.testing.assert_array_equal(s.poses(), t.poses())
    # pgo_solve always starts anew with the current losses
    s.set_losses([pgo.Loss("trivial"), pgo.Loss("tukey", 0.4)])
    s.solve()
    L = pgo.lib()
    ok = (pgo.Loss * 4)(*[pgo.Loss("huber", 0.1)] * 4)
    cls = np.zeros(g.n_edges, np.uint8)
    bp = cls.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    for bad in (pgo.Loss("cauchy", 0.0), pgo.Loss("softlone", -1.0), pgo.Loss("tukey", float("nan")),
                pgo.Loss("arctan", float("inf"))):
        assert L.pgo_set_losses(s._h, 1, ctypes.byref(bad), None) == -1
    unknown = pgo.Loss("cauchy", 1.0)
    unknown.type = 6
    assert L.pgo_set_losses(s._h, 1, ctypes.byref(unknown), None) == -1
    unknown.type = -1
    assert L.pgo_set_losses(s._h, 1, ctypes.byref(unknown), None) == -1
    assert L.pgo_set_losses(s._h, 0, ok, None) == -1 and L.pgo_set_losses(s._h, 5, ok, None) == -1
    assert L.pgo_set_losses(s._h, 1, None, None) == -1 and L.pgo_set_losses(None, 1, ok, None) == -1
    cls[17] = 2
    assert L.pgo_set_losses(s._h, 2, ok, bp) == -1      # a class index >= n_classes
    assert L.pgo_set_losses(s._h, 3, ok, bp) == 0
    nan_trivial = pgo.Loss("trivial", float("nan"))      # Trivial ignores its scale
    assert L.pgo_set_losses(s._h, 1, ctypes.byref(nan_trivial), None) == 0
    with pytest.raises(ValueError):
        s.set_losses(pgo.Loss("cauchy", 1.0), np.zeros(3))
    # a refused call leaves the losses as they were
    s.set_losses(pgo.Loss("cauchy", 0.1))
    c1 = s.evaluate(want_r=False, want_J=False)[0]
    assert L.pgo_set_losses(s._h, 1, ctypes.byref(pgo.Loss("tukey", -2.0)), None) == -1
    assert s.evaluate(want_r=False, want_J=False)[0] == c1
    s.close(), t.close()


# ------------------------------------------------------------------ 8. drop-in surface
def test_cpp_mirror_with_cauchy_on_loops(pgo, tmp_path):
    """pgo::CauchyLoss on the loop blocks, NULL on the odometry blocks (two classes) through the C++ mirror = the Python solve"""
    exe = str(tmp_path / "loss_mirror_main")
    pkg = os.path.join(ROOT, "toy-robust-backend-slam_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host"),
                           os.path.join(ROOT, "tests", "native", "loss_mirror_main.cpp"), "-o", exe, "-L" + pkg, "-lpgo",
                           "-Wl,-rpath," + pkg])
    out = str(tmp_path / "poses.txt")
    p = subprocess.run([exe, os.path.join(DATA, "INTEL.g2o"), out, "0.1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "loss mirror ok" in p.stdout
    rho = pgo.Loss("cauchy", 0.1).evaluate(4.0)
    assert ("%.17g %.17g %.17g" % tuple(rho)) in p.stdout
    g = load(pgo, "INTEL", 50)
    s = pgo.Solver(g, pgo.Options(method=1), losses=[pgo.Loss("trivial"), pgo.Loss("cauchy", 0.1)])
    s.solve()
    got = np.loadtxt(out)
    assert np.abs(got - s.poses()).max() < 1e-9
    s.close()


def test_cli_loss_flag(pgo, tmp_path):
    from importlib import import_module
    exe = import_module("toy_robust_backend_slam_amd._build").build_cli()
    save = str(tmp_path / "save")
    p = subprocess.run([exe, "INTEL", "50", "0", "--loss", "cauchy:0.1", "--seed", "1", "--data", DATA, "--save", save,
                        "--precision", "17"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    g = load(pgo, "INTEL", 50)
    s = pgo.Solver(g, pgo.Options(method=0), losses=pgo.Loss("cauchy", 0.1))
    s.solve()
    got = np.loadtxt(os.path.join(save, "opt_nodes.txt"))
    assert np.abs(got[:, 1:] - s.poses()).max() < 1e-9
    s.close()
    # --loop-loss overrides the loss on closure and bogus blocks
    save2 = str(tmp_path / "save2")
    p = subprocess.run([exe, "INTEL", "50", "0", "--loss", "trivial", "--loop-loss", "tukey:0.5", "--seed", "1", "--data", DATA,
                        "--save", save2, "--precision", "17"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    s = pgo.Solver(g, pgo.Options(method=0), losses=[pgo.Loss("trivial"), pgo.Loss("tukey", 0.5)])
    s.set_poses(np.loadtxt(os.path.join(save, "init_nodes.txt"))[:, 1:])
    s.solve()
    assert np.abs(np.loadtxt(os.path.join(save2, "opt_nodes.txt"))[:, 1:] - s.poses()).max() < 1e-9
    s.close()
    assert subprocess.run([exe, "INTEL", "0", "0", "--loss", "welsch:1"], capture_output=True).returncode != 0
