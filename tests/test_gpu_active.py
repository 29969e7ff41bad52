"""pgo_set_active / pgo_batch_set_active on the GPU: edge subsets (layers) and pose windows solved on a live handle.

Yardsticks: the CPU oracle (oracle.evaluate / lm_direct) on the EXTRACTED problem -- the active edges and the used poses
renumbered 0..n-1 in order, fixed_pose = the anchor's new index -- and the existing product on the extracted graph or on
the unmasked graph.  The masked handle is never compared with itself.  Input: INTEL + 50 bogus loops, seed 1."""
import os
import subprocess

import numpy as np
import pytest

import _active_cases as AC
from conftest import DATA, ROOT, oracle_graph

pytestmark = pytest.mark.gpu

TIGHT = dict(pcg_rtol=1e-12, pcg_max_iters=400000)      # PCG standing in for an exact solve, as the parity tests run it


@pytest.fixture(scope="module")
def case(pgo):
    g = AC.intel(pgo)
    a = AC.arrays(g)
    n, E = len(a["poses"]), len(a["ia"])
    lm = AC.layer_mask(a["kind"])
    wm, wpc, wanchor = AC.window_masks(a)
    assert lm.sum() == 1363 and wm.sum() == 21 and wanchor == 39
    pc4 = np.zeros(n, bool)
    pc4[[5, 64, 600, 1227]] = True
    blk = np.ones(E, bool)
    blk[256:512] = False
    last = np.zeros(E, bool)
    last[E - 1] = True
    masks = {"layer": (lm, None, 0), "window": (wm, wpc, wanchor), "layer+4": (lm, pc4, 0), "block256": (blk, None, 0),
             "last": (last, None, -1)}
    return dict(g=g, a=a, n=n, E=E, masks=masks, cache={})


def _const(case, name, fixed=0):
    m, pc, _ = case["masks"][name]
    return AC.plan(case["n"], case["a"]["ia"], case["a"]["ib"], m, pc, fixed)[0].astype(bool)


def _sparse_J(J, ia, ib, n):
    import scipy.sparse as sp
    E = len(ia)
    rows = np.repeat(np.arange(3 * E).reshape(E, 3), 6, axis=1).reshape(-1)
    cols = np.concatenate([3 * ia[:, None] + np.arange(3), 3 * ib[:, None] + np.arange(3)], axis=1)
    cols = np.tile(cols, (1, 3)).reshape(-1)
    return sp.csr_matrix((J.reshape(-1), (rows, cols)), shape=(3 * E, 3 * n)).tocsc()


# ---------------------------------------------------------------------------------------------------- 1. evaluation
@pytest.mark.parametrize("name", ["layer", "window", "block256", "last"])
@pytest.mark.parametrize("iw", [0, 1])
@pytest.mark.parametrize("method", [0, 1])
def test_evaluation(pgo, oracle, case, method, iw, name):
    m, pc, anchor = case["masks"][name]
    gx, _, _ = AC.extract(pgo, case["a"], m, max(anchor, 0))
    ogx = oracle_graph(oracle, gx)
    s = pgo.Solver(case["g"], pgo.Options(method=method, info_weighting=iw))
    for apply_loss in (True, False):
        c0, r0, J0 = s.evaluate(apply_loss=apply_loss)
        s.set_active(m, pc)
        c, r, J = s.evaluate(apply_loss=apply_loss)
        assert np.all(r[~m] == 0) and np.all(J[~m] == 0)
        dr, dJ = np.abs(r[m] - r0[m]).max(), np.abs(J[m] - J0[m]).max()
        bitwise = np.array_equal(r[m], r0[m]) and np.array_equal(J[m], J0[m])
        oc = oracle.evaluate(ogx, method=method, apply_loss=apply_loss, want_r=False, want_J=False, info_weighting=bool(iw))[0]
        print(f"{name} M{method} info {iw} loss {apply_loss}: active rows bitwise equal {bitwise} (|dr| {dr:.1e}, |dJ| {dJ:.1e}); "
              f"cost {c!r} vs oracle {oc!r}")
        assert dr < 1e-11 and dJ < 1e-11
        assert c == pytest.approx(oc, rel=1e-12)      # (with pytest's absolute floor of 1e-12, as test_edge_kernel_parity)
        c1 = s.evaluate(apply_loss=apply_loss, want_r=False, want_J=False)[0]     # the cost-only instantiation
        assert c1 == c
        s.set_active()
        assert s.evaluate(apply_loss=apply_loss, want_r=False, want_J=False)[0] == c0
    s.close()


# ---------------------------------------------------------------------------------- 2. a non-finite inactive edge
def test_nonfinite_inactive_edge(pgo):
    poses = np.array([[0, 0, 0], [1, 0, 0], [2, 0, np.pi / 2]])
    g = pgo.Graph.from_arrays(poses, [0, 1, 0], [1, 2, 2], [[1, 0, 0], [1, 0, 0], [2, 0, 0]], [0, 0, 1])
    for method in (0, 1):
        s = pgo.Solver(g, pgo.Options(method=method))
        with pytest.raises(pgo.PgoError) as e:          # the premise: sin(delta) = 1.0 exactly, d asin is +-inf
            s.evaluate()
        assert e.value.status == -7
        s.set_active([1, 0, 0])
        c, r, J = s.evaluate()
        assert np.isfinite(c) and np.isfinite(r).all() and np.isfinite(J).all()
        assert np.all(r[1:] == 0) and np.all(J[1:] == 0)
        summ = s.solve()                                 # (raises on a non-zero status)
        assert summ.termination in (1, 2, 3, 4) and np.isfinite(summ.final_cost)
        x = s.poses()
        assert x[2].tobytes() == poses[2].tobytes() and x[0].tobytes() == poses[0].tobytes()
        i = s.info()
        assert (i.n_active_edges, i.n_constant_poses) == (1, 2)
        s.close()


# ------------------------------------------------------------------------------------------------------ 3. operators
VARIANTS = {"auto": {}, "block32": dict(linear_solver=1, pcg_block_poses=32), "chain64": dict(linear_solver=1, pcg_chain_len=64),
            "coarse16": dict(linear_solver=1, pcg_coarse_poses=16)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["layer", "window", "layer+4"])
@pytest.mark.parametrize("method", [0, 1])
def test_operators(pgo, case, method, name, variant):
    a, n = case["a"], case["n"]
    m, pc, _ = case["masks"][name]
    const = _const(case, name)
    free3 = np.repeat(~const, 3)
    ref_h = pgo.Solver(case["g"], pgo.Options(method=method))            # the unmasked product: J, and the fixed pose's row

    def system(x):
        """sparse J of the active problem at x with the constant columns zeroed, and r"""
        _, r, J = ref_h.evaluate(x)
        r, J = r.copy(), J.copy()
        r[~m] = 0
        J[~m] = 0
        import scipy.sparse as sp
        return _sparse_J(J, a["ia"], a["ib"], n) @ sp.diags(free3.astype(float)), r.reshape(-1)

    s = pgo.Solver(case["g"], pgo.Options(method=method, max_iters=2, **VARIANTS[variant]))
    s.set_active(m, pc)
    # normal equations at the file poses
    Jc, r = system(a["poses"])
    grad, hd = s.normal_eq()
    H = (Jc.T @ Jc).tocsr()
    g_ref = Jc.T @ r
    hd_ref = np.stack([H[3 * i:3 * i + 3, 3 * i:3 * i + 3].toarray().reshape(-1) for i in range(n)])
    assert np.abs(grad - g_ref).max() < 1e-11 * max(1.0, np.abs(g_ref).max())
    assert np.abs(hd - hd_ref).max() < 1e-11 * max(1.0, np.abs(hd_ref).max())
    assert np.all(grad[~free3] == 0) and np.all(hd[const] == 0)
    # one LM iteration, then the product kernel's (H + D'D) x against the dense restatement at the handle's poses
    scale = 1.0 / (1.0 + np.sqrt(np.asarray(Jc.multiply(Jc).sum(axis=0)).reshape(-1)))
    scale[~free3] = 0.0
    s.lm_begin()
    s.lm_step(1)
    rng = np.random.default_rng(5)
    x = rng.standard_normal(3 * n)
    y, d2 = s.system_spmv(x, want_d2=True)
    import scipy.sparse as sp
    J1, _ = system(s.poses())
    Js = J1 @ sp.diags(scale)
    y_ref = Js.T @ (Js @ x) + d2 * x
    assert np.abs(y - y_ref).max() < 1e-11 * max(1.0, np.abs(y_ref).max())
    # constant rows: what the row of opt.fixed_pose is on an unmasked handle -- identity LM row, nothing else
    ref_h.lm_begin()
    ref_h.lm_step(1)
    y0, d20 = ref_h.system_spmv(x, want_d2=True)
    assert np.all(d20[:3] == 1.0) and np.array_equal(y0[:3], x[:3])
    assert np.all(d2[~free3] == 1.0) and np.array_equal(y[~free3], x[~free3])
    # the preconditioner the next LM iteration applies
    u, v = rng.standard_normal(3 * n), rng.standard_normal(3 * n)
    Mu, Mv = s.precond(u), s.precond(v)
    assert np.isfinite(Mu).all() and np.isfinite(Mv).all()
    ab, ba = float(u @ Mv), float(v @ Mu)
    assert ab == pytest.approx(ba, rel=1e-10, abs=1e-10 * np.sqrt(float(u @ Mu) * float(v @ Mv)))
    assert float(u @ Mu) > 0.0 and float(v @ Mv) > 0.0
    np.testing.assert_allclose(s.precond(2.0 * u - 3.0 * v), 2.0 * Mu - 3.0 * Mv, rtol=1e-9, atol=1e-9 * np.abs(Mu).max())
    np.testing.assert_allclose(Mu[~free3], u[~free3], rtol=1e-12)
    e = np.where(free3, 0.0, u)                              # constant rows only: they stay decoupled
    z = s.precond(e)
    np.testing.assert_allclose(z[~free3], e[~free3], rtol=1e-12)
    assert np.abs(z[free3]).max() == 0.0
    s.lm_step(1)
    i = s.info()
    if variant == "coarse16":
        assert i.pcg_coarse_poses == 16 and i.pcg_coarse_off_iters == 0
    s.close()
    ref_h.close()


# ------------------------------------------------------------------------------------------------------ 4. LM parity
def _oracle_lm(pgo, oracle, case, name, method, max_iters):
    key = (name, method, max_iters)
    if key not in case["cache"]:
        m, pc, anchor = case["masks"][name]
        gx, used, fx = AC.extract(pgo, case["a"], m, anchor)
        res = oracle.lm_direct(oracle_graph(oracle, gx), oracle.Options(method=method, max_iters=max_iters, fixed_pose=fx))
        sx = pgo.Solver(gx, pgo.Options(method=method, max_iters=max_iters, fixed_pose=fx))
        sx.solve()
        case["cache"][key] = (res, used, sx.poses())
        sx.close()
    return case["cache"][key]


LM_VARIANTS = {"auto": {}, "pcg": dict(linear_solver=1, **TIGHT), "pcg-chain64": dict(linear_solver=1, pcg_chain_len=64, **TIGHT),
               "pcg-coarse16": dict(linear_solver=1, pcg_coarse_poses=16, **TIGHT)}


@pytest.mark.parametrize("variant", list(LM_VARIANTS))
@pytest.mark.parametrize("name,max_iters", [("layer", 6), ("window", 3)])
@pytest.mark.parametrize("method", [0, 1])
def test_lm_parity(pgo, oracle, case, method, name, max_iters, variant):
    m, pc, _ = case["masks"][name]
    res, used, x_product = _oracle_lm(pgo, oracle, case, name, method, max_iters)
    if name == "layer":      # the premise, as checked with the oracle when the cases were chosen
        assert res.initial_cost == pytest.approx((17.917999727, 1.317409184)[method], rel=1e-9)
        assert [r["step_ok"] for r in res.records] == [1] * 7 and res.iterations == 6
    else:
        assert res.iterations == 3 and res.termination == 4
        if method == 0:
            assert res.initial_cost == pytest.approx(0.019520974, rel=1e-7)
    s = pgo.Solver(case["g"], pgo.Options(method=method, max_iters=max_iters, **LM_VARIANTS[variant]))
    s.set_active(m, pc)
    summ = s.solve()
    recs = s.iter_records()
    x = s.poses()
    const = _const(case, name)
    d_oracle = np.abs(x[used] - res.poses).max()
    d_product = np.abs(x[used] - x_product).max()
    print(f"{name} M{method} {variant}: final cost {summ.final_cost!r} vs oracle {res.final_cost!r}; max |d pose| vs oracle "
          f"{d_oracle:.2e}, vs the product's solve of the extracted graph {d_product:.2e}; PCG iterations {summ.total_pcg_iters}")
    assert [r["step_ok"] for r in recs] == [r["step_ok"] for r in res.records]
    assert summ.termination == res.termination and summ.iterations == res.iterations
    assert summ.initial_cost == pytest.approx(res.initial_cost, rel=1e-12)
    assert summ.final_cost == pytest.approx(res.final_cost, rel=1e-7)
    assert d_oracle < 1e-6
    assert x[const].tobytes() == case["a"]["poses"][const].tobytes()
    i = s.info()
    assert i.pcg_coarse_off_iters == 0
    if variant == "pcg-coarse16":
        assert i.pcg_coarse_poses == 16
    s.close()


@pytest.mark.parametrize("k", [0, 700])
def test_single_constant_pose_equals_fixed_pose(pgo, case, k):
    kw = dict(method=1, max_iters=4, linear_solver=1, **TIGHT)
    a = pgo.Solver(case["g"], pgo.Options(fixed_pose=-1, **kw))
    pc = np.zeros(case["n"], bool)
    pc[k] = True
    a.set_active(None, pc)
    sa = a.solve()
    b = pgo.Solver(case["g"], pgo.Options(fixed_pose=k, **kw))
    sb = b.solve()
    d = np.abs(a.poses() - b.poses()).max()
    print(f"pose_constant = {{{k}}} vs fixed_pose = {k}: max |d pose| {d:.2e}")
    assert [r["step_ok"] for r in a.iter_records()] == [r["step_ok"] for r in b.iter_records()]
    assert sa.final_cost == pytest.approx(sb.final_cost, rel=1e-9) and d < 1e-9
    assert a.poses()[k].tobytes() == case["a"]["poses"][k].tobytes()
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------- 5. direct solve gating
def test_direct_solve_gating(pgo, case):
    lm, _, _ = case["masks"]["layer"]
    wm, wpc, _ = case["masks"]["window"]
    o = dict(method=1, max_iters=6)
    s = pgo.Solver(case["g"], pgo.Options(**o))
    assert s.info().linear_solver == 2
    s.set_active(lm)
    assert s.info().linear_solver == 2            # every chain edge is active: the inactive loops are zero columns
    sd = s.solve()
    assert sd.total_pcg_iters == 0 and s.info().direct_fallbacks == 0
    p = pgo.Solver(case["g"], pgo.Options(linear_solver=1, **TIGHT, **o))
    p.set_active(lm)
    sp_ = p.solve()
    d = np.abs(s.poses() - p.poses()).max()
    print(f"layer mask: direct vs PCG(1e-12) max |d pose| {d:.2e}")
    assert [r["step_ok"] for r in s.iter_records()] == [r["step_ok"] for r in p.iter_records()]
    assert d < 1e-7 and sd.final_cost == pytest.approx(sp_.final_cost, rel=1e-9)
    s.set_active(wm, wpc)
    assert s.info().linear_solver == 1            # the window cuts the chain: PCG
    sw = s.solve()
    assert sw.total_pcg_iters > 0
    s.set_active(None, None)
    assert s.info().linear_solver == 2
    s.set_poses(case["a"]["poses"])
    s1 = s.solve()
    f = pgo.Solver(case["g"], pgo.Options(**o))
    s2 = f.solve()
    assert s.poses().tobytes() == f.poses().tobytes() and s1.final_cost == s2.final_cost      # bitwise a fresh handle's
    assert [r["cost"] for r in s.iter_records()] == [r["cost"] for r in f.iter_records()]
    for h in (s, p, f):
        h.close()


# --------------------------------------------------------------------------------------------- 6. life cycle and errors
def test_life_cycle_and_errors(pgo, case):
    lm, _, _ = case["masks"]["layer"]
    wm, wpc, _ = case["masks"]["window"]
    a = case["a"]
    s = pgo.Solver(case["g"], pgo.Options(method=1, max_iters=4))
    s.lm_begin()
    s.set_active(lm)
    with pytest.raises(pgo.PgoError) as e:
        s.lm_step(1)
    assert e.value.status == -1
    s.lm_begin()
    done, summ = s.lm_step(1)
    assert summ.iterations == 1
    for m, pc in ((lm, None), (wm, wpc), (None, None), (None, wpc)):
        s.set_active(m, pc)
        const, n_act, n_free = pgo.active_plan(case["n"], a["ia"], a["ib"], m, pc, 0)
        i = s.info()
        assert (i.n_active_edges, i.n_constant_poses) == (n_act, case["n"] - n_free) == (n_act, int(const.sum()))
    assert pgo.lib().pgo_set_active(None, None, None) == -1
    assert pgo.lib().pgo_batch_set_active(None, None, None) == -1
    s.close()
    # METHOD 2: refused, and the handle solves as a handle that was never asked
    o2 = pgo.Options(method=2, max_iters=3)
    s2, f2 = pgo.Solver(case["g"], o2), pgo.Solver(case["g"], o2)
    with pytest.raises(pgo.PgoError) as e:
        s2.set_active(lm)
    assert e.value.status == -8
    assert s2.info().n_active_edges == case["E"]
    assert s2.solve().final_cost == f2.solve().final_cost and s2.poses().tobytes() == f2.poses().tobytes()
    s2.close(); f2.close()
    # alternating masks do not allocate: a two-level PCG handle (the dead-aggregate list follows the masks)
    s3 = pgo.Solver(case["g"], pgo.Options(method=1, max_iters=2, linear_solver=1))
    assert s3.info().pcg_coarse_poses > 0
    s3.set_active(lm)
    s3.set_active(wm, wpc)
    bytes0 = s3.info().device_bytes      # baseline AFTER one call with each mask: the mask buffer and the full-size dead list
                                         # are allocated once, at the first call that needs them; nothing may follow
    for k in range(200):
        s3.set_active(*((lm, None) if k % 2 else (wm, wpc)))
    assert s3.info().device_bytes == bytes0
    assert s3.solve().iterations == 2 and s3.info().pcg_coarse_off_iters == 0
    s3.close()


# ------------------------------------------------------------------------------------------------------ 7. covariance
def test_covariance(pgo, case):
    from test_gpu_covariance import BLOCK_REL, block_errors
    lm, _, _ = case["masks"]["layer"]
    wm, wpc, _ = case["masks"]["window"]
    idx = np.array([1, 600, 1227])
    s = pgo.Solver(case["g"], pgo.Options(method=1, max_iters=5))
    s.set_active(lm)
    s.solve()
    got, rep = s.covariance(idx)
    gx, used, fx = AC.extract(pgo, case["a"], lm, 0)
    assert len(used) == case["n"] and fx == 0            # every pose is used: same numbering
    x = pgo.Solver(gx, pgo.Options(method=1, max_iters=5))
    x.set_poses(s.poses())
    ref, _ = x.covariance(idx)
    err = block_errors(got, ref)
    print(f"layer mask: covariance blocks vs the extracted graph's handle, relative errors {err}")
    assert err.max() <= BLOCK_REL
    s.set_active(wm, wpc)
    s.set_poses(case["a"]["poses"])
    s.solve()
    got, rep = s.covariance([100, 39, 189])
    assert np.array_equal(got[0], np.zeros((3, 3))) and np.array_equal(got[1], np.zeros((3, 3)))
    assert np.isfinite(got[2]).all() and np.array_equal(got[2], got[2].T) and np.linalg.eigvalsh(got[2]).min() > 0
    s.close(); x.close()


# ----------------------------------------------------------------------------------------------------------- 8. batch
def _round_masks(a, seeds):
    """4 layer masks and 4 windows (radius 30 around one of the layer's loops, as the layer managers cut them): per problem
    (edge mask, pose_constant mask)"""
    n, ia, ib, kind = len(a["poses"]), a["ia"], a["ib"], a["kind"]
    loops = np.nonzero(kind != 0)[0]
    out = []
    for j, seed in enumerate(seeds):
        keep = AC.layer_mask(kind, seed)
        pc = np.zeros(n, bool)
        if j >= 4:
            mine = loops[keep[loops]]
            e = mine[seed % len(mine)]
            lo, hi = max(0, min(ia[e], ib[e]) - 30), min(n - 1, max(ia[e], ib[e]) + 30)
            keep = keep & (ia >= lo) & (ia <= hi) & (ib >= lo) & (ib <= hi)
            pc[min(ia[keep].min(), ib[keep].min())] = True           # anchor = the smallest used pose
        out.append((keep, pc))
    return out


def test_batch(pgo, case):
    a, g = case["a"], case["g"]
    opt = dict(method=0, max_iters=2)
    b = pgo.Batch([g] * 8, pgo.Options(**opt))
    for seeds in (range(0, 8), range(4, 12)):
        masks = _round_masks(a, list(seeds))
        for k in range(8):
            b.set_poses(k, a["poses"])
        b.set_active([m for m, _ in masks], [pc for _, pc in masks])
        sb = b.solve()
        worst = 0.0
        for k, (m, pc) in enumerate(masks):
            s = pgo.Solver(g, pgo.Options(linear_solver=1, **opt))
            s.set_active(m, pc)
            ss = s.solve()
            assert [r["step_ok"] for r in s.iter_records()] == [r["step_ok"] for r in b.iter_records(k)], k
            assert (ss.iterations, ss.termination) == (sb[k].iterations, sb[k].termination)
            assert sb[k].initial_cost == pytest.approx(ss.initial_cost, rel=1e-12)
            assert sb[k].final_cost == pytest.approx(ss.final_cost, rel=1e-10)
            d = np.abs(s.poses() - b.poses(k)).max()
            worst = max(worst, d)
            assert d < 1e-9, (k, d)
            const = AC.plan(case["n"], a["ia"], a["ib"], m, pc, 0)[0].astype(bool)
            assert b.poses(k)[const].tobytes() == a["poses"][const].tobytes()
            s.close()
        print(f"batch of 8 masked problems (seeds {list(seeds)}): max |d pose| vs the masked solo handles {worst:.2e}")
    b.close()


def _loss_graph(pgo):
    """the 3-pose graph of test 2: the loop 0-2 sits at sin(delta) = 1.0"""
    poses = np.array([[0, 0, 0], [1, 0, 0], [2, 0, np.pi / 2]])
    return poses, pgo.Graph.from_arrays(poses, [0, 1, 0], [1, 2, 2], [[1, 0, 0], [1, 0, 0], [2, 0, 0]], [0, 0, 1])


@pytest.mark.parametrize("method", [0, 1])
def test_set_losses_after_set_active_keeps_the_mask(pgo, oracle, case, method):
    """pgo_set_losses shares the flags byte with the edge mask: changing the losses of a masked handle must leave the
    problem's edge set alone.  Cost against the loss restatement (tests/_loss_restatement.py, the yardstick of
    test_gpu_loss.py, with its 1e-12 cost bound) on the EXTRACTED graph."""
    import _loss_restatement as LR
    lm, _, _ = case["masks"]["layer"]
    gx, _, _ = AC.extract(pgo, case["a"], lm, 0)
    ogx = oracle_graph(oracle, gx)
    losses = [("huber", 0.05), ("cauchy", 0.1), ("tukey", 1.5)]                # classes follow the edge kind
    cls_x = np.minimum(np.array(gx.kind), 2)
    s = pgo.Solver(case["g"], pgo.Options(method=method))
    f = pgo.Solver(case["g"], pgo.Options(method=method), losses=[pgo.Loss(n, a) for n, a in losses])   # unmasked, same losses
    s.set_active(lm)
    before = (s.info().n_active_edges, s.info().n_constant_poses)
    s.set_losses([pgo.Loss(n, a) for n, a in losses])
    assert (s.info().n_active_edges, s.info().n_constant_poses) == before == (1363, 1)
    for apply_loss in (True, False):
        c, r, J = s.evaluate(apply_loss=apply_loss)
        oc = LR.evaluate(oracle, ogx, losses, cls_x, None, method, apply_loss)[0]
        _, r0, J0 = f.evaluate(apply_loss=apply_loss)
        assert np.all(r[~lm] == 0) and np.all(J[~lm] == 0)
        print(f"M{method} loss {apply_loss}: masked cost with three loss classes {c!r} vs restatement on the extracted graph {oc!r}")
        assert c == pytest.approx(oc, rel=1e-12)
        assert np.abs(r[lm] - r0[lm]).max() < 1e-11 and np.abs(J[lm] - J0[lm]).max() < 1e-11   # the bound of test 1
    # ... and a non-finite inactive edge stays out after the losses change
    poses, g3 = _loss_graph(pgo)
    s3 = pgo.Solver(g3, pgo.Options(method=method))
    s3.set_active([1, 0, 0])
    s3.set_losses(pgo.Loss("cauchy", 0.1))
    c, r, J = s3.evaluate()
    assert np.isfinite(c) and np.isfinite(J).all() and np.all(J[1:] == 0)
    s3.solve()
    assert s3.poses()[2].tobytes() == poses[2].tobytes()
    s.close(); s3.close(); f.close()


def test_batch_set_losses_after_set_active_keeps_the_masks(pgo, oracle, case):
    import _loss_restatement as LR
    a, g = case["a"], case["g"]
    opt = dict(method=0, max_iters=2)
    losses = [("huber", 0.05), ("cauchy", 0.1)]                                # odometry / loops
    L = [pgo.Loss(n, al) for n, al in losses]
    masks = _round_masks(a, [0, 1, 2, 3, 4, 5, 6, 7])
    masks = [masks[0], masks[1], masks[4], masks[5]]                           # two layers, two windows
    b = pgo.Batch([g] * 4, pgo.Options(**opt))
    b.set_active([m for m, _ in masks], [pc for _, pc in masks])
    b.set_losses(L)                                                            # after the masks
    sb = b.solve()
    for k, (m, pc) in enumerate(masks):
        anchor = int(np.nonzero(pc)[0][0]) if pc.any() else 0
        gx, used, _ = AC.extract(pgo, a, m, anchor)
        oc = LR.evaluate(oracle, oracle_graph(oracle, gx), losses, np.minimum(np.array(gx.kind), 1), None, 0, True)[0]
        assert sb[k].initial_cost == pytest.approx(oc, rel=1e-12), k          # the masked problem's cost, not the full graph's
        s = pgo.Solver(g, pgo.Options(linear_solver=1, **opt), losses=L)       # losses first, then the mask
        s.set_active(m, pc)
        ss = s.solve()
        assert [r["step_ok"] for r in s.iter_records()] == [r["step_ok"] for r in b.iter_records(k)], k
        assert sb[k].final_cost == pytest.approx(ss.final_cost, rel=1e-10)
        d = np.abs(s.poses() - b.poses(k)).max()
        assert d < 1e-9, (k, d)
        const = AC.plan(case["n"], a["ia"], a["ib"], m, pc, 0)[0].astype(bool)
        assert b.poses(k)[const].tobytes() == a["poses"][const].tobytes()
        s.close()
    b.close()


@pytest.mark.parametrize("method", [0, 1])
def test_direct_solve_with_several_constant_poses(pgo, oracle, case, method):
    """linear_solver 2 with the layer mask and pose_constant = {5, 64, 600, 1227} on top of opt.fixed_pose, against the LM
    restatement with a sparse direct solve (AC.lm_direct_const: oracle.lm_direct's policy for any constant set, first
    checked to reproduce oracle.lm_direct for the single anchor), with the bounds of test_lm_parity"""
    m, pc, _ = case["masks"]["layer+4"]
    gx, used, fx = AC.extract(pgo, case["a"], m, 0)
    ogx = oracle_graph(oracle, gx)
    assert len(used) == case["n"]                                              # every pose is used: same numbering
    oo = oracle.Options(method=method, max_iters=6, fixed_pose=0)
    res = _oracle_lm(pgo, oracle, case, "layer", method, 6)[0]
    one = np.zeros(case["n"], bool)
    one[0] = True
    x1, t1, it1, c1, h1 = AC.lm_direct_const(oracle, ogx, oo, one)
    assert np.array_equal(x1, res.poses) and (t1, it1, c1) == (res.termination, res.iterations, res.final_cost)
    const = _const(case, "layer+4")
    xr, term, iters, cost, hist = AC.lm_direct_const(oracle, ogx, oo, const)
    s = pgo.Solver(case["g"], pgo.Options(method=method, max_iters=6))
    s.set_active(m, pc)
    assert s.info().linear_solver == 2 and s.info().n_constant_poses == 5
    summ = s.solve()
    x = s.poses()
    d = np.abs(x - xr).max()
    print(f"layer+4 M{method} direct solve: final cost {summ.final_cost!r} vs restatement {cost!r}; max |d pose| {d:.2e}")
    assert s.info().linear_solver == 2 and s.info().direct_fallbacks == 0 and summ.total_pcg_iters == 0
    assert [r["step_ok"] for r in s.iter_records()] == hist
    assert (summ.termination, summ.iterations) == (term, iters)
    assert summ.final_cost == pytest.approx(cost, rel=1e-7) and d < 1e-6
    assert x[const].tobytes() == case["a"]["poses"][const].tobytes()
    s.close()


# ----------------------------------------------------------------------------------------------------- 9. host mirror
def test_host_active_mirror(tmp_path):
    """pgo::Problem with several constant blocks and an unused block (tests/native/active_mirror_main.cpp)"""
    exe = str(tmp_path / "active_mirror_main")
    pkg = os.path.join(ROOT, "toy-robust-backend-slam_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host"),
                           os.path.join(ROOT, "tests", "native", "active_mirror_main.cpp"), "-o", exe, "-L" + pkg, "-lpgo",
                           "-Wl,-rpath," + pkg])
    p = subprocess.run([exe, os.path.join(DATA, "INTEL.g2o")], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "active mirror ok" in p.stdout
