"""CPU: the numpy restatement of METHOD 2's joint LM system (_switch_restatement.py) pinned against oracle.lm_direct_sc, on
every case of test_gpu_switch_system.py, before any GPU run relies on it.

The state after k LM iterations (k = 0 .. 8) is reached through lm_direct_sc(max_iters = k); from each state the restated
joint step must reproduce record k + 1 of the longer run -- step_norm, cost_change, relative_decrease to 1e-9 relative, step_ok,
and gradient_max_norm after it.  The reduced route (switches eliminated, pose solve, back-substitution) must give the joint
route's step; their difference delta_ref is printed.  The LMSystem identities H = JS'JS and b = JS'r~ hold to 1e-14 of the
largest entry (of H; for b, whose entries are cancelling sums, of |JS|'|r~| -- see there).  The graph conditions the GPU tests rely on are asserted here, on the oracle alone."""
import numpy as np
import pytest
import scipy.sparse as sp

import _switch_restatement as R
from test_gpu_switch_system import CASES, TILE_INC, build_case, restate_args, tile_rows

REL = 1e-9
STATES = 9      # k = 0 .. 8


def close(a, b):
    return abs(a - b) <= REL * max(abs(a), abs(b))


def options(O, c, k):
    o = c["opts"]
    return O.Options(method=2, max_iters=k, fixed_pose=c["fixed"], jacobi_scaling=o.get("jacobi_scaling", 1),
                     radius0=o.get("radius0", 1e4), min_lm_diagonal=o.get("min_lm_diagonal", 1e-6), threads=1)


@pytest.mark.parametrize("case", list(CASES))
def test_restated_joint_step_reproduces_the_oracle(oracle, case):
    O, c = oracle, CASES[case]
    ag, og = build_case(case, O)
    kw = restate_args(c)
    kw["threads"] = 1
    lam = kw["lam"]
    long_run = O.lm_direct_sc(og, options(O, c, STATES), lam)
    recs = long_run.records
    assert len(recs) == STATES + 1, (case, "the solve ended early", len(recs), long_run.termination)
    g0 = R.gradient(O, og, ag.poses, None, lam, c["fixed"])
    assert close(g0.gmax, recs[0]["gradient_max_norm"])
    worst = {}
    for k in range(STATES):
        res = O.lm_direct_sc(og, options(O, c, k), lam)
        assert res.records == recs[:k + 1], (case, k)
        radius = res.records[-1]["radius"]
        st = R.joint_step(O, og, res.poses, res.switches, ag.poses, radius, **kw)
        rec = recs[k + 1]
        assert st.valid and not st.term and rec["step_ok"] >= 0, (case, k, rec)
        assert st.kappa_joint <= 1e8, (case, k, st.kappa_joint)
        tol = R.step_tolerances(st, 1e-16, radius)
        assert abs(st.rho - 1e-3) > tol["rho"], (case, k, st.rho, tol["rho"])
        assert rec["step_ok"] == int(st.step_ok), (case, k, rec, st.rho)
        assert close(st.step_norm, rec["step_norm"]), (case, k, st.step_norm, rec["step_norm"])
        assert close(st.cost_change, rec["cost_change"]), (case, k, st.cost_change, rec["cost_change"])
        assert close(st.rho, rec["relative_decrease"]), (case, k, st.rho, rec["relative_decrease"])
        gmax = st.gmax if st.step_ok else R.gradient(O, og, res.poses, res.switches, lam, c["fixed"]).gmax
        assert close(gmax, rec["gradient_max_norm"]), (case, k, gmax, rec["gradient_max_norm"])
        if st.step_ok:
            assert close(R.accepted_radius(radius, st.rho), rec["radius"]), (case, k)
        # the reduced route is the joint route
        rel = {q: st.delta_ref[q] / max(abs(getattr(st, q)), 1e-300) for q in R.QUANTITIES}
        rel["vector"] = st.delta_ref["vector"] / max(1.0, st.step_norm)
        for q, v in rel.items():
            worst[q] = max(worst.get(q, 0.0), v)
            assert v <= REL, (case, k, q, v)
        worst["kappa"] = max(worst.get("kappa", 0.0), st.kappa)
        worst["kappa_joint"] = max(worst.get("kappa_joint", 0.0), st.kappa_joint)
        # the LMSystem identities
        S = st.S
        H, JS = S.sysm.H, S.sysm.JS
        assert JS.shape == (3 * og.n_edges, 3 * og.n_poses)
        assert abs(H - JS.T @ JS).max() <= 1e-14 * abs(H).max(), (case, k)
        # b: an entry is a sum of up to 3 x 301 products that cancel (hub's heavy row: summands of 1e-1, the largest entry of
        # b 8e-3), and the two sides sum them in different orders -- the rounding of such a sum scales with its summands, so
        # the largest entry is taken of |JS|'|r~|, the sums of the absolute products (>= |b| entrywise), not of b
        b_scale = (abs(JS).T @ np.abs(S.r_tilde)).max()
        assert np.abs(S.sysm.b - JS.T @ S.r_tilde).max() <= 1e-14 * b_scale, (case, k, b_scale, np.abs(S.sysm.b).max())
        f = c["fixed"]
        A = (H + sp.diags(S.sysm.d2)).toarray()
        eye = np.eye(3 * og.n_poses)[3 * f:3 * f + 3]
        assert np.array_equal(A[3 * f:3 * f + 3], eye) and np.array_equal(A[:, 3 * f:3 * f + 3], eye.T)
        assert not S.sysm.b[3 * f:3 * f + 3].any()
    pattern = "".join("1" if r["step_ok"] == 1 else "0" for r in recs)
    print("%s: step_ok %s, largest delta_ref (relative) %s, cond_2 reduced %.2e joint %.2e; switch / pose gradient at the start %.3e / %.3e" % (
        case, pattern, {q: "%.1e" % v for q, v in worst.items() if not q.startswith("kappa")}, worst["kappa"], worst["kappa_joint"],
        g0.switch_max, g0.pose_max))
    if case == "rejecting":
        assert "001" in pattern, pattern      # at least two rejections in a row, then an accepted step


def test_rejected_state_keeps_the_previous_elimination(oracle):
    """radius_elim touches the switch block alone: the pose part of D'D follows the current radius, and with radius_elim = radius
    the default comes back"""
    O, c = oracle, CASES["small"]
    ag, og = build_case("small", O)
    kw = restate_args(c)
    a = R.joint_system(O, og, ag.poses, None, ag.poses, 50.0, **kw)
    b = R.joint_system(O, og, ag.poses, None, ag.poses, 50.0, radius_elim=100.0, **kw)
    e = R.joint_system(O, og, ag.poses, None, ag.poses, 100.0, **kw)
    np.testing.assert_array_equal(a.sysm.d2, b.sysm.d2)
    np.testing.assert_array_equal(b.c, e.c)
    np.testing.assert_array_equal(b.gamma, e.gamma)
    assert abs(b.sysm.H - e.sysm.H).max() == 0.0 and abs(a.sysm.H - b.sysm.H).max() > 0.0
    # unscaled_reduced is the reduced system with unit pose scales: rescaled by s it is the LMSystem's
    g, hd = R.unscaled_reduced(O, og, ag.poses, None, ag.poses, 50.0, **kw)
    s = a.sysm.s
    np.testing.assert_allclose(s * g, a.sysm.b, rtol=0, atol=1e-14 * np.abs(g).max())
    Hd = a.sysm.H.toarray()
    for i in range(og.n_poses):
        blk = hd[i].reshape(3, 3) * np.outer(s[3 * i:3 * i + 3], s[3 * i:3 * i + 3])
        np.testing.assert_allclose(blk, Hd[3 * i:3 * i + 3, 3 * i:3 * i + 3], rtol=0, atol=1e-14 * np.abs(hd).max())


def test_case_conditions(oracle):
    """what the case table promises (the LM trajectories' conditions are asserted per case above)"""
    O = oracle
    for case, c in CASES.items():
        ag, _ = build_case(case, O)
        n, f = ag.n_poses, c["fixed"]
        sw = [(int(a), int(b), int(k)) for a, b, k in zip(ag.ia, ag.ib, ag.kind) if k != 0]
        assert np.array_equal(ag.ia[:n - 1], np.arange(n - 1)) and np.array_equal(ag.ib[:n - 1], np.arange(1, n)) and not ag.kind[:n - 1].any()
        assert any(a > b for a, b, _ in sw), case
        assert any(a == f for a, b, _ in sw) and any(b == f for a, b, _ in sw), case
        assert any(b == a + 1 for a, b, _ in sw) and any(b == a - 1 for a, b, _ in sw), case
        assert any((b, a, 3 - k) in sw for a, b, k in sw), case
        assert {k for _, _, k in sw} == {1, 2}, case
    ag, _ = build_case("hub", O)
    deg = np.bincount(np.concatenate([ag.ia, ag.ib]))
    assert deg[-1] == 301 and deg[-1] > TILE_INC and int((ag.kind[(ag.ia == 300) | (ag.ib == 300)] != 0).sum()) == 300
    assert tile_rows(ag.n_poses, ag.ia, ag.ib)[0][-1] == 1 and tile_rows(ag.n_poses, ag.ia, ag.ib)[1][-1] == 301
    ag, _ = build_case("tiles", O)
    rows, incs = tile_rows(ag.n_poses, ag.ia, ag.ib)
    assert rows == [85, 85, 22, 64, 1] and incs[0] == TILE_INC and incs[3] == TILE_INC, (rows, incs)
    assert all(3 * r <= TILE_INC for r in rows)     # (the padded-slot layout accepts every tile)
    sizes = {(c["n"], len(c["loops"])) for c in CASES.values()}
    assert (40, 12) in sizes and (60, 13) in sizes and (301, 300) in sizes
    start = {}     # case -> (largest switch gradient, largest pose gradient) at the start
    for case, c in CASES.items():
        ag, og = build_case(case, O)
        g0 = R.gradient(O, og, ag.poses, None, restate_args(c)["lam"], c["fixed"])
        start[case] = (g0.switch_max, g0.pose_max)
    assert any(s > p for s, p in start.values()) and any(s <= p for s, p in start.values()), start
