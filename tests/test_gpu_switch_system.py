"""METHOD 2's per-edge switch elimination (k_switch_prepare, k_assemble<true>, k_switch_backsub, the direct solve's c j j'
term) against the JOINT LM system over poses and switches, restated in numpy (_switch_restatement.py; pinned on the CPU by
test_switch_restatement.py against oracle.lm_direct_sc).

Cases (deterministic, seeded; CASES below): a walk with noisy odometry, initial poses by dead reckoning, kind 1 loops
measured from the truth, kind 2 edges with random measurements.  Every case carries a switchable edge with a > b, one on
the constant pose in each orientation, switchable edges between adjacent poses in both orientations (they share the block
slot (i, i - 1) with the odometry edge) and a duplicated loop pair whose copy is reversed and of the other kind.
  small      40 poses, 6 loops + 6 bogus; also with sc_prior_lambda 4.0 / 0.25, jacobi_scaling = 0, fixed_pose = N - 1, and with
             min_lm_diagonal = 0.3 at radius0 = 1 (the clamp of the LM diagonal acting on every h_ss)
  rejecting  60 poses, heading noise 1.5 rad, radius0 = 1e6: rejected steps and the refresh after them
  hub        301 poses, the last one with 300 switchable incidences: the heavy-row branch of k_assemble<true>, two chunks
  tiles      257 poses: row tiles of 85 rows, a tile of exactly 256 incidences, a last tile of one row
Handle variants, METHOD 2 throughout: "direct" (linear_solver = 2), "pcg" (linear_solver = 1, pcg_rtol 1e-13, no coarse level,
chain preconditioner of 8, knob verify_residual), "pcg-pad" (the same with knob pad_tiles), "pcg-order" (the same with
pose_ordering flipped from its default).

At the state after lm_begin() and after each lm_step(1):
  (a) all variants: system_spmv on every unit vector against the restated H + diag(d2), entrywise within PROD x max(1, largest
      entry); d2 to 1e-12 relative; the constant pose's rows and columns those of the identity.  After a rejected step the
      restatement takes radius_elim = the radius of the record before the rejection.
  (b) direct, pcg: the joint step restated from the handle's own poses, switches and radius; step_ok equal; step_norm, the
      model decrease (cost_change / relative_decrease), cost_change, relative_decrease, gradient_max_norm and radius within
      _switch_restatement.step_tolerances -- 10 x (the two restated routes' own difference + the first-order effect of a solve
      error kappa x pcg_rel_residual), at least 1e-12 relative; nothing there is tuned on GPU output.  After an accepted step
      poses() and switches() are the restated candidate, record.cost is oracle.evaluate_sc at them to 1e-12; odometry
      switches stay exactly 1 and the constant pose stays bitwise.
  (c) once per handle, last (it resets the scales): normal_eq() against unscaled_reduced within PROD x max(1, largest entry).
  (d) direct: direct_solve(b, -1) for the system's own b and two Gaussian right-hand sides, backward error against the
      restated matrix <= BE_ONE.
Every test prints measured error / tolerance per quantity.

Measured on an MI355X (36 tests, 20 s): largest error / tolerance -- d2 0.94 (hub, pcg: a diagonal entry summed over 301
incidences against 1e-12 relative), operator 0.09 (hub), model decrease 0.09, step_norm 0.05 (small-clamped, direct), direct solve
1e-5 of BE_ONE, normal_eq 0.007; everything else of (b) below 0.01 -- its tolerances are dominated by cond_2 x residual (cond_2
8e3 .. 6e7).  Three one-line perturbations of the kernels, each on a scratch build: without the clamp in k_switch_prepare's `den`
only small-clamped fails (operator 2e6 x its bound: no other case has an h_ss outside the clamp); with d2 taken from the reduced
diagonal in asm_incidence every case fails (a) at state 0 (5e3 x); with the sign of ub2's term flipped in k_switch_backsub every
direct / pcg case fails (b) at the first step (cost_change 1e4 x, gmax 2e2 x its tolerance) while (a) still passes."""
import os
import time

import numpy as np
import pytest

import _switch_restatement as R
from _direct_restatement import backward_error, system_matrix
from test_gpu_direct import BE_ONE, ArrayGraph

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
PROD = 1e-11       # the project's bound on a product against the oracle's (test_gpu_parity.py, test_gpu_fuzz.py)
TILE_INC = 256     # incidences (and rows) a K2 / K3 tile holds at most
PCG_RTOL = 1e-13   # variants "pcg*"
RESIDUAL_CAP = R.RATIO * PCG_RTOL     # the largest pcg_rel_residual a record of (b) may report, either solver


# ------------------------------------------------------------------------------------------------------------ cases
def walk_graph(n, loops, seed, heading_noise=0.01):
    """loops = [(a, b, kind)]: kind 1 measured a -> b from the true walk (noise 0.02, 0.02, 0.01), kind 2 a random measurement;
    odometry i -> i + 1 first, with noise (0.02, 0.02, heading_noise); initial poses = the odometry integrated from pose 0.
    The loops are sorted by kind here (stably), so the arrays come out grouped as odometry, kind 1, kind 2 -- the order
    pgo.Graph.from_arrays regroups edges into, which is the order Solver.switches() answers in"""
    rng = np.random.default_rng(seed)
    loops = sorted(loops, key=lambda l: l[2])      # (stable)
    turn = rng.choice([-1, 0, 0, 0, 1], n)
    turn[0] = 0
    th = np.cumsum(turn) * (np.pi / 2)
    xy = np.zeros((n, 2))
    xy[1:] = np.cumsum(np.column_stack([np.cos(th[:-1]), np.sin(th[:-1])]), axis=0)
    ia = np.concatenate([np.arange(n - 1), np.array([l[0] for l in loops], np.int64)]).astype(np.int32)
    ib = np.concatenate([np.arange(1, n), np.array([l[1] for l in loops], np.int64)]).astype(np.int32)
    kind = np.concatenate([np.zeros(n - 1, np.uint8), np.array([l[2] for l in loops], np.uint8)])
    d = xy[ib] - xy[ia]
    c, s = np.cos(th[ia]), np.sin(th[ia])
    meas = np.column_stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], th[ib] - th[ia]])
    noise = rng.standard_normal(meas.shape) * np.array([0.02, 0.02, 0.01])
    noise[:n - 1, 2] *= heading_noise / 0.01
    meas += noise
    bogus = kind == 2
    meas[bogus] = rng.standard_normal((int(bogus.sum()), 3)) * np.array([1.0, 1.0, 0.5])
    odo = meas[:n - 1]
    th0 = np.concatenate([[0.0], np.cumsum(odo[:, 2])])
    c, s = np.cos(th0[:-1]), np.sin(th0[:-1])
    xy0 = np.zeros((n, 2))
    xy0[1:] = np.cumsum(np.column_stack([c * odo[:, 0] - s * odo[:, 1], s * odo[:, 0] + c * odo[:, 1]]), axis=0)
    return ArrayGraph(np.column_stack([xy0, th0]), ia, ib, meas, kind)


def small_loops(f):
    """f = the constant pose (0 or 39)"""
    return [(25, 5, 1), (f, 12, 1), (10, 11, 1), (3, 30, 1), (7, 19, 1), (22, 35, 1),
            (17, f, 2), (21, 20, 2), (30, 3, 2), (2, 33, 2), (28, 9, 2), (14, 38, 2)]


REJECTING_LOOPS = [(50, 10, 1), (0, 20, 1), (30, 31, 1), (5, 45, 1), (12, 40, 1), (25, 55, 1), (8, 33, 1), (18, 52, 1),
                   (44, 0, 2), (36, 35, 2), (45, 5, 2), (3, 58, 2), (27, 14, 2)]


def hub_loops(n=301):
    """300 switchable edges on pose n - 1, a third of them as (hub, j), every fifth bogus; on the constant pose 0 and on the
    neighbour n - 2 one edge in each orientation, the second of the other kind"""
    h = n - 1
    out = [(0, h, 1), (h, 0, 2), (h - 1, h, 1), (h, h - 1, 2)]
    for j in range(2, h - 2):
        out.append((h, j, 2 if j % 5 == 0 else 1) if j % 3 == 0 else (j, h, 2 if j % 5 == 0 else 1))
    return out


def tiles_loops():
    """257 poses: poses 0 .. 167 carry one loop incidence each (pairs (p, p + 2), (p + 1, p + 3) of every four poses, some
    reversed, every seventh bogus; the seams sit in the groups at 100 and 104 and on pose 0), poses 170 .. 191 a dense cluster,
    poses 192 .. 255 two loop incidences each, pose 256 none -- tile_rows() gives 85, 85, 22, 64 and 1 rows"""
    out, k = [(6, 0, 2)], 0
    for p in range(0, 168, 4):
        if p == 100:       # adjacent poses, both orientations
            out += [(100, 101, 1), (103, 102, 2)]
        elif p == 104:     # a pair twice: the copy reversed and of the other kind
            out += [(104, 106, 1), (106, 104, 2)]
        else:
            for a in (p, p + 1):
                k += 1
                out.append((a + 2, a, 1) if k % 3 == 0 else (a, a + 2, 2 if k % 7 == 0 else 1))
    lo, hi = 170, 192
    deg = {i: 2 for i in range(lo, hi)}
    for d in range(2, hi - lo):
        for a in range(lo, hi - d):
            if sum(deg.values()) + 2 <= TILE_INC - 2:
                out.append((a, a + d, 1))
                deg[a] += 1
                deg[a + d] += 1
    out += [(i, i + 2, 1) for i in range(192, 254)] + [(192, 255, 1), (254, 193, 2)]
    return out


def tile_rows(n, ia, ib):
    """rows per K2 / K3 tile in the caller's pose order (structure.cpp): at least one row, more while the incidences fit
    TILE_INC and the rows stay below TILE_INC; also the incidences per tile"""
    ptr = np.concatenate([[0], np.cumsum(np.bincount(np.concatenate([ia, ib]), minlength=n))])
    rows, incs, row = [], [], 0
    while row < n:
        begin = row
        row += 1
        while row < n and ptr[row + 1] - ptr[begin] <= TILE_INC and row - begin < TILE_INC:
            row += 1
        rows.append(row - begin)
        incs.append(int(ptr[row] - ptr[begin]))
    return rows, incs


def _case(n, loops, seed, steps=8, fixed=0, heading_noise=0.01, **opts):
    return dict(n=n, loops=loops, seed=seed, steps=steps, fixed=fixed, heading_noise=heading_noise, opts=opts)


CASES = {
    "small": _case(40, small_loops(0), 11),
    "small-lambda4": _case(40, small_loops(0), 11, sc_prior_lambda=4.0),
    "small-lambda0.25": _case(40, small_loops(0), 11, sc_prior_lambda=0.25),
    "small-unscaled": _case(40, small_loops(0), 11, jacobi_scaling=0),
    "small-fixed-last": _case(40, small_loops(39), 11, fixed=39),
    # h_ss = sigma^2 (|j|^2 + lambda) is 0.25 .. 0.27 here: the clamp of the LM diagonal acts on every switch and, at a radius of
    # 1, weighs as much as h_ss itself (with the default 1e-6 no case would notice a missing clamp in `den`)
    "small-clamped": _case(40, small_loops(0), 11, min_lm_diagonal=0.3, radius0=1.0),
    "rejecting": _case(60, REJECTING_LOOPS, 15, heading_noise=1.5, radius0=1e6),
    "hub": _case(301, hub_loops(), 5, steps=4),
    "tiles": _case(257, tiles_loops(), 7, steps=4),
}
# (pad_tiles: the padded-slot layout takes plain tiles only -- on hub, whose heavy row is a tile of 301 incidences, the knob leaves
# the layout as it is; small, rejecting and tiles are padded)
VARIANTS = {
    "direct": dict(opts=dict(linear_solver=2), knobs={}),
    "pcg": dict(opts=dict(linear_solver=1, pcg_rtol=PCG_RTOL, pcg_coarse_poses=0, pcg_chain_len=8), knobs=dict(verify_residual=1)),
    "pcg-pad": dict(opts=dict(linear_solver=1, pcg_rtol=PCG_RTOL, pcg_coarse_poses=0, pcg_chain_len=8), knobs=dict(verify_residual=1, pad_tiles=1)),
    "pcg-order": dict(opts=dict(linear_solver=1, pcg_rtol=PCG_RTOL, pcg_coarse_poses=0, pcg_chain_len=8), knobs=dict(verify_residual=1), flip_order=True),
}


def build_case(case, O):
    c = CASES[case]
    ag = walk_graph(c["n"], c["loops"], c["seed"], c["heading_noise"])
    return ag, ag.to_oracle(O)


def restate_args(c):
    """the keyword arguments of _switch_restatement's functions for a case"""
    o = c["opts"]
    return dict(lam=o.get("sc_prior_lambda", 1.0), fixed=c["fixed"], jacobi_scaling=o.get("jacobi_scaling", 1),
                min_diag=o.get("min_lm_diagonal", 1e-6), threads=THREADS)


# ------------------------------------------------------------------------------------------------------------ checks
def operator_columns(s, n):
    cols, d2 = np.zeros((3 * n, 3 * n)), None
    e = np.zeros(3 * n)
    for k in range(3 * n):
        e[k] = 1.0
        if k == 0:
            cols[:, k], d2 = s.system_spmv(e, want_d2=True)
        else:
            cols[:, k] = s.system_spmv(e)
        e[k] = 0.0
    return cols, d2


def check_operator(O, s, ag, og, c, label, worst):
    """(a), and (d) on a handle on the direct solve"""
    recs = s.iter_records()
    radius = recs[-1]["radius"]
    radius_elim = recs[-2]["radius"] if recs[-1]["step_ok"] != 1 else None
    S = R.joint_system(O, og, s.poses(), s.switches(), ag.poses, radius, radius_elim=radius_elim, **restate_args(c))
    A = system_matrix(S.sysm)
    Ad = A.toarray()
    n, f = ag.n_poses, c["fixed"]
    G, d2 = operator_columns(s, n)
    scale = max(1.0, np.abs(Ad).max())
    err = np.abs(G - Ad).max() / (PROD * scale)
    err_d2 = (np.abs(d2 - S.sysm.d2) / S.sysm.d2).max() / 1e-12
    worst["operator"] = max(worst.get("operator", 0.0), err)
    worst["d2"] = max(worst.get("d2", 0.0), err_d2)
    print("%s radius %.3e%s: operator %.3f of its bound (largest entry %.2e), d2 %.3f" % (
        label, radius, "" if radius_elim is None else " (eliminated at %.3e)" % radius_elim, err, scale, err_d2))
    assert err <= 1.0, (label, np.abs(G - Ad).max(), scale)
    # (1e-12 relative is the issue's bound.  hub's heavy row reaches 0.94 of it: a diagonal entry summed over 301 incidences, in
    # chunks of 256 in a fixed order, against scipy's order.  Stable while that order stands; a kernel change that re-orders the
    # chunk sums of the heavy row can cross it without being wrong -- look at this entry first then.)
    assert err_d2 <= 1.0, (label, err_d2)
    eye = np.eye(3 * n)[3 * f:3 * f + 3]
    np.testing.assert_array_equal(G[3 * f:3 * f + 3], eye)
    np.testing.assert_array_equal(G[:, 3 * f:3 * f + 3], eye.T)
    if s.info().linear_solver == 2:
        rng = np.random.default_rng(7)
        for name, b in (("b", np.array(S.sysm.b)), ("gauss0", rng.standard_normal(3 * n)), ("gauss1", rng.standard_normal(3 * n))):
            b[3 * f:3 * f + 3] = 0.0
            y = s.direct_solve(np.ascontiguousarray(b), -1)
            eta = backward_error(A, y, b)
            worst["direct"] = max(worst.get("direct", 0.0), eta / BE_ONE)
            print("%s direct_solve(%s): eta %.2e" % (label, name, eta))
            assert np.isfinite(y).all() and not y[3 * f:3 * f + 3].any(), (label, name)
            assert eta <= BE_ONE, (label, name, eta)


def check_step(O, s, ag, og, c, st, before, dec, label, worst):
    """(b): the record the handle just wrote against the step restated from the state `before` = (poses, switches, radius,
    gmax of that state)"""
    P0, SW0, radius, gmax0 = before
    rec = s.iter_records()[-1]
    opt = s.options
    assert st.valid and not st.term, (label, st.valid, st.term)
    # the tolerances below scale with a residual the handle itself reports: it is bounded first, or a stalled solve would widen its
    # own tolerances.  PCG was asked for pcg_rtol = 1e-13 on its recurrence residual and reports the recomputed true one
    # (verify_residual), which may lag by the rounding of the iterations: RATIO x pcg_rtol.  The direct solve is held to the same.
    assert 0.0 <= rec["pcg_rel_residual"] <= RESIDUAL_CAP, (label, rec["pcg_rel_residual"])
    tol = R.step_tolerances(st, rec["pcg_rel_residual"], radius, opt.max_radius)
    assert abs(st.rho - opt.min_relative_decrease) > tol["rho"], (label, st.rho, tol["rho"])
    assert rec["step_ok"] == int(st.step_ok), (label, rec, st.rho)
    got = {"step_norm": rec["step_norm"], "model": rec["cost_change"] / rec["relative_decrease"], "cost_change": rec["cost_change"],
           "rho": rec["relative_decrease"]}
    want = {"step_norm": st.step_norm, "model": st.model, "cost_change": st.cost_change, "rho": st.rho}
    P1, SW1 = s.poses(), s.switches()
    cost1 = O.evaluate_sc(og, P1, SW1, restate_args(c)["lam"], want=False, threads=THREADS)[0]
    if st.step_ok:
        got.update(gmax=rec["gradient_max_norm"], radius=rec["radius"])
        want.update(gmax=st.gmax, radius=R.accepted_radius(radius, st.rho, opt.max_radius))
        vec = max(np.abs(P1 - st.cand_poses).max(), np.abs(SW1 - st.cand_switches).max())
        ratios = {"vector": vec / tol["vector"]}
        assert rec["cost"] == pytest.approx(cost1, rel=1e-12), (label, rec["cost"], cost1)
    else:
        ratios = {"gmax": abs(rec["gradient_max_norm"] - gmax0) / (R.FLOOR * gmax0),
                  "radius": abs(rec["radius"] - radius / dec) / (R.FLOOR * radius / dec),
                  "cand_cost": abs(rec["cost"] - st.cand_cost) / tol["cost_change"]}
        np.testing.assert_array_equal(P1, P0)
        np.testing.assert_array_equal(SW1, SW0)
    for q in got:
        ratios[q] = abs(got[q] - want[q]) / tol[q]
    print("%s iteration %d step_ok %d rho %.3e kappa %.1e rel_residual %.1e: error / tolerance %s" % (
        label, rec["iter"], rec["step_ok"], st.rho, st.kappa, rec["pcg_rel_residual"],
        " ".join("%s %.3f" % (q, v) for q, v in sorted(ratios.items()))))
    for q, v in ratios.items():
        worst[q] = max(worst.get(q, 0.0), v)
    assert all(v <= 1.0 for v in ratios.values()), (label, ratios, got, want, tol)
    assert np.all(SW1[ag.kind == 0] == 1.0), label
    np.testing.assert_array_equal(P1[c["fixed"]], ag.poses[c["fixed"]])


def check_normal_eq(O, s, ag, og, c, label, worst):
    """(c)"""
    rec = s.iter_records()[-1]
    assert rec["step_ok"] == 1, label
    P, SW = s.poses(), s.switches()
    g_ref, hd_ref = R.unscaled_reduced(O, og, P, SW, ag.poses, rec["radius"], **restate_args(c))
    g, hd = s.normal_eq()
    scale = max(1.0, np.abs(hd_ref).max(), np.abs(g_ref).max())
    err = max(np.abs(g - g_ref).max(), np.abs(hd - hd_ref).max()) / (PROD * scale)
    worst["normal_eq"] = err
    print("%s normal_eq: %.3f of its bound (largest entry %.2e)" % (label, err, scale))
    assert err <= 1.0, (label, np.abs(g - g_ref).max(), np.abs(hd - hd_ref).max(), scale)
    f = c["fixed"]
    assert not g[3 * f:3 * f + 3].any() and not hd[f].any(), label


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", list(CASES))
def test_switch_elimination_matches_the_joint_system(pgo, oracle, case, variant):
    c, v = CASES[case], VARIANTS[variant]
    t0 = time.perf_counter()
    ag, og = build_case(case, oracle)
    g = ag.to_pgo(pgo)
    assert np.array_equal(g.ia, ag.ia) and np.array_equal(g.ib, ag.ib) and np.array_equal(g.kind, ag.kind), case   # one edge order
    opts = dict(method=2, max_iters=50, fixed_pose=c["fixed"], **c["opts"], **v["opts"])
    if v.get("flip_order"):   # (the default, -1, resolves to the caller's order on single-rank graphs of this size)
        opts["pose_ordering"] = 1
    for k, val in v["knobs"].items():
        pgo.set_knob(k, val)
    try:
        s = pgo.Solver(g, pgo.Options(**opts))
    finally:
        for k in v["knobs"]:
            pgo.set_knob(k, -1)
    info = s.info()
    assert info.linear_solver == opts["linear_solver"], (case, variant, info.linear_solver)
    assert info.pose_ordering == (1 if v.get("flip_order") else 0), (case, variant, info.pose_ordering)
    if case == "hub":
        assert info.n_incidences == 2 * ag.n_edges and np.bincount(np.concatenate([ag.ia, ag.ib])).max() > TILE_INC
    stepping = variant in ("direct", "pcg")
    worst, dec, seen = {}, 2.0, []
    s.lm_begin()
    for k in range(c["steps"] + 1):
        label = "%s %s state %d" % (case, variant, k)
        check_operator(oracle, s, ag, og, c, label, worst)
        if k == c["steps"]:
            break
        rec = s.iter_records()[-1]
        before = (s.poses(), s.switches(), rec["radius"], rec["gradient_max_norm"])
        st = R.joint_step(oracle, og, before[0], before[1], ag.poses, before[2], **restate_args(c)) if stepping else None
        done, _ = s.lm_step(1)
        assert not done, (case, variant, k, s.iter_records()[-1])
        ok = s.iter_records()[-1]["step_ok"]
        seen.append(ok)
        if stepping:
            check_step(oracle, s, ag, og, c, st, before, dec, label, worst)
        dec = 2.0 if ok == 1 else 2.0 * dec
    if case == "rejecting":   # the refresh after a rejected step was exercised: rejections in a row, then an accepted step
        runs = "".join("1" if ok == 1 else "0" for ok in seen)
        assert "001" in runs, (case, variant, runs)
    extra = 0
    while s.iter_records()[-1]["step_ok"] != 1 and extra < 8:   # (c) wants a state after an accepted step
        s.lm_step(1)
        extra += 1
    check_normal_eq(oracle, s, ag, og, c, "%s %s" % (case, variant), worst)
    assert s.info().direct_fallbacks == 0, (case, variant)
    print("%s %s: steps %s, worst error / tolerance %s, %.1f s" % (
        case, variant, seen, {q: round(float(x), 3) for q, x in sorted(worst.items())}, time.perf_counter() - t0))
    s.close()
