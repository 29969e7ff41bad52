"""Every PCG preconditioner's z = M^-1 r, and the product the PCG loop runs, against the numpy restatement
(oracle.lm_system / oracle.Precond, itself checked against the dense definition in test_precond_restatement.py).

A handle is advanced with lm_begin / lm_step(1) to a state after an ACCEPTED step (new linearisation) and, where the first
iterations have one, after a REJECTED step (new radius); the restatement is built at (s.poses(), initial poses, radius of the
last record) and compared there.  H on the GPU agrees with the oracle to ~1e-11 relative (test_assembly_and_spmv_parity),
so a forward error in z grows with the conditioning of each block; the primary criteria are therefore BACKWARD errors,
which do not depend on it and which a wrong operator still misses by orders of magnitude:
  one level   for every block / group / segment k:  |M_k z_k - r_k| <= 1e-10 (|M_k| |z_k| + |r_k|)   (infinity norms)
              and the forward error |z - z_ref| <= 1e-9 |z_ref| where every block has cond <= 1e4 (computed here)
  two levels  the coarse share c = z - M1_ref^-1 r lies in range(P) and solves the Galerkin system P'AP e = P'r backward
              stably; z - P e passes the one-level criterion
Cases name the kernel instantiation they reach (solver_create.hip: chain apply <poses per lane, wavefronts per
workgroup>, serial or scan recurrence; product kernel; coarse order and apply)."""
import os
import time

import numpy as np
import pytest

from conftest import DATA, oracle_graph

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
BE_ONE = 1e-10      # one-level backward error
BE_GAL = 1e-9       # Galerkin backward error and range(P) test
FWD = 1e-9          # forward error where max cond(M_k) <= 1e4
PROD = 1e-11        # (H + D'D) x and d2: relative share (rounding) of the bound
# agreement of the Jacobian entries with the oracle: |dJ| <= DJ + DJ_REL |J| per entry.  test_edge_kernel_parity asserts
# 1e-11 absolute at the initial poses; at later LM states an absolute 1e-11 was exceeded 15.8x (synthetic 30011, chain 64,
# DCS: one d2 entry 4.8e-10 relative), and whitened Jacobians (info weighting, entries up to ~1e2) agree to ~2e-11
# RELATIVE (INTEL: d2 and product 4.4e-11 relative), hence the two terms.  A d2 without its 1 / radius, or a missing
# block, is off by orders of magnitude more.
DJ = 4e-10
DJ_REL = 1e-10


def load(pgo, name, n_out=0, seed=1):
    g = pgo.ReadG2O(os.path.join(DATA, name + ".g2o"))
    if n_out:
        g.add_random_C(n_out, seed)
    return g


def arrays(g):
    return [np.array(a) for a in (g.poses, g.ia, g.ib, g.meas, g.kind, g.info)]


def mit_duplicates(pgo):
    """test_duplicate_edges_are_summed_in_a_fixed_order's graph: every fifth odometry pair tripled, every loop doubled"""
    poses, ia, ib, meas, kind, info = arrays(load(pgo, "MIT"))
    rng = np.random.default_rng(11)
    odo = np.nonzero(kind == 0)[0][::5]
    extra = np.concatenate([odo, odo, np.nonzero(kind != 0)[0]])
    ia2, ib2 = np.concatenate([ia, ia[extra]]), np.concatenate([ib, ib[extra]])
    meas2 = np.concatenate([meas, meas[extra] + 0.01 * rng.standard_normal((len(extra), 3))])
    kind2 = np.concatenate([kind, kind[extra]])
    order = np.argsort(kind2, kind="stable")
    return pgo.Graph.from_arrays(poses, ia2[order], ib2[order], meas2[order], kind2[order])


def mit_gaps(pgo):
    """MIT with the odometry edge 100-101 removed (C = 0 inside a chain segment) and a closure-kind edge 200-201 added
    (a non-odometry block on the chain)"""
    poses, ia, ib, meas, kind, info = arrays(load(pgo, "MIT"))
    keep = ~((ia == 100) & (ib == 101))
    k = np.nonzero((ia == 200) & (ib == 201))[0][:1]
    ia2, ib2 = np.concatenate([ia[keep], ia[k]]), np.concatenate([ib[keep], ib[k]])
    meas2 = np.concatenate([meas[keep], meas[k] + np.array([0.05, -0.02, 0.01])])
    kind2 = np.concatenate([kind[keep], np.ones(1, np.uint8)])
    order = np.argsort(kind2, kind="stable")
    return pgo.Graph.from_arrays(poses, ia2[order], ib2[order], meas2[order], kind2[order])


def mit_free(pgo, n_free=40):
    """MIT (808 poses) with n_free edge-less poses appended: with 16-pose aggregates, 816..831 and 832..847 hold no pose of
    the coarse space (dead aggregates)"""
    poses, ia, ib, meas, kind, info = arrays(load(pgo, "MIT"))
    extra = poses[-1] + np.arange(1, n_free + 1)[:, None] * np.array([0.5, 0.25, 0.0])
    return pgo.Graph.from_arrays(np.concatenate([poses, extra]), ia, ib, meas, kind)


SYN = {}


def synth(pgo, n):
    if n not in SYN:
        SYN[n] = pgo.synth_manhattan(n, 4.0, 0.10, 5)
    return SYN[n]


EXACT = dict(pcg_rtol=1e-8, pcg_max_iters=400000)
# id: (graph builder, options, knobs, expected info fields, checks)
#   checks: "all" = product, one / two levels, side effects; "product" = the product kernel only
CASES = {
    "MIT-3x3-k_cg_init": (lambda p: load(p, "MIT"), dict(method=1, pcg_block_poses=1, pcg_chain_len=0, linear_solver=1), {},
                          dict(pcg_block_poses=1, pcg_chain_len=0), "all"),
    "MIT-k_spmv_t": (lambda p: load(p, "MIT"), dict(method=1, pcg_block_poses=1, pcg_chain_len=0, linear_solver=1),
                     {"spmv_pipe": 0}, dict(pcg_block_poses=1), "product"),
    "INTEL50-B32-ragged-k_cg_init_g": (lambda p: load(p, "INTEL", 50), dict(method=1, pcg_block_poses=32, pcg_chain_len=0, linear_solver=1),
                                       {}, dict(pcg_block_poses=32, pcg_chain_len=0, pcg_coarse_poses=0), "all"),
    "M3500-B6-ragged-k_cg_init_g": (lambda p: load(p, "M3500"), dict(method=1, pcg_block_poses=6, pcg_chain_len=0, linear_solver=1),
                                    {}, dict(pcg_block_poses=6, pcg_coarse_poses=0), "all"),
    "MITdup-B32": (mit_duplicates, dict(method=1, pcg_block_poses=32, pcg_chain_len=0, linear_solver=1), {},
                   dict(pcg_block_poses=32), "all"),
    "MITdup-chain64-k_chain_dupfix": (mit_duplicates, dict(method=1, pcg_chain_len=64, linear_solver=1), {},
                                      dict(pcg_chain_len=64, chain_kernel=2), "all"),
    "MITgaps-chain64-C0-closure": (mit_gaps, dict(method=1, pcg_chain_len=64, linear_solver=1), {},
                                   dict(pcg_chain_len=64, chain_kernel=2), "all"),
    "syn30011-chain8-cl2x1-serial": (lambda p: synth(p, 30011), dict(method=1, pcg_chain_len=8, pcg_rtol=0.1), {},
                                     dict(pcg_chain_len=8, chain_kernel=2, pose_ordering=0), "all"),
    "syn30011-chain64-cl2x1-scan": (lambda p: synth(p, 30011), dict(method=1, pcg_chain_len=64, pcg_rtol=0.1), {},
                                    dict(pcg_chain_len=64, chain_kernel=2, pose_ordering=0), "all"),
    "syn30011-chain256-cl4x1-scan": (lambda p: synth(p, 30011), dict(method=1, pcg_chain_len=256, pcg_rtol=0.1), {},
                                     dict(pcg_chain_len=256, chain_kernel=4, pose_ordering=0), "all"),
    "syn160000-chain64-cl2x4-order-k_spmv_1pad": (lambda p: synth(p, 160000), dict(method=1, pcg_chain_len=64, pcg_rtol=0.1), {},
                                                  dict(pcg_chain_len=64, chain_kernel=2, pose_ordering=1), "all"),
    "syn160000-chain256-cl4x4-order": (lambda p: synth(p, 160000), dict(method=1, pcg_chain_len=256, pcg_rtol=0.1), {},
                                       dict(pcg_chain_len=256, chain_kernel=4, pose_ordering=1), "all"),
    "syn160000-k_spmv_1-unpadded": (lambda p: synth(p, 160000), dict(method=1, pcg_chain_len=64, pcg_rtol=0.1), {"pad_tiles": 0},
                                    dict(pcg_chain_len=64), "product"),
    "syn160000-k_spmv_p": (lambda p: synth(p, 160000), dict(method=1, pcg_chain_len=64, pcg_rtol=0.1), {"spmv_pipe": 2},
                           dict(pcg_chain_len=64), "product"),
    "M3500-m1-two-level-matvec": (lambda p: load(p, "M3500"), dict(method=1, linear_solver=1, **EXACT), {},
                                  dict(pcg_block_poses=32, pcg_coarse_poses=16), "all"),
    "M3500-m0-two-level-matvec": (lambda p: load(p, "M3500"), dict(method=0, linear_solver=1, **EXACT), {},
                                  dict(pcg_block_poses=32, pcg_coarse_poses=16), "all"),
    "FRH-two-level-matvec": (lambda p: load(p, "FRH"), dict(method=1, linear_solver=1, **EXACT), {},
                             dict(pcg_coarse_poses=16), "all"),
    "syn30011-two-level-k_tri_apply": (lambda p: synth(p, 30011), dict(method=1, **EXACT), {},
                                       dict(pcg_coarse_poses=64, pcg_coarse_rank=1407), "all"),
    "syn100000-two-level-chain64-order": (lambda p: synth(p, 100000), dict(method=1, **EXACT), {},
                                          dict(pcg_coarse_poses=64, pcg_chain_len=64, pose_ordering=1), "all"),
    "CSAIL-fixed17-B32-coarse16": (lambda p: load(p, "CSAIL"), dict(method=1, fixed_pose=17, pcg_block_poses=32, pcg_chain_len=0,
                                                                     pcg_coarse_poses=16, linear_solver=1, **EXACT), {},
                                   dict(pcg_block_poses=32, pcg_coarse_poses=16), "all"),
    "MIT-nofixed-coarse16": (lambda p: load(p, "MIT"), dict(method=1, fixed_pose=-1, pcg_block_poses=32, pcg_chain_len=0,
                                                            pcg_coarse_poses=16, linear_solver=1, **EXACT), {},
                             dict(pcg_block_poses=32, pcg_coarse_poses=16), "all"),
    "INTEL-B32-coarse20-unrounded": (lambda p: load(p, "INTEL"), dict(method=1, pcg_block_poses=32, pcg_chain_len=0,
                                                                      pcg_coarse_poses=20, linear_solver=1, **EXACT), {},
                                     dict(pcg_block_poses=32, pcg_coarse_poses=20, pcg_coarse_rank=3 * 62), "all"),
    "MITfree-coarse16-dead-aggregates": (mit_free, dict(method=1, pcg_block_poses=32, pcg_chain_len=0, pcg_coarse_poses=16,
                                                        linear_solver=1, **EXACT), {},
                                         dict(pcg_block_poses=32, pcg_coarse_poses=16), "all"),
    "INTEL-info-weighting-m1": (lambda p: load(p, "INTEL"), dict(method=1, info_weighting=1, pcg_block_poses=32, pcg_chain_len=0,
                                                                 linear_solver=1), {}, dict(pcg_block_poses=32), "all"),
    "INTEL50-direct-handle": (lambda p: load(p, "INTEL", 50), dict(method=1), {}, dict(linear_solver=2), "all"),
}


def block_norms(v, blk, nb):
    out = np.zeros(nb)
    np.maximum.at(out, blk, np.abs(v))
    return out


def one_level_backward(M, z, r):
    """max over blocks k of |M_k z_k - r_k| / (|M_k| |z_k| + |r_k|), infinity norms"""
    nb = M.n_blocks
    res = M.M1 @ z - r
    rows = np.asarray(abs(M.M1).sum(axis=1)).reshape(-1)
    den = block_norms(rows, M.blk, nb) * block_norms(z, M.blk, nb) + block_norms(r, M.blk, nb)
    return float(np.max(block_norms(res, M.blk, nb) / den))


def max_block_cond(M):
    """max over blocks of cond_2(M_k), or None where stacking the blocks densely would take more than ~250 MB"""
    b = int(np.bincount(M.blk).max())
    if M.n_blocks * b * b > 3e7:
        return None
    n = M.M1.shape[0]
    conds = []
    for k0 in range(0, n, b):
        sl = slice(k0, min(n, k0 + b))
        conds.append(np.linalg.cond(M.M1[sl, sl].toarray()))
    return float(max(conds))


def check_state(pgo, O, s, g, og, opts, info, what, label, report):
    rec = s.iter_records()[-1]
    x, radius = s.poses(), rec["radius"]
    t0 = time.perf_counter()
    sysm = O.lm_system(og, x, np.array(g.poses), radius, method=opts.get("method", 1), fixed_pose=opts.get("fixed_pose", 0),
                       info_weighting=bool(opts.get("info_weighting", 0)), threads=THREADS)
    N = g.n_poses
    perm = pgo.pose_order(N, g.ia, g.ib, max(64, info.pcg_chain_len)) if info.pose_ordering == 1 else None
    rng = np.random.default_rng(7)
    out = {}
    # the LM diagonal and the product (H + D'D) x through the kernel the PCG loop runs.  The GPU's Jacobian agrees with the
    # oracle's to DJ absolute per entry (test_edge_kernel_parity), so an entry of H = (JS)'(JS) -- a sum of products, d2 a
    # sum of squares -- may differ by far more than 1e-11 RELATIVE where it is small (measured: 4.8e-10 on one d2 entry of
    # the synthetic graph); the bounds below are that Jacobian agreement carried through the products (first order, |.|
    # entrywise, pattern of J) plus rounding: a wrong radius, diagonal or block exceeds them by orders of magnitude.
    xv = rng.standard_normal(3 * N)
    y, d2 = s.system_spmv(xv, want_d2=True)
    JSa = abs(sysm.JS)
    pat = JSa.copy()
    pat.data[:] = 1.0
    d2_bound = (2.0 * DJ * sysm.s * np.asarray(JSa.sum(axis=0)).reshape(-1) + 2.0 * DJ_REL * sysm.H.diagonal()) / radius + PROD * sysm.d2
    out["d2"] = float(np.max(np.abs(d2 - sysm.d2) / np.abs(sysm.d2)))
    out["d2/bound"] = float(np.max(np.abs(d2 - sysm.d2) / d2_bound))
    y_ref = sysm.H @ xv + sysm.d2 * xv
    y_bound = (DJ * (sysm.s * (pat.T @ abs(sysm.JS @ xv)) + JSa.T @ (pat @ abs(sysm.s * xv)))
               + DJ_REL * (JSa.T @ abs(sysm.JS @ xv) + JSa.T @ (JSa @ abs(xv))) + d2_bound * abs(xv) + PROD * np.abs(y_ref).max())
    out["product"] = float(np.abs(y - y_ref).max() / np.abs(y_ref).max())
    out["product/bound"] = float(np.max(np.abs(y - y_ref) / y_bound))
    assert out["d2/bound"] <= 1.0, (label, out)
    assert out["product/bound"] <= 1.0, (label, out)
    if what == "all":
        M = O.Precond(sysm, x, block_poses=info.pcg_block_poses, chain_len=info.pcg_chain_len,
                      coarse_poses=info.pcg_coarse_poses, perm=perm)
        cond = max_block_cond(M)
        out["cond"] = cond
        out["one"], out["fwd"] = 0.0, 0.0
        for _ in range(3):
            r = rng.standard_normal(3 * N)
            ri, zi = M.to_internal(r), M.to_internal(s.precond(r))
            assert np.isfinite(zi).all()
            z1 = zi
            if M.P is not None:
                # the coarse share c = z - M1_ref^-1 r.  M1_ref^-1 r carries the forward error of the one-level apply
                # (cond(M1_k) x ~1e-11), which lands in c outside range(P): that is what bounds the range test below.
                c = zi - M.apply1(ri)
                PtP = (M.P.T @ M.P).toarray()
                dead = np.diag(PtP) == 0.0
                PtP[dead, dead] = 1.0
                e = np.linalg.solve(PtP, M.P.T @ c)
                rng_err = float(np.linalg.norm(c - M.P @ e) / np.linalg.norm(c))
                rc = M.P.T @ ri
                gal = float(np.abs(M.Ac @ e - rc).max() / (np.abs(M.Ac).sum(axis=1).max() * np.abs(e).max() + np.abs(rc).max()))
                out["range"] = max(out.get("range", 0.0), rng_err)
                out["galerkin"] = max(out.get("galerkin", 0.0), gal)
                z1 = zi - M.P @ e
            out["one"] = max(out["one"], one_level_backward(M, z1, ri))
            if cond is not None and cond <= 1e4:
                zr = M.apply(ri)
                out["fwd"] = max(out["fwd"], float(np.abs(zi - zr).max() / np.abs(zr).max()))
        out["n_dead"] = M.n_dead
    out["oracle_s"] = time.perf_counter() - t0
    report.append((label, rec["iter"], out))
    print(label, "LM iteration", rec["iter"], {k: (("%.2e" % v) if isinstance(v, float) else v) for k, v in out.items()})
    if what == "all":
        assert out["one"] <= BE_ONE, (label, out)
        assert out["fwd"] <= FWD, (label, out)
        if "range" in out:
            assert out["range"] <= BE_GAL and out["galerkin"] <= BE_GAL, (label, out)


def strip(recs):
    return [{k: v for k, v in r.items() if k != "seconds"} for r in recs]


@pytest.mark.parametrize("case", list(CASES))
def test_preconditioner_matches_the_restatement(pgo, oracle, case):
    build, opts, knobs, expect, what = CASES[case]
    O = oracle
    g = build(pgo)
    og = oracle_graph(O, g)
    for k, v in knobs.items():
        pgo.set_knob(k, v)
    try:
        s = pgo.Solver(g, pgo.Options(max_iters=12, **opts))
        ref = pgo.Solver(g, pgo.Options(max_iters=12, **opts))
    finally:
        for k in knobs:
            pgo.set_knob(k, -1)
    info = s.info()
    for k, v in expect.items():
        assert getattr(info, k) == v, (case, k, getattr(info, k), v)
    t0 = time.perf_counter()
    s.lm_begin()
    seen, report = set(), []
    steps = 0
    while steps < 12 and not ({1, 0} <= seen or (what == "product" and 1 in seen)):
        done, _ = s.lm_step(1)
        steps += 1
        ok = s.iter_records()[-1]["step_ok"]
        if ok in (0, 1) and ok not in seen:
            seen.add(ok)
            check_state(pgo, O, s, g, og, opts, info, what, "%s %s" % (case, "accepted" if ok else "rejected"), report)
        if done:
            break
    assert 1 in seen, case
    t_gpu = time.perf_counter() - t0
    # the debug entry points have no side effects: a second handle stepped without them takes the same trajectory, bitwise
    ref.lm_begin()
    for _ in range(steps):
        ref.lm_step(1)
    np.testing.assert_array_equal(s.poses(), ref.poses())
    assert strip(s.iter_records()) == strip(ref.iter_records())
    if info.pcg_coarse_poses:
        assert s.info().pcg_coarse_off_iters == 0 and ref.info().pcg_coarse_off_iters == 0, case
    print(case, "steps", steps, "seen", sorted(seen), "%.1f s" % t_gpu)
    s.close()
    ref.close()
