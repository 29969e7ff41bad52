"""Scoring on the host (include/pgo.h, "scoring"): pgo_synth_manhattan_truth is the ground truth of the graph the generator
builds, and pgo_trajectory_error_eval is the ATE / RPE the header defines -- checked against a numpy longdouble restatement.
No GPU."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

EPS = np.finfo(np.float64).eps
CASES = [(300, 3), (2000, 7), (5000, 11)]
LD = np.longdouble


@pytest.fixture(scope="module")
def graphs(pgo):
    out = {}
    for n, seed in CASES:
        g = pgo.synth_manhattan(n, 4.0, 0.1, seed)
        out[(n, seed)] = (g, np.array(g.poses), pgo.synth_manhattan_truth(n, seed))
    return out


def wrap(a):
    return np.arctan2(np.sin(a), np.cos(a))


def rel_pose(P, ia, ib):
    """P_a^-1 P_b for pose arrays (any float dtype)"""
    d = P[ib, :2] - P[ia, :2]
    c, s = np.cos(P[ia, 2]), np.sin(P[ia, 2])
    return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], P[ib, 2] - P[ia, 2]], axis=1)


def restate(est, ref, mask=None, align=False, delta=1):
    """the definitions of include/pgo.h in longdouble; returns the dict of pgo_traj_error and the (n, 2) per-pose array"""
    est, ref = np.asarray(est, LD), np.asarray(ref, LD)
    n = len(est)
    m = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    out = dict(n_poses=int(m.sum()), n_pairs=0, ate_max_pose=-1, rpe_max_pose=-1, align_x=LD(0), align_y=LD(0), align_phi=LD(0))
    for k in ("ate_rmse", "ate_mean", "ate_max", "rot_rmse", "rot_max", "rpe_trans_rmse", "rpe_trans_max", "rpe_rot_rmse", "rpe_rot_max"):
        out[k] = LD(0)
    per = np.zeros((n, 2), LD)
    if m.any():
        p, q = est[m, :2], ref[m, :2]
        phi, t = LD(0), np.zeros(2, LD)
        if align:
            pb, qb = p.mean(axis=0), q.mean(axis=0)
            u, v = p - pb, q - qb
            a, b = (u * v).sum(), (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]).sum()
            phi = np.arctan2(b, a) if (a != 0 or b != 0) else LD(0)
            c, s = np.cos(phi), np.sin(phi)
            t = qb - np.array([c * pb[0] - s * pb[1], s * pb[0] + c * pb[1]])
        c, s = np.cos(phi), np.sin(phi)
        e = np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1]], axis=1) + t - q
        tr = np.sqrt((e * e).sum(axis=1))
        rot = np.abs(wrap(est[m, 2] + phi - ref[m, 2]))
        per[m, 0], per[m, 1] = tr, rot
        idx = np.flatnonzero(m)
        out.update(align_x=t[0], align_y=t[1], align_phi=phi, ate_rmse=np.sqrt((tr * tr).mean()), ate_mean=tr.mean(), ate_max=tr.max(),
                   ate_max_pose=int(idx[np.argmax(tr)]), rot_rmse=np.sqrt((rot * rot).mean()), rot_max=rot.max())
    if 0 < delta < n:
        i = np.flatnonzero(m[:-delta] & m[delta:])
        if i.size:
            dp, dq = rel_pose(est, i, i + delta), rel_pose(ref, i, i + delta)
            c, s = np.cos(dq[:, 2]), np.sin(dq[:, 2])
            u = dp[:, :2] - dq[:, :2]
            tr = np.sqrt((c * u[:, 0] + s * u[:, 1]) ** 2 + (-s * u[:, 0] + c * u[:, 1]) ** 2)
            rot = np.abs(wrap(dp[:, 2] - dq[:, 2]))
            out.update(n_pairs=int(i.size), rpe_max_pose=int(i[np.argmax(tr)]), rpe_trans_rmse=np.sqrt((tr * tr).mean()),
                       rpe_trans_max=tr.max(), rpe_rot_rmse=np.sqrt((rot * rot).mean()), rpe_rot_max=rot.max())
    return out, per


DOUBLES = ("ate_rmse", "ate_mean", "ate_max", "rot_rmse", "rot_max", "rpe_trans_rmse", "rpe_trans_max", "rpe_rot_rmse", "rpe_rot_max")


def compare(got, ref, n, what):
    """8 n eps relative on every rmse / mean / max, 8 n eps rad on align_phi; counts exact.  (The indices of the maxima are
    compared by the callers that can: two poses may tie within rounding.)"""
    tol = 8 * n * EPS
    for k in ("n_poses", "n_pairs"):
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in DOUBLES:
        assert abs(LD(got[k]) - ref[k]) <= tol * abs(ref[k]), (what, k, got[k], float(ref[k]))
    assert abs(LD(got["align_phi"]) - ref["align_phi"]) <= tol, (what, got["align_phi"], float(ref["align_phi"]))


# ------------------------------------------------------------------ ground truth
@pytest.mark.parametrize("n,seed", CASES)
def test_truth_is_the_generators(graphs, n, seed):
    """measurement minus the truth's relative pose, on every odometry and closure edge: the generator's noise, sigma 0.02 m and
    0.01 rad -- every component within 6 sigma, the sample deviations within 10 % of the sigmas"""
    g, _, truth = graphs[(n, seed)]
    kind = np.array(g.kind)
    sel = kind <= 1
    ia, ib, meas = np.array(g.ia)[sel], np.array(g.ib)[sel], np.array(g.meas)[sel]
    rel = rel_pose(truth, ia, ib)
    d = meas - rel
    d[:, 2] = wrap(d[:, 2])
    print("n %d: max |dx| %.4f |dy| %.4f |dth| %.4f, std %.5f %.5f %.5f" % (n, *np.abs(d).max(axis=0), *d.std(axis=0)))
    assert sel.sum() > n and (kind == 1).sum() > n
    assert np.abs(d[:, :2]).max() < 0.12 and np.abs(d[:, 2]).max() < 0.06
    assert 0.018 <= d[:, :2].std() <= 0.022 and 0.018 <= d[:, 0].std() <= 0.022 and 0.018 <= d[:, 1].std() <= 0.022
    assert 0.009 <= d[:, 2].std() <= 0.011


@pytest.mark.parametrize("n,seed", CASES)
def test_truth_is_a_grid_walk_from_the_origin(pgo, graphs, n, seed):
    _, _, truth = graphs[(n, seed)]
    assert truth.shape == (n, 3) and np.all(truth[0] == 0.0)
    step = np.abs(np.diff(truth[:, :2], axis=0))
    assert np.array_equal(np.sort(step, axis=1), np.tile([0.0, 1.0], (n - 1, 1)))      # one unit along one axis
    q = truth[:, 2] / (np.pi / 2)
    assert np.array_equal(q, np.round(q)) and set(np.unique(q)) <= {-1.0, 0.0, 1.0, 2.0}   # multiples of pi/2 in (-pi, pi]
    # a step goes along the heading held before it
    h = truth[:-1, 2]
    assert np.allclose(np.diff(truth[:, :2], axis=0), np.stack([np.cos(h), np.sin(h)], axis=1), atol=1e-15)
    # the walk does not depend on the edge budget or the outlier share, and the seed matters
    g2 = pgo.synth_manhattan(n, 2.0, 0.5, seed)
    assert np.array_equal(np.array(g2.poses), np.array(graphs[(n, seed)][1]))
    assert not np.array_equal(pgo.synth_manhattan_truth(n, seed + 1), truth)


def test_truth_errors(pgo):
    L = pgo.lib()
    out = np.zeros((4, 3))
    assert L.pgo_synth_manhattan_truth(1, 1, out.ctypes.data_as(pgo.C.POINTER(pgo.C.c_double))) == -1
    assert L.pgo_synth_manhattan_truth(4, 1, None) == -1
    assert np.all(out == 0.0)
    assert pgo.synth_manhattan_truth(2, 5).shape == (2, 3)


def test_generator_output_is_the_parents(pgo):
    """pgo_synth_manhattan returns bitwise what it returned before the walk moved into a function of its own"""
    ref = np.load(os.path.join(GOLDEN, "synth_manhattan_2000_s7.npz"))
    g = pgo.synth_manhattan(2000, 4.0, 0.1, 7)
    for k, a in (("poses", g.poses), ("ia", g.ia), ("ib", g.ib), ("meas", g.meas), ("kind", g.kind)):
        a = np.array(a)
        assert a.dtype == ref[k].dtype and a.shape == ref[k].shape and a.tobytes() == ref[k].tobytes(), k


# ------------------------------------------------------------------ trajectory error
@pytest.mark.parametrize("n,seed", CASES)
def test_trajectory_error_against_longdouble(pgo, graphs, n, seed):
    _, dead, truth = graphs[(n, seed)]
    rng = np.random.default_rng(100 + seed)
    masks = {"all": None, "random": rng.random(n) < 0.6, "none": np.zeros(n, bool), "one": np.arange(n) == n // 3}
    for mname, mask in masks.items():
        for align in (False, True):
            for delta in (1, 10, n):
                got, per = pgo.trajectory_error(dead, truth, mask=mask, align=align, rpe_delta=delta, per_pose=True)
                ref, rper = restate(dead, truth, mask, align, delta)
                what = (n, mname, align, delta)
                compare(got, ref, n, what)
                assert got["ate_max_pose"] == ref["ate_max_pose"] and got["rpe_max_pose"] == ref["rpe_max_pose"], what
                assert np.abs(per - rper).max() <= 8 * EPS * (np.abs(dead[:, :2]).max() + np.abs(truth[:, :2]).max() + np.pi), what
                if not align:
                    assert (got["align_x"], got["align_y"], got["align_phi"]) == (0.0, 0.0, 0.0)
                else:
                    assert abs(LD(got["align_x"]) - ref["align_x"]) <= 8 * n * EPS * (1 + np.abs(truth[:, :2]).max()), what
                if delta == n:
                    assert got["n_pairs"] == 0 and got["rpe_max_pose"] == -1 and got["rpe_trans_rmse"] == 0.0
                if mname == "none":
                    assert got["n_poses"] == 0 and got["ate_max_pose"] == -1 and all(got[k] == 0.0 for k in DOUBLES)
                    assert not per.any()
                if mname == "one":
                    assert got["n_poses"] == 1 and got["n_pairs"] == 0 and got["ate_max_pose"] == n // 3
                    if align:   # one pose fits exactly
                        assert got["ate_rmse"] <= 8 * EPS * (np.abs(truth[n // 3, :2]).max() + np.abs(dead[n // 3, :2]).max()) and got["align_phi"] == 0.0
    full = pgo.trajectory_error(dead, truth)
    assert full["n_poses"] == n and full["n_pairs"] == n - 1
    assert pgo.trajectory_error(dead, truth, align=True)["ate_rmse"] < full["ate_rmse"]


def test_single_pose_and_defaults(pgo):
    got, per = pgo.trajectory_error([[1.0, 2.0, 0.5]], [[1.5, 2.0, 0.25]], per_pose=True)
    assert got["n_poses"] == 1 and got["n_pairs"] == 0 and got["ate_rmse"] == 0.5 and got["ate_max_pose"] == 0 and got["rot_max"] == 0.25
    assert got["rpe_max_pose"] == -1 and per.tolist() == [[0.5, 0.25]]
    o = pgo.TrajOptions()
    assert (o.align, o.rpe_delta) == (0, 1) and pgo.C.sizeof(pgo.TrajOptions) == 8
    assert pgo.C.sizeof(pgo.TrajError) == 16 + 12 * 8 and pgo.C.sizeof(pgo.EdgeWeight) == 48
    # ties of a maximum go to the smallest index
    est = np.zeros((5, 3))
    ref = np.zeros((5, 3))
    ref[[1, 3], 0] = 2.0
    got = pgo.trajectory_error(est, ref, rpe_delta=0)
    assert got["ate_max_pose"] == 1 and got["ate_max"] == 2.0 and got["n_pairs"] == 0


def test_invariants(pgo, graphs):
    _, dead, truth = graphs[(2000, 7)]
    n = len(dead)
    th, t = 0.7, np.array([3.0, -11.0])
    c, s = np.cos(th), np.sin(th)
    moved = dead.copy()
    moved[:, 0] = c * dead[:, 0] - s * dead[:, 1] + t[0]
    moved[:, 1] = s * dead[:, 0] + c * dead[:, 1] + t[1]
    moved[:, 2] = dead[:, 2] + th
    scale = np.abs(moved[:, :2]).max() + np.abs(truth[:, :2]).max()
    for delta in (1, 10):
        a, b = pgo.trajectory_error(dead, truth, rpe_delta=delta), pgo.trajectory_error(moved, truth, rpe_delta=delta)
        assert a["n_pairs"] == b["n_pairs"] == n - delta
        for k in ("rpe_trans_rmse", "rpe_trans_max"):       # RPE does not see a rigid transform of the estimate
            assert abs(a[k] - b[k]) <= 64 * EPS * scale, (k, a[k], b[k])
        for k in ("rpe_rot_rmse", "rpe_rot_max"):
            assert abs(a[k] - b[k]) <= 64 * EPS * (np.abs(moved[:, 2]).max() + np.pi), (k, a[k], b[k])
        assert abs(a["ate_rmse"] - b["ate_rmse"]) > 1.0       # ... which the unaligned ATE does
    a, b = pgo.trajectory_error(dead, truth, align=True), pgo.trajectory_error(moved, truth, align=True)
    for k in ("ate_rmse", "ate_mean", "ate_max", "rot_rmse", "rot_max"):   # the aligned ATE does not see it either
        assert abs(a[k] - b[k]) <= 8 * n * EPS * scale, (k, a[k], b[k])
    assert abs(wrap(a["align_phi"] - b["align_phi"] - th)) <= 8 * n * EPS


def test_non_finite_and_bad_arguments(pgo, graphs):
    _, dead, truth = graphs[(300, 3)]
    for bad_val in (np.nan, np.inf):
        for which in (0, 1):
            est, ref = dead.copy(), truth.copy()
            (est if which == 0 else ref)[[41, 200], 1] = bad_val
            with pytest.raises(pgo.PgoError) as e:
                pgo.trajectory_error(est, ref)
            assert e.value.status == -7 and "pose 41 " in str(e.value)
            mask = np.ones(300, bool)
            mask[[41, 200]] = False
            got = pgo.trajectory_error(est, ref, mask=mask, align=True)      # a pose that is not counted may hold anything
            ref_d, _ = restate(dead, truth, mask, True, 1)
            compare(got, ref_d, 300, "masked-out non-finite pose")
    L = pgo.lib()
    dp = pgo.C.POINTER(pgo.C.c_double)
    e, r = dead.ctypes.data_as(dp), truth.ctypes.data_as(dp)
    out = pgo.TrajError()
    assert L.pgo_trajectory_error_eval(300, None, r, None, None, pgo.C.byref(out), None) == -1
    assert L.pgo_trajectory_error_eval(300, e, None, None, None, pgo.C.byref(out), None) == -1
    assert L.pgo_trajectory_error_eval(300, e, r, None, None, None, None) == -1
    assert L.pgo_trajectory_error_eval(0, e, r, None, None, pgo.C.byref(out), None) == -1
    for kw in (dict(align=2), dict(align=-1), dict(rpe_delta=-1)):
        o = pgo.TrajOptions(**kw)
        assert L.pgo_trajectory_error_eval(300, e, r, None, pgo.C.byref(o), pgo.C.byref(out), None) == -1
    assert L.pgo_trajectory_error_eval(300, e, r, None, None, pgo.C.byref(out), None) == 0 and out.n_poses == 300   # NULL options: the defaults
    assert out.n_pairs == 299


# ------------------------------------------------------------------ the classification thresholds of test_gpu_score.py
@pytest.mark.parametrize("method", [0, 1])
def test_classification_threshold_is_clear_of_every_oracle_weight(pgo, method):
    """INTEL + 50 seeded outliers at the oracle's final poses: no restated weight lies within 1e-3 of the threshold, so that
    the pose-parity bound of the GPU solve (5e-6) cannot move an edge across it; METHOD 1 turns every bogus loop down"""
    import _score_cases as SC
    g = SC.intel50(pgo)
    w = SC.restate_weights(g, SC.oracle_final_poses(method), method)["weight"]
    kind = np.array(g.kind)
    gap = np.abs(w - SC.TAU[method]).min()
    below = w < SC.TAU[method]
    print("method %d tau %g: %d edges below (%d of %d bogus), nearest weight %.3e away" % (method, SC.TAU[method], below.sum(), below[kind == 2].sum(), (kind == 2).sum(), gap))
    assert gap > SC.TAU_GAP
    assert np.all(w[kind == 0] <= 1.0) and 0 < below.sum() < len(w)
    if method == 1:
        assert below[kind == 2].all() and below.sum() == (kind == 2).sum() == 50
