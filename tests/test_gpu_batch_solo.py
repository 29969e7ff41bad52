"""The batched one-workgroup PCG solve (k_pcg_solo, csrc/solo.hip.h) as an operator, through pgo_batch_debug_solve, against
the numpy restatement of _solo_cases.py (itself checked on the CPU in test_solo_restatement.py).

One Batch per chain length L in {0, 4, 8, 16, 32, 64, 128, 256} holds the eleven accepted cases in a fixed order (each
reaches a branch of solo.hip.h, _solo_cases.CASES); one METHOD 1 batch (L = 64, with the outlier case appended) and one
batch without constant poses (L = 32) besides.  Criteria:
  (a) truncated iterates y_k, k in {1, 2, 3, 8}, radius 1, rtol 0, on a fixed random right-hand side and on the gradient:
      iters == k, done == 0, |y_dev - y_k| <= 10 spread_k + eps 3n kappa |y_k|_inf (per group of rows, _solo_cases.rows());
      k = 1 also backward, per chain segment, and alpha against the device's own direction
  (b) converged solves, radius 1e4, rtol 1e-9: done, the recurrence residual, the TRUE residual in the restated system in
      np.longdouble, iteration counts against the restatement's
  (c) the epilogue sums against np.longdouble sums over the device's own y, on every run of (a) and (b): rounding alone
      (3n eps) on a right-hand side that was passed in; under the gradient, which is the device's own, y.b and b.b also
      admit the restatement's change of b under the Jacobian disagreement (epilogue())
  (d) max_it = 0 and zero right-hand sides beside running neighbours
  (e) a problem alone in a batch returns what it returns in the bundle
  (f) a row of 256 incidences is accepted, 257 refused
  (g) one LM iteration through Batch.solve() against a dense solve of the restated system; the hook leaves no trace
Every test prints its worst ratio to the bound per criterion."""
import ctypes as C

import numpy as np
import pytest

import _solo_cases as SC

pytestmark = pytest.mark.gpu

BE_ONE = 1e-10     # one-level backward error (test_gpu_precond.py)
PROD = 1e-11       # relative share of a product with the restated H (test_gpu_precond.py)
EPS = SC.EPS
LD = np.longdouble
KS = (1, 2, 3, 8)
RTOL_B, RADIUS_B, MAXIT_B = 1e-9, 1e4, 100000

# id: (L, method, fixed_pose, cases)
CONFIGS = {("L%d" % L): (L, 0, 0, SC.ORDER) for L in SC.CHAIN_LENS}
CONFIGS["L64-method1"] = (64, 1, 0, SC.ORDER + ("w257_bogus",))
CONFIGS["L32-nofixed"] = (32, 0, -1, SC.ORDER)
ALONE = ("five", "w257", "w2049")
for _n in ALONE:
    CONFIGS["L64-alone-" + _n] = (64, 0, 0, (_n,))

BATCHES, RUNS = {}, {}


def options(pgo, L, method, fixed_pose, **kw):
    o = dict(method=method, fixed_pose=fixed_pose, pcg_chain_len=L, **kw)
    if L == 0:
        o["pcg_block_poses"] = 1
    return pgo.Options(**o)


def batch(pgo, cfg):
    if cfg not in BATCHES:
        L, method, fixed_pose, names = CONFIGS[cfg]
        BATCHES[cfg] = pgo.Batch([SC.pgo_graph(pgo, n) for n in names], options(pgo, L, method, fixed_pose))
    return BATCHES[cfg]


@pytest.fixture(scope="module", autouse=True)
def close_batches():
    yield
    for b in BATCHES.values():
        b.close()
    BATCHES.clear()
    RUNS.clear()


def rhs_of(O, cfg, kind, radius):
    L, method, fixed_pose, names = CONFIGS[cfg]
    return [SC.random_rhs(SC.system(O, n, radius, method, fixed_pose)) for n in names] if kind == "random" else None


def run(pgo, O, cfg, radius, max_it, rtol, kind):
    """one launch of the hook (cached): ([y per problem], [result dict per problem])"""
    key = (cfg, radius, max_it, rtol, kind)
    if key not in RUNS:
        RUNS[key] = batch(pgo, cfg).debug_solve(radius, max_it, rtol, rhs_of(O, cfg, kind, radius))
    return RUNS[key]


class Worst(dict):
    def see(self, what, ratio, where):
        if ratio > self.get(what, (-1.0, None))[0]:
            self[what] = (float(ratio), where)

    def show(self, title):
        print(title, {k: ("%.2e" % v[0], v[1]) for k, v in self.items()})

    def check(self):
        """every criterion within its bound; the "(+10 spread)" entries are printed only"""
        bad = {k: v for k, v in self.items() if not v[0] <= 1.0 and "(+" not in k}
        assert not bad, bad


def ratio(err, bound):
    """max err / bound; where the bound is 0 the error must be 0"""
    err, bound = np.atleast_1d(np.asarray(err, np.float64)), np.atleast_1d(np.asarray(bound, np.float64))
    zero = bound == 0.0
    if np.any(err[zero] != 0.0) or not np.isfinite(err).all():
        return np.inf
    return float(np.max(err[~zero] / bound[~zero])) if (~zero).any() else 0.0


def segment_max(v, blk, nb):
    out = np.zeros(nb)
    np.maximum.at(out, blk, np.abs(v))
    return out


def epilogue(W, where, sysm, b, db, y, res):
    """(c): the sums of the step's epilogue from the device's own y, in np.longdouble.  b is the restatement's right-hand
    side.  A right-hand side that was passed in is the device's bit for bit: db = 0 and the bounds are rounding alone.  The
    gradient is the device's own sum J'r: it differs from the restatement's by the admitted Jacobian disagreement, db per
    entry (10 x the largest change of b over the restatement's reruns with every Jacobian entry moved by 1e-11), carried
    through y.b and b.b to first order.  (Without that share the plain 3n eps bound was missed under the gradient on the
    MI355X: bb of `five` without a constant pose 3.9e-15 relative against 15 eps = 3.3e-15 -- the two gradients differ in
    their last bits; with it the worst ratio is 6e-4.)"""
    n3 = sysm.n3
    yl, bl = y.astype(LD), b.astype(LD)
    ay = np.abs(y)
    W.see("ydotg", ratio(abs(float(yl @ bl) - res["ydotg"]), n3 * EPS * float(ay @ np.abs(b)) + float(ay @ db)), where)
    sy = sysm.s.astype(LD) * yl
    W.see("step2", ratio(abs(float(sy @ sy) - res["step2"]), n3 * EPS * res["step2"]), where)
    W.see("bb", ratio(abs(float(bl @ bl) - res["bb"]), n3 * EPS * res["bb"] + 2.0 * float(np.abs(b) @ db)), where)
    Hy = sysm.H.astype(LD) @ yl
    W.see("yHy", ratio(abs(float(yl @ Hy) - res["yHy"]), (n3 * EPS + PROD) * float(ay @ (abs(sysm.H) @ ay))), where)


def gradient_spread(O, name, L, kind, method, fixed_pose, radius):
    key = (name, radius, method, fixed_pose)
    if kind == "random":
        return np.zeros(SC.system(O, *key).n3)
    if key not in SC.B_SPREAD:
        SC.spread(O, name, L, radius, "gradient", method, fixed_pose)
    return 10.0 * SC.B_SPREAD[key]


def one_iteration(O, name, L, kind, method, fixed_pose):
    return SC.reference(O, name, L, 1.0, 1e-9, 100, kind, method, fixed_pose)[3].iters == 1


def truncated(W, O, cfg, name, k, kind, y, res):
    """(a) and (c) for one problem of one run"""
    L, method, fixed_pose, _ = CONFIGS[cfg]
    where = (name, k, kind)
    sysm, M, b, ref = SC.reference(O, name, L, 1.0, 0.0, 8, kind, method, fixed_pose)
    assert np.isfinite(y).all(), where
    epilogue(W, where, sysm, b, gradient_spread(O, name, L, kind, method, fixed_pose, 1.0), y, res)
    if k >= 2 and one_iteration(O, name, L, kind, method, fixed_pose):
        return
    assert res["iters"] == k and res["done"] == 0, (where, res)
    y_k = ref.ys[k - 1]
    bound = SC.iterate_bound(sysm, y_k, SC.spread(O, name, L, 1.0, kind, method, fixed_pose)[k - 1])
    for m, bd in zip(sysm.rows(), bound):
        W.see("iterate", ratio(np.abs(y - y_k)[m].max(), bd), where)
    if k == 1:
        # conditioning-free: y_1 = alpha M^-1 b.  alpha^ from the device's y through the restated M, the backward error of
        # z per segment, and alpha^ against (b.z) / (z.A z) of the device's own direction z
        My = M.M1 @ y
        ah = float(b @ My) / float(b @ b)
        rows = np.asarray(abs(M.M1).sum(axis=1)).reshape(-1)
        nb = M.n_blocks
        den = segment_max(rows, M.blk, nb) * segment_max(y, M.blk, nb) + segment_max(ah * b, M.blk, nb)
        num = segment_max(My - ah * b, M.blk, nb)
        W.see("backward", ratio(num, BE_ONE * den), where)
        z, bl = y.astype(LD) / LD(ah), b.astype(LD)
        Az = sysm.A.astype(LD) @ z
        bz, zAz = float(bl @ z), float(z @ Az)
        tol = sysm.n3 * EPS * (float(np.abs(bl * z).sum()) / abs(bz) + float(np.abs(z * Az).sum()) / abs(zAz))
        a_err = abs(ah - bz / zAz) / abs(bz / zAz)
        W.see("alpha", ratio(a_err, tol), where)
        W.see("alpha/(+10 spread)", ratio(a_err, tol + 10.0 * SC.ALPHA_SPREAD[(name, L, 1.0, kind, method, fixed_pose, 8)]), where)


def converged(W, O, cfg, name, kind, y, res):
    """(b) and (c) for one problem of one run.  Returns (device iterations, restatement's)"""
    L, method, fixed_pose, _ = CONFIGS[cfg]
    where = (name, kind)
    sysm, M, b, ref = SC.reference(O, name, L, RADIUS_B, RTOL_B, MAXIT_B, kind, method, fixed_pose)
    assert np.isfinite(y).all(), where
    assert res["done"] == 1 and res["rr"] <= RTOL_B ** 2 * res["bb"], (where, res)
    epilogue(W, where, sysm, b, gradient_spread(O, name, L, kind, method, fixed_pose, RADIUS_B), y, res)
    yl, bl = y.astype(LD), b.astype(LD)
    true = float(np.sqrt(np.sum((bl - sysm.A.astype(LD) @ yl) ** 2)))
    bn = float(np.linalg.norm(b))
    W.see("residual", ratio(true, 2.0 * RTOL_B * bn + BE_ONE * (float(np.linalg.norm(abs(sysm.A) @ np.abs(y))) + bn)), where)
    if ref.iters == 1:
        assert res["iters"] == 1, (where, res)
    W.see("iterations", ratio(abs(res["iters"] - ref.iters), max(2.0, 0.06 * ref.iters)), where)
    return res["iters"], ref.iters


MAIN = [c for c in CONFIGS if "alone" not in c]


@pytest.mark.parametrize("cfg", MAIN)
def test_truncated_iterates_match_the_restatement(pgo, oracle, cfg):
    W = Worst()
    names = CONFIGS[cfg][3]
    for kind in ("random", "gradient"):
        for k in KS:
            ys, res = run(pgo, oracle, cfg, 1.0, k, 0.0, kind)
            for name, y, r in zip(names, ys, res):
                truncated(W, oracle, cfg, name, k, kind, y, r)
    W.show(cfg + " (a), (c):")
    W.check()


@pytest.mark.parametrize("cfg", MAIN)
def test_converged_solves_match_the_restatement(pgo, oracle, cfg):
    W = Worst()
    names = CONFIGS[cfg][3]
    counts = {}
    for kind in ("gradient", "random"):
        ys, res = run(pgo, oracle, cfg, RADIUS_B, MAXIT_B, RTOL_B, kind)
        for name, y, r in zip(names, ys, res):
            counts[(name, kind)] = converged(W, oracle, cfg, name, kind, y, r)
    W.show(cfg + " (b), (c):")
    print(cfg, "iterations device / restatement (gradient):", {n: "%d / %d" % counts[(n, "gradient")] for n in names})
    W.check()


@pytest.mark.parametrize("cfg", MAIN)
def test_degenerate_entries(pgo, oracle, cfg):
    L, method, fixed_pose, names = CONFIGS[cfg]
    b = batch(pgo, cfg)
    rhs = rhs_of(oracle, cfg, "random", 1.0)
    ys, res = b.debug_solve(1.0, 0, 0.0, rhs)
    for name, y, r in zip(names, ys, res):
        assert not y.any(), name
        assert r["iters"] == 0 and r["done"] == 0 and r["ydotg"] == 0.0 and r["yHy"] == 0.0 and r["step2"] == 0.0, (name, r)
        assert r["bb"] > 0.0 and r["rr"] == r["bb"], (name, r)
    # zero right-hand sides beside running neighbours
    zero = ("two", "chain130", "w2049")
    ys0, res0 = run(pgo, oracle, cfg, 1.0, 3, 0.0, "random")
    ys, res = b.debug_solve(1.0, 3, 0.0, [np.zeros_like(v) if n in zero else v for n, v in zip(names, rhs)])
    for name, y, r, y0, r0 in zip(names, ys, res, ys0, res0):
        if name in zero:
            assert not y.any(), name
            assert r["iters"] == 0 and r["done"] == 1, (name, r)
            assert all(np.isfinite(v) for v in r.values()) and r["bb"] == 0.0 and r["ydotg"] == 0.0 and r["yHy"] == 0.0, (name, r)
        else:
            np.testing.assert_array_equal(y, y0, err_msg=name)
            assert r == r0, (name, r, r0)


@pytest.mark.parametrize("name", ALONE)
def test_neighbours_do_not_matter(pgo, oracle, name):
    """A problem alone in a batch of its own (L = 64) against the same problem in the bundle: the same iteration counts, every
    criterion of (a) and (b) -- and on the MI355X the very same numbers: a workgroup reads and writes its own problem's rows
    only, the row tiles and chain tiles of a problem do not depend on its neighbours, hence array_equal."""
    W = Worst()
    cfg, i = "L64-alone-" + name, CONFIGS["L64"][3].index(name)
    worst = 0.0
    for kind in ("random", "gradient"):
        for k in KS:
            (y,), (r,) = run(pgo, oracle, cfg, 1.0, k, 0.0, kind)
            truncated(W, oracle, cfg, name, k, kind, y, r)
            ys, res = run(pgo, oracle, "L64", 1.0, k, 0.0, kind)
            worst = max(worst, float(np.abs(y - ys[i]).max()))
            assert r["iters"] == res[i]["iters"]
            np.testing.assert_array_equal(y, ys[i])
        (y,), (r,) = run(pgo, oracle, cfg, RADIUS_B, MAXIT_B, RTOL_B, kind)
        converged(W, oracle, cfg, name, kind, y, r)
        ys, res = run(pgo, oracle, "L64", RADIUS_B, MAXIT_B, RTOL_B, kind)
        worst = max(worst, float(np.abs(y - ys[i]).max()))
        assert r["iters"] == res[i]["iters"], (r, res[i])
        np.testing.assert_array_equal(y, ys[i])
        assert r == res[i]
    W.show(name + " alone (a), (b), (c):")
    print(name, "largest |y_alone - y_bundle| = %.3e" % worst)
    W.check()


def test_a_row_of_257_incidences_is_refused(pgo):
    """(f): hub256 is part of every bundle above; one more incident edge is PGO_ERR_UNSUPPORTED, alone or in a bundle, and the
    refusal leaves no handle"""
    L = pgo.lib()
    for names in (("hub257",), ("five", "hub257", "w255"), ("hub256", "hub257")):
        graphs = [SC.pgo_graph(pgo, n) for n in names]
        hs = (C.c_void_p * len(graphs))(*[g._h for g in graphs])
        h = C.c_void_p()
        opt = options(pgo, 64, 0, 0)
        assert L.pgo_batch_create(C.byref(h), len(graphs), hs, C.byref(opt), 0) == -8, names
        assert h.value is None, names
        with pytest.raises(pgo.PgoError) as e:
            pgo.Batch(graphs, opt)
        assert e.value.status == -8
    b = pgo.Batch([SC.pgo_graph(pgo, "hub256")], options(pgo, 64, 0, 0))   # the accepted side, alone
    b.close()


def test_the_hook_refuses_bad_arguments(pgo, oracle):
    b = batch(pgo, "L64-alone-five")
    L = pgo.lib()
    y = np.zeros(15)
    res = (pgo.SoloResult * 1)()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ok = (1.0, 3, 0.0)
    assert L.pgo_batch_debug_solve(b._h, *ok, None, dp(y), res) == 0
    assert L.pgo_batch_debug_solve(None, *ok, None, dp(y), res) == -1
    assert L.pgo_batch_debug_solve(b._h, *ok, None, None, res) == -1
    assert L.pgo_batch_debug_solve(b._h, *ok, None, dp(y), None) == -1
    for bad in ((0.0, 3, 0.0), (-1.0, 3, 0.0), (np.inf, 3, 0.0), (np.nan, 3, 0.0), (1.0, -1, 0.0), (1.0, 1000001, 0.0),
                (1.0, 3, -1e-3), (1.0, 3, np.nan), (1.0, 3, np.inf)):
        with pytest.raises(pgo.PgoError) as e:
            b.debug_solve(*bad)
        assert e.value.status == -1, bad


def strip(recs):
    return [{k: v for k, v in r.items() if k != "seconds"} for r in recs]


@pytest.mark.parametrize("L", [4, 32, 128])
def test_one_lm_iteration_through_the_public_path(pgo, oracle, L):
    """(g): Batch.solve() with max_iters = 1 and an exact inner solve against one restated LM iteration (dense solve of the
    restated system at the initial radius); and the hook leaves the state alone"""
    O = oracle
    names = [n for n in SC.ORDER if len(SC.arrays(n)["poses"]) <= SC.DENSE_MAX_POSES]
    rtol = 1e-12
    kw = dict(max_iters=1, pcg_rtol=rtol, pcg_max_iters=100000, ftol=0.0, ptol=0.0, gtol=0.0)
    opt = options(pgo, L, 0, 0, **kw)
    graphs = [SC.pgo_graph(pgo, n) for n in names]
    touched, fresh = pgo.Batch(graphs, opt), pgo.Batch(graphs, opt)
    touched.debug_solve(1.0, 5, 0.0, [SC.random_rhs(SC.system(O, n, 1.0)) for n in names])
    touched.debug_solve(RADIUS_B, 50, 1e-3)
    touched.solve()
    fresh.solve()
    W = Worst()
    for k, name in enumerate(names):
        np.testing.assert_array_equal(touched.poses(k), fresh.poses(k), err_msg=name)
        assert strip(touched.iter_records(k)) == strip(fresh.iter_records(k)), name
        recs = fresh.iter_records(k)
        assert len(recs) == 2, (name, recs)
        rec = recs[1]
        sysm = SC.system(O, name, opt.radius0)
        kap = SC.kappa(sysm)
        tol = kap * (rtol + PROD)
        c = sysm.coupled
        y = np.zeros(sysm.n3)
        y[c] = np.linalg.solve(sysm.A[c][:, c].toarray(), sysm.b[c])     # (b is 0 on the diagonal-only rows)
        step = sysm.s * y
        model = float(y @ sysm.b - 0.5 * (y @ (sysm.H @ y)))
        g = SC.oracle_graph(O, name)
        x = g.poses.reshape(-1)
        cost0 = O.evaluate(g, g.poses, 0, want_r=False, want_J=False)[0]
        cand = O.evaluate(g, (x - step).reshape(-1, 3), 0, want_r=False, want_J=False)[0]
        ok = int((cost0 - cand) / model > opt.min_relative_decrease)
        assert rec["step_ok"] == ok, (name, rec)
        W.see("step_norm", ratio(abs(rec["step_norm"] - np.linalg.norm(step)), tol * np.linalg.norm(step)), name)
        W.see("model decrease", ratio(abs(rec["cost_change"] / rec["relative_decrease"] - model), tol * abs(model)), name)
        if ok:
            W.see("poses", ratio(np.abs(fresh.poses(k).reshape(-1) - (x - step)),
                                 tol * np.abs(step).max() + EPS * np.abs(x)), name)
        else:
            np.testing.assert_array_equal(fresh.poses(k), g.poses, err_msg=name)
    touched.close()
    fresh.close()
    W.show("L%d (g):" % L)
    W.check()
