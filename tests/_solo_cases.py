"""Cases and numpy restatement for the one-workgroup PCG solve of a batch (csrc/solo.hip.h, pgo_batch_debug_solve).

Plain numpy / scipy on top of oracle.lm_system / oracle.Precond, importable without a GPU: test_solo_restatement.py checks
the restatement and the caps the GPU criteria rest on; test_gpu_batch_solo.py judges the kernel by it.

Every case is a small synthetic graph whose pose count is chosen for a branch of solo.hip.h (CASES below).  A problem of a
batch starts on a 256-row boundary, so its chain segments of L poses and its 256-row chain tiles are those of the problem
alone: the restatement of problem k is built on problem k only.

Conditioning: a pose without edges and the constant pose are rows of A = H + diag(d2) with nothing off the diagonal (H is
0 there, d2 = min_lm_diagonal / radius resp. 1).  Every preconditioner here contains the diagonal, so PCG solves those rows
exactly in its first iteration whatever their size; kappa() is therefore taken over the COUPLED rows (nonzero H diagonal),
and the comparisons of iterates use the two groups of rows with their own norms (rows())."""
import functools

import numpy as np

CHAIN_LENS = (0, 4, 8, 16, 32, 64, 128, 256)
ORDER = ("w4100", "two", "w2049", "five", "chain130", "w255", "w256", "w257", "gaps300", "awkward", "hub256")
DENSE_MAX_POSES = 1100       # kappa by dense eigvalsh up to here, by the row-sum bound above
DJ = 1e-11                   # |J_device - J_oracle| per entry that test_edge_kernel_parity asserts at the initial poses
EPS = float(np.finfo(np.float64).eps)


def wrap(a):
    return (a + np.pi) % (2.0 * np.pi) - np.pi


def relative(truth, a, b):
    """measurement of pose b in the frame of pose a"""
    d = truth[b, :2] - truth[a, :2]
    c, s = np.cos(truth[a, 2]), np.sin(truth[a, 2])
    return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], wrap(truth[b, 2] - truth[a, 2])], axis=1)


def draw_loops(rng, n, n_loops, ok=lambda a, b: True):
    out = []
    while len(out) < n_loops:
        a, b = sorted(int(v) for v in rng.integers(0, n, 2))
        if b - a >= 2 and ok(a, b):
            out.append((a, b))
    return np.array(out, np.int32).reshape(-1, 2)


def truth_walk(rng, n):
    """headings: cumulative sums of draws from {0, 0, 0, +pi/2, -pi/2}; unit steps"""
    turn = rng.choice(np.array([0.0, 0.0, 0.0, np.pi / 2, -np.pi / 2]), size=n)
    turn[0] = 0.0
    th = np.cumsum(turn)
    xy = np.zeros((n, 2))
    xy[1:] = np.cumsum(np.stack([np.cos(th[:-1]), np.sin(th[:-1])], axis=1), axis=0)
    return np.concatenate([xy, th[:, None]], axis=1)


def finish(rng, truth, ia, ib, kind):
    """dict of arrays: measurements = true relative pose + 0.01 N(0,1), start = truth + 0.02 N(0,1); edges sorted by kind"""
    ia, ib, kind = np.asarray(ia, np.int32), np.asarray(ib, np.int32), np.asarray(kind, np.uint8)
    meas = relative(truth, ia, ib) + 0.01 * rng.standard_normal((len(ia), 3))
    poses = truth + 0.02 * rng.standard_normal(truth.shape)
    o = np.argsort(kind, kind="stable")
    return dict(poses=poses, ia=ia[o], ib=ib[o], meas=meas[o], kind=kind[o])


def walk(n, n_loops, seed):
    """the graph recipe: odometry i -> i+1, n_loops closures between uniformly drawn poses with |a - b| >= 2"""
    rng = np.random.default_rng(seed)
    truth = truth_walk(rng, n)
    lp = draw_loops(rng, n, n_loops)
    ia = np.concatenate([np.arange(n - 1), lp[:, 0]])
    ib = np.concatenate([np.arange(1, n), lp[:, 1]])
    kind = np.concatenate([np.zeros(n - 1), np.ones(len(lp))])
    return finish(rng, truth, ia, ib, kind)


def gaps300():
    """n = 300: poses 20..279 without edges; 0..19 and 280..299 are two halves of a 40-pose walk, not joined to each other
    (the second has no constant pose), 10 closures inside the halves"""
    rng = np.random.default_rng(300)
    t40 = truth_walk(rng, 40)
    pos = np.concatenate([np.arange(20), np.arange(280, 300)])
    truth = np.zeros((300, 3))
    truth[:, 0] = -5.0 - 0.5 * np.arange(300)      # the edge-less poses: anywhere
    truth[pos] = t40
    lp = draw_loops(rng, 40, 10, ok=lambda a, b: (a < 20) == (b < 20))
    odo = np.array([i for i in range(39) if i != 19])
    ia = pos[np.concatenate([odo, lp[:, 0]])]
    ib = pos[np.concatenate([odo + 1, lp[:, 1]])]
    return finish(rng, truth, ia, ib, np.concatenate([np.zeros(len(odo)), np.ones(len(lp))]))


def awkward():
    """w257 with the odometry edge 100-101 removed (C = 0 inside a segment), 150-151 tripled (k_chain_dupfix), 200-201 reversed
    (a > b) and a closure-kind edge 220-221 between consecutive poses"""
    g = walk(257, 60, 257)
    rng = np.random.default_rng(2570)
    ia, ib, meas, kind = (g[k].copy() for k in ("ia", "ib", "meas", "kind"))
    e150 = int(np.nonzero((ia == 150) & (ib == 151))[0][0])
    e200 = int(np.nonzero((ia == 200) & (ib == 201))[0][0])
    e220 = int(np.nonzero((ia == 220) & (ib == 221))[0][0])
    # reversed: the inverse measurement
    x, y, t = meas[e200]
    ia[e200], ib[e200] = 201, 200
    meas[e200] = [-(np.cos(t) * x + np.sin(t) * y), -(-np.sin(t) * x + np.cos(t) * y), -t]
    add = [e150, e150, e220]
    ia, ib = np.concatenate([ia, ia[add]]), np.concatenate([ib, ib[add]])
    meas = np.concatenate([meas, meas[add] + 0.01 * rng.standard_normal((3, 3))])
    kind = np.concatenate([kind, [0, 0, 1]]).astype(np.uint8)
    keep = ~((ia == 100) & (ib == 101))
    o = np.argsort(kind[keep], kind="stable")
    return dict(poses=g["poses"], ia=ia[keep][o], ib=ib[keep][o], meas=meas[keep][o], kind=kind[keep][o])


HUB = 200


def hub(incidences):
    """n = 400 walk, 20 closures away from pose HUB, plus closures that bring HUB to `incidences` incident edges"""
    def spokes(rng, n):
        far = np.array([i for i in range(n) if abs(i - HUB) >= 2])
        return [(min(HUB, int(j)), max(HUB, int(j))) for j in rng.choice(far, incidences - 2, replace=False)]
    rng = np.random.default_rng(400)
    truth = truth_walk(rng, 400)
    lp = np.concatenate([draw_loops(rng, 400, 20, ok=lambda a, b: HUB not in (a, b)), np.array(spokes(rng, 400), np.int32)])
    ia = np.concatenate([np.arange(399), lp[:, 0]])
    ib = np.concatenate([np.arange(1, 400), lp[:, 1]])
    return finish(rng, truth, ia, ib, np.concatenate([np.zeros(399), np.ones(len(lp))]))


def w257_bogus():
    """the METHOD 1 case: w257 with 25 closures overwritten by random measurements and kind 2"""
    g = walk(257, 60, 257)
    rng = np.random.default_rng(2571)
    lp = np.nonzero(g["kind"] == 1)[0]
    bad = rng.choice(lp, 25, replace=False)
    meas, kind = g["meas"].copy(), g["kind"].copy()
    meas[bad] = np.stack([rng.uniform(-10, 10, 25), rng.uniform(-10, 10, 25), rng.uniform(-np.pi, np.pi, 25)], axis=1)
    kind[bad] = 2
    o = np.argsort(kind, kind="stable")
    return dict(poses=g["poses"], ia=g["ia"][o], ib=g["ib"][o], meas=meas[o], kind=kind[o])


# case: (builder, the branch of solo.hip.h it reaches)
CASES = {
    "two": (lambda: walk(2, 0, 2), "chain tile with rows_here = 2; one product tile of 2 + 254 padding rows (three passes)"),
    "five": (lambda: walk(5, 2, 5), "a problem shorter than one 4-pose lane chunk plus one"),
    "chain130": (lambda: walk(130, 0, 130), "128-row tile: second pass of solo_spmv; chain length 256: M = A"),
    "w255": (lambda: walk(255, 60, 255), "problem end one row before the 256-row chain tile's"),
    "w256": (lambda: walk(256, 60, 256), "problem end on the 256-row chain tile's"),
    "w257": (lambda: walk(257, 60, 257), "a second chain tile of one row"),
    "gaps300": (gaps300, "256-row tile without incidences (three passes), a component without a constant pose"),
    "awkward": (awkward, "C = 0 inside a segment, k_chain_dupfix in a batch, a > b, a closure on the chain"),
    "hub256": (lambda: hub(256), "a row of exactly 256 incidences"),
    "w2049": (lambda: walk(2049, 600, 2049), "9 chain tiles: wave 0 takes a second one of one row; ragged product rounds"),
    "w4100": (lambda: walk(4100, 1500, 4100), "17 chain tiles: three trips of the waves"),
    "w257_bogus": (w257_bogus, "METHOD 1: 25 outlier closures of kind 2"),
    "hub257": (lambda: hub(257), "refused: a row of 257 incidences"),
}


@functools.lru_cache(maxsize=None)
def arrays(name):
    return CASES[name][0]()


def oracle_graph(O, name):
    a = arrays(name)
    n, e = len(a["poses"]), len(a["ia"])
    info = np.tile(np.array([1.0, 0, 0, 1.0, 0, 1.0]), (e, 1))
    return O.Graph(np.arange(n, dtype=np.int32), a["poses"].copy(), a["ia"], a["ib"], a["meas"], info, a["kind"])


def pgo_graph(pgo, name):
    a = arrays(name)
    return pgo.Graph.from_arrays(a["poses"], a["ia"], a["ib"], a["meas"], a["kind"])


# ------------------------------------------------------------------------------------------------ the restated system
class System:
    """A = H + diag(d2), b (the scaled gradient), s, H, and what the perturbed copies need (JS, r, radius, fixed_pose)"""

    def __init__(self, O, name, H, d2, b, s, JS, r, radius, fixed_pose, poses):
        import scipy.sparse as sp
        self.O, self.name, self.H, self.d2, self.b, self.s, self.JS, self.r = O, name, H.tocsr(), d2, b, s, JS, r
        self.radius, self.fixed_pose, self.poses = radius, fixed_pose, poses
        self.A = (self.H + sp.diags(d2)).tocsr()
        self.n3 = len(b)
        self.coupled = self.H.diagonal() != 0.0

    def rows(self):
        """the two groups of rows compared with their own norms: coupled, and diagonal-only (edge-less / constant poses)"""
        return [m for m in (self.coupled, ~self.coupled) if m.any()]

    def precond(self, L):
        return self.O.Precond(self, self.poses, block_poses=1, chain_len=L)

    def perturbed(self, seed):
        """every stored Jacobian entry moved by +-DJ (random signs); scales, residuals and radius kept"""
        import scipy.sparse as sp
        rng = np.random.default_rng(seed)
        J = self.JS.tocsc(copy=True)
        scol = np.repeat(self.s, np.diff(J.indptr))
        J.data = J.data + DJ * rng.choice(np.array([-1.0, 1.0]), size=len(J.data)) * scol
        J = J.tocsr()
        H = (J.T @ J).tocsr()
        d2 = np.clip(H.diagonal(), 1e-6, 1e32) / self.radius
        if self.fixed_pose >= 0:
            d2[3 * self.fixed_pose:3 * self.fixed_pose + 3] = 1.0
        return System(self.O, self.name, H, d2, J.T @ self.r, self.s, J, self.r, self.radius, self.fixed_pose, self.poses)


_SYS = {}


def system(O, name, radius, method=0, fixed_pose=0):
    """oracle.lm_system at the case's start poses (Jacobi scales from the same Jacobian, as at a solve's start)"""
    key = (name, radius, method, fixed_pose)
    if key not in _SYS:
        g = oracle_graph(O, name)
        m = O.lm_system(g, g.poses, g.poses, radius, method=method, fixed_pose=fixed_pose)
        _, r, _ = O.evaluate(g, g.poses, method, want_J=False)
        _SYS[key] = System(O, name, m.H, m.d2, m.b, m.s, m.JS, r.reshape(-1), radius, fixed_pose, g.poses)
    return _SYS[key]


def random_rhs(sysm, seed=12345):
    """a fixed random vector, zero on the constant pose"""
    v = np.random.default_rng(seed + sysm.n3).standard_normal(sysm.n3)
    v[sysm.s == 0.0] = 0.0
    return v


class Pcg:
    pass


def pcg(A, M, b, max_it, rtol, keep=8):
    """textbook PCG from y = 0 in the update order of the kernels.  Returns: iters, done, the iterates y[1..min(iters, keep)]
    (list index k - 1), y (the last iterate), rr (recurrence |r|^2), bb, alpha1"""
    out = Pcg()
    y = np.zeros_like(b)
    r = b.copy()
    out.bb = float(b @ b)
    out.rr = out.bb
    out.iters, out.done, out.ys, out.alpha1 = 0, int(out.bb == 0.0), [], None
    if not out.done and max_it > 0:
        z = M.apply1(r)
        p = z.copy()
        rz = float(r @ z)
        tol2 = rtol * rtol * out.bb
        while out.iters < max_it:
            Ap = A @ p
            alpha = rz / float(p @ Ap)
            y = y + alpha * p
            r = r - alpha * Ap
            out.iters += 1
            if out.iters == 1:
                out.alpha1 = alpha
            if out.iters <= keep:
                out.ys.append(y.copy())
            out.rr = float(r @ r)
            if out.rr <= tol2:
                out.done = 1
                break
            z = M.apply1(r)
            rz2 = float(r @ z)
            p = z + (rz2 / rz) * p
            rz = rz2
    out.y = y
    return out


_KAPPA = {}


def kappa(sysm):
    """cond_2 of A on the coupled rows: dense eigvalsh up to DENSE_MAX_POSES poses; above, the upper bound (largest absolute
    row sum of A) / (smallest d2 there) -- H is positive semi-definite, so lambda_min(A) >= min d2"""
    key = (sysm.name, sysm.radius, sysm.fixed_pose, float(sysm.d2.sum()))
    if key not in _KAPPA:
        c = sysm.coupled
        A = sysm.A[c][:, c]
        if sysm.n3 <= 3 * DENSE_MAX_POSES:
            w = np.linalg.eigvalsh(A.toarray())
            _KAPPA[key] = float(w[-1] / w[0])
        else:
            _KAPPA[key] = float(np.asarray(abs(A).sum(axis=1)).max() / sysm.d2[c].min())
    return _KAPPA[key]


_REF = {}


def reference(O, name, L, radius, rtol, max_it, rhs="random", method=0, fixed_pose=0, keep=8):
    """the restated solve of a case (cached): (System, Precond, b, Pcg)"""
    key = (name, L, radius, rtol, max_it, rhs, method, fixed_pose, keep)
    if key not in _REF:
        sysm = system(O, name, radius, method, fixed_pose)
        M = sysm.precond(L)
        b = random_rhs(sysm) if rhs == "random" else sysm.b
        _REF[key] = (sysm, M, b, pcg(sysm.A, M, b, max_it, rtol, keep))
    return _REF[key]


_SPREAD = {}
ALPHA_SPREAD = {}    # same key: the largest |d alpha_1| / alpha_1 of those reruns
B_SPREAD = {}        # (name, radius, method, fixed_pose): the largest |db| per entry of the scaled gradient over those reruns


def spread(O, name, L, radius, rhs="random", method=0, fixed_pose=0, keep=8):
    """spread_k, k = 1..keep: per group of rows() the largest |dy_k| over three reruns of the restatement with every Jacobian
    entry moved by +-DJ.  Returns a list (over k) of lists (over rows())."""
    key = (name, L, radius, rhs, method, fixed_pose, keep)
    if key not in _SPREAD:
        sysm, M, b, ref = reference(O, name, L, radius, 0.0, keep, rhs, method, fixed_pose, keep)
        groups = sysm.rows()
        out = [[0.0] * len(groups) for _ in ref.ys]
        da, db = 0.0, np.zeros(sysm.n3)
        for seed in (1, 2, 3):
            pk = (name, radius, method, fixed_pose, seed)
            if pk not in _SYS:
                _SYS[pk] = sysm.perturbed(seed)
            ps = _SYS[pk]
            pr = pcg(ps.A, ps.precond(L), random_rhs(ps) if rhs == "random" else ps.b, len(ref.ys), 0.0, keep)
            da = max(da, abs(pr.alpha1 - ref.alpha1) / abs(ref.alpha1))
            db = np.maximum(db, np.abs(ps.b - sysm.b))
            for k, (y0, y1) in enumerate(zip(ref.ys, pr.ys)):
                for j, m in enumerate(groups):
                    out[k][j] = max(out[k][j], float(np.abs(y1 - y0)[m].max()))
        _SPREAD[key] = out
        ALPHA_SPREAD[key] = da
        B_SPREAD[(name, radius, method, fixed_pose)] = db
    return _SPREAD[key]


def iterate_bound(sysm, y_k, spread_k):
    """|y_dev - y_k| per group of rows(): 10 spread_k + eps 3n kappa |y_k|_inf, the norm over the group's rows"""
    kap = kappa(sysm)
    return [10.0 * sp_ + EPS * sysm.n3 * kap * float(np.abs(y_k[m]).max()) for m, sp_ in zip(sysm.rows(), spread_k)]
