"""numpy restatement of graduated non-convexity with the truncated-least-squares surrogate (GNC-TLS; Yang, Antonante,
Tzoumas, Carlone, RA-L 2020) as pgo_gnc_solve runs it: the reference of tests/test_gnc_host.py and tests/test_gpu_gnc.py.
A helper, not a test.

The inner solves are tests/_loss_restatement.lm (Ceres' LM loop with a sparse LU) on an oracle wrapper that scales every
block's r and J by sqrt(w); with a Trivial loss that is the cost sum w 1/2 |e|^2.  The weights follow the plain |e|^2 of
the oracle's METHOD 0 blocks at the poses a round ends with."""
import os

import numpy as np

import _loss_restatement as LR

TRIVIAL = [("trivial", 0.0)]


def mu0(c2, rmax2):
    return c2 / (2.0 * rmax2 - c2)


def tls_weight(c2, mu, s):
    """gnc_tls_weight of csrc/gnc.h, vectorised, in its order of operations; a non-finite s gives 0"""
    s = np.asarray(s, np.float64)
    lo, hi = mu / (mu + 1.0) * c2, (mu + 1.0) / mu * c2
    with np.errstate(all="ignore"):
        mid = np.minimum(1.0, np.maximum(0.0, np.sqrt(c2 * mu * (mu + 1.0) / s) - mu))
    w =np.where(s <= lo, 1.0, np.where(s >= hi, 0.0, mid))
    return np.where(np.isfinite(s), w, 0.0)


class WeightedOracle:
    """oracle.evaluate with every block's r and J scaled by sqrt(w)"""

    def __init__(self, O, w):
        self.O, self.w = O, np.asarray(w, np.float64)

    def evaluate(self, og, *args):
        c, r, J = self.O.evaluate(og, *args)
        q = np.sqrt(self.w)[:, None]
        return c, q * r, q * J


def plain_s(O, og, poses):
    _, r, _ = O.evaluate(og, poses, 0, 0.5, 0.0, False, True, True, 1, False)
    return (r * r).sum(axis=1)


def subgraph(O, n):
    """the sub-graph "poses < n" of tests/golden/synth_manhattan_2000_s7.npz as an oracle graph, edges in file order"""
    here = os.path.dirname(os.path.abspath(__file__))
    z = np.load(os.path.join(here, "golden", "synth_manhattan_2000_s7.npz"))
    keep = (z["ia"] < n) & (z["ib"] < n)
    poses = np.array(z["poses"][:n], np.float64)
    E = int(keep.sum())
    info = np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]), (E, 1))
    return O.Graph(np.arange(n, dtype=np.int32), poses, np.array(z["ia"][keep], np.int32), np.array(z["ib"][keep], np.int32),
                   np.array(z["meas"][keep], np.float64), info, np.array(z["kind"][keep], np.uint8))


class GncResult:
    pass


def gnc(O, og, cbar, mu_factor=1.4, inner_iters=5, final_iters=50, max_rounds=100, select=None, poses=None):
    """the loop of pgo_gnc_solve, METHOD 0, Trivial loss.  select: a mask over the edges (default kind != 0)"""
    kind = np.asarray(og.kind)
    sel = (kind != 0) if select is None else (np.asarray(select).reshape(-1) != 0)
    E = og.n_edges
    cls = np.zeros(E, np.int64)
    c2 = cbar * cbar
    x = np.array(og.poses if poses is None else poses, np.float64).reshape(-1, 3)
    w = np.ones(E)
    res = GncResult()
    res.rounds, res.hit_max_rounds = [], False

    def solve(x0, iters):
        saved = np.array(og.poses)
        og.poses[:] = x0
        try:
            return LR.lm(WeightedOracle(O, w), og, TRIVIAL, cls, method=0, max_iters=iters)
        finally:
            og.poses[:] = saved

    s = plain_s(O, og, x)
    rmax2 = float(s[sel].max()) if sel.any() else 0.0
    res.rmax2 = rmax2
    if not (2.0 * rmax2 > c2):
        fin = solve(x, final_iters)
        res.poses, res.weights, res.final = fin.poses, w, fin
        return res
    mu = mu0(c2, rmax2)
    for k in range(max_rounds):
        r = solve(x, inner_iters)
        if r.termination == 6:
            res.poses, res.weights, res.final = x, w, r
            return res
        x = r.poses
        s = plain_s(O, og, x)
        w = np.where(sel, tls_weight(c2, mu, s), w)
        nonbin = int(((w > 0.0) & (w < 1.0) & sel).sum())
        res.rounds.append(dict(mu=mu, weighted_cost=float((w[sel] * s[sel]).sum()), n_nonbinary=nonbin,
                               n_zero=int(((w == 0.0) & sel).sum()), lm_iterations=r.iterations, lm_termination=r.termination))
        if nonbin == 0 and k > 0:
            break
        mu *= mu_factor
    else:
        res.hit_max_rounds = True
    fin = solve(x, final_iters)
    res.poses, res.weights, res.final = fin.poses, w, fin
    res.s_plain = plain_s(O, og, fin.poses)
    return res
