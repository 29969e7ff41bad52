"""Shared by test_score_host.py and test_gpu_score.py: the per-edge weights of include/pgo.h ("scoring", pgo_edge_weight) restated
in numpy, and the thresholds of the classification check on INTEL + 50 seeded outliers."""
import os

import numpy as np

from conftest import DATA, GOLDEN

PHI = 0.5
# weight < TAU[method] is the "turned down" class of the classification check; test_score_host.py checks that no weight at
# the oracle's final poses (tests/golden/lm_INTEL_out50_m<method>_poses.npy) lies within 1e-3 of it
TAU = {0: 0.5, 1: 0.02}
TAU_GAP = 1e-3


def intel50(pgo):
    g = pgo.ReadG2O(os.path.join(DATA, "INTEL.g2o"))
    g.add_random_C(50, 1)
    return g


def oracle_final_poses(method):
    return np.load(os.path.join(GOLDEN, "lm_INTEL_out50_m%d_poses.npy" % method))


def rho(loss, s):
    """(rho, rho') of a (name, a) loss at s: the table of include/pgo.h, "robust losses\""""
    name, a = loss
    s = np.asarray(s, np.float64)
    if name == "trivial":
        return s.copy(), np.ones_like(s)
    if name == "huber":
        out = s > a * a
        r = np.sqrt(np.where(out, s, 1.0))
        return np.where(out, 2 * a * r - a * a, s), np.where(out, np.maximum(a / r, 2.2250738585072014e-308), 1.0)
    if name == "cauchy":
        b = a * a
        return b * np.log1p(s / b), 1.0 / (1.0 + s / b)
    raise ValueError(name)


def restate_weights(g, poses, method, losses=(("huber", 0.01),), edge_class=None):
    """dict of arrays s_plain, scale, rho1, weight, cost over the edges of g at `poses`; losses: the (name, a) of each class,
    an edge's class min(kind, n_classes - 1) unless edge_class says otherwise"""
    poses = np.asarray(poses, np.float64)
    ia, ib, meas, kind = np.array(g.ia), np.array(g.ib), np.array(g.meas), np.array(g.kind)
    P1, P2 = poses[ia], poses[ib]
    d = P2[:, :2] - P1[:, :2]
    c, s = np.cos(P1[:, 2]), np.sin(P1[:, 2])
    ux, uy = c * d[:, 0] + s * d[:, 1] - meas[:, 0], -s * d[:, 0] + c * d[:, 1] - meas[:, 1]
    cd, sd = np.cos(meas[:, 2]), np.sin(meas[:, 2])
    ex, ey = cd * ux + sd * uy, -sd * ux + cd * uy
    et = np.arcsin(np.sin(P2[:, 2] - P1[:, 2] - meas[:, 2]))
    s_plain = ex ** 2 + ey ** 2 + et ** 2
    scale = np.ones(len(ia))
    if method == 1:
        psi = np.sqrt(2 * PHI / (PHI + ex ** 2 + ey ** 2))
        scale = np.where((kind != 0) & (psi < 1.0), psi, 1.0)
    sv = scale ** 2 * s_plain
    cls = np.minimum(kind, len(losses) - 1) if edge_class is None else np.asarray(edge_class)
    r0, r1 = np.zeros(len(ia)), np.zeros(len(ia))
    for k, loss in enumerate(losses):
        sel = cls == k
        r0[sel], r1[sel] = rho(loss, sv[sel])
    return {"s_plain": s_plain, "scale": scale, "rho1": r1, "weight": scale ** 2 * r1, "cost": 0.5 * r0}
