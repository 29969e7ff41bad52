"""pgo_pose_covariance without a GPU: the C-ABI surface (symbols, option defaults, struct layouts) and the restatement the
GPU path is built on -- Sigma = (J'J)^-1 with the constant pose removed equals S A^-1 S, A the Jacobi-scaled undamped system
of the LM loop (oracle.lm_system at radius = infinity, whose d2 is 1 on the constant pose and 0 elsewhere)."""
import ctypes
import os
import re

import numpy as np

from conftest import DATA, ROOT, oracle_graph


def test_symbols_declared_and_exported(pgo):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgo.h")).read(), flags=re.S)
    for sym in ("pgo_covariance_options_default", "pgo_pose_covariance"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in pgo.EXPORTS
        assert getattr(pgo.lib(), sym) is not None
    assert re.search(r'^ \*   "cov_poses_per_pass"', open(os.path.join(ROOT, "include", "pgo.h")).read(), flags=re.M)
    pgo.set_knob("cov_poses_per_pass", -1)


def test_option_defaults_and_layouts(pgo):
    o = pgo.CovarianceOptions()
    assert (o.rtol, o.max_iters, o.poses_per_pass, o.cross) == (1e-10, 20000, 8, 0)
    assert ctypes.sizeof(pgo.CovarianceOptions) == 24 and ctypes.sizeof(pgo.CovarianceReport) == 32
    assert pgo.CovarianceOptions(cross=1, poses_per_pass=16).poses_per_pass == 16


def test_null_handle_is_an_invalid_argument(pgo):
    out = np.zeros(9)
    idx = np.zeros(1, np.int32)
    st = pgo.lib().pgo_pose_covariance(None, 1, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None,
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None)
    assert st == -1


def test_scaled_undamped_system_restates_the_covariance(pgo, oracle):
    """(J'J)^-1 on the free poses == S (S J'J S + I_fixed)^-1 S, INTEL + 50 outliers with DCS at the golden solution"""
    import scipy.sparse as sp
    g = pgo.ReadG2O(os.path.join(DATA, "INTEL.g2o"))
    g.add_random_C(50, 1)
    og = oracle_graph(oracle, g)
    poses = np.load(os.path.join(ROOT, "tests", "golden", "lm_INTEL_out50_m1_poses.npy"))
    L = oracle.lm_system(og, poses, np.array(g.poses), np.inf, method=1)
    assert np.array_equal(L.d2[3:], np.zeros(3 * g.n_poses - 3)) and np.array_equal(L.d2[:3], np.ones(3))
    A = (L.H + sp.diags(L.d2)).toarray()
    Sig_scaled = L.s[:, None] * np.linalg.inv(A) * L.s[None, :]
    _, _, J = oracle.evaluate(og, poses, method=1)
    E, N = g.n_edges, g.n_poses
    ia, ib = np.asarray(og.ia), np.asarray(og.ib)
    Jd = np.zeros((3 * E, 3 * N))
    for e in range(E):
        Je = J[e].reshape(3, 6)   # (the oracle's layout: per residual row, d/dP1 then d/dP2)
        Jd[3 * e:3 * e + 3, 3 * ia[e]:3 * ia[e] + 3] = Je[:, :3]
        Jd[3 * e:3 * e + 3, 3 * ib[e]:3 * ib[e] + 3] = Je[:, 3:]
    H = Jd.T @ Jd
    Sig = np.zeros_like(H)
    Sig[3:, 3:] = np.linalg.inv(H[3:, 3:])
    scale = np.abs(Sig).max()
    assert np.abs(Sig_scaled - Sig).max() <= 1e-6 * scale
    for i in (1, 400, N - 1):
        b, r = Sig_scaled[3 * i:3 * i + 3, 3 * i:3 * i + 3], Sig[3 * i:3 * i + 3, 3 * i:3 * i + 3]
        assert np.linalg.norm(b - r) <= 1e-7 * np.linalg.norm(r)
