"""The pair operations of csrc/coarsen.h as a program of their own, tests/native/coarsen_info_main.cpp, built by g++ under
ASan + UBSan: the run is clean and its output is bitwise what the library's host entry point pgo_coarsen_info_plan returns (the
same statement, the same serial order)."""
import os

import numpy as np
import pytest

import _coarsen_cases as CC
import _coarsen_info_cases as CI
import _native_san as NS


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("coarsen_info_native"), "coarsen_info_main")


@pytest.mark.parametrize("S", [2, 7, 64, 65, 256])
def test_sanitized_program_is_bitwise_the_library(pgo, exe, tmp_path, S):
    n = 403
    P, ia, ib, meas, kind = CC.exact_graph(n, 60, seed=S)
    meas = meas + np.random.default_rng(S).normal(0, 0.05, meas.shape)
    info = CI.random_spd_info(len(ia), S)
    want = pgo.coarsen_info_plan(n, ia, ib, meas, kind, S, info)
    K = want["n_poses"]
    keep = want["origin"][K - 1:]
    src, dst = os.path.join(str(tmp_path), "in.txt"), os.path.join(str(tmp_path), "out.txt")
    num = lambda v: " ".join("%.17g" % x for x in v)
    with open(src, "w") as f:
        f.write("%d %d %d\n" % (n, S, len(keep)))
        for i in range(n - 1):
            f.write("%d %s %s\n" % (ia[i] > ib[i], num(meas[i]), num(info[i])))
        for e in keep:
            f.write("%d %d %s %s\n" % (ia[e], ib[e], num(meas[e]), num(info[e])))
    out = NS.run([exe, src, dst])
    assert "coarsen info ok: %d poses, %d key poses, %d edges" % (n, K, len(keep)) in out
    v = np.loadtxt(dst, ndmin=2)
    assert v.shape == (n + K - 1 + 2 * len(keep), 6)
    assert v[:n].tobytes() == want["Ccov"].tobytes() and v[n:n + K - 1].tobytes() == want["Cendcov"].tobytes()
    T = v[n + K - 1:].reshape(-1, 12)
    assert T[:, :6].tobytes() == want["cov"][K - 1:].tobytes() and T[:, 6:].tobytes() == want["info"][K - 1:].tobytes()
