"""csrc/coarsen.h as a program of its own, tests/native/coarsen_main.cpp, built by g++ under ASan + UBSan: the run is clean and
its output is bitwise what the library's host entry points, pgo_coarsen_plan and pgo_prolong_eval, return (the same statement,
the same serial order)."""
import os

import numpy as np
import pytest

import _coarsen_cases as CC
import _native_san as NS


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("coarsen_native"), "coarsen_main")


def run_program(exe, tmp, n, S, rev, chain_meas, ea, eb, em, X):
    src, dst = os.path.join(str(tmp), "in.txt"), os.path.join(str(tmp), "out.txt")
    with open(src, "w") as f:
        f.write("%d %d %d\n" % (n, S, len(ea)))
        for r, m in zip(rev, chain_meas):
            f.write("%d %s\n" % (r, " ".join("%.17g" % v for v in m)))
        for a, b, m in zip(ea, eb, em):
            f.write("%d %d %s\n" % (a, b, " ".join("%.17g" % v for v in m)))
        for x in X:
            f.write(" ".join("%.17g" % v for v in x) + "\n")
    K = -(-n // S)
    out = NS.run([exe, src, dst])
    assert "coarsen ok: %d poses, %d key poses, %d edges" % (n, K, len(ea)) in out
    v = np.loadtxt(dst, ndmin=2)
    assert v.shape == (2 * n + K - 1 + len(ea), 3)
    return v[:n], v[n:n + K - 1], v[n + K - 1:n + K - 1 + len(ea)], v[n + K - 1 + len(ea):]


@pytest.mark.parametrize("S", [2, 7, 64, 65, 256])
def test_sanitized_program_is_bitwise_the_library(pgo, exe, tmp_path, S):
    n = 403
    P, ia, ib, meas, kind = CC.exact_graph(n, 60, seed=S)
    meas = meas + np.random.default_rng(S).normal(0, 0.05, meas.shape)
    X = np.random.default_rng(S + 1).normal(0, 5, (-(-n // S), 3))
    want = pgo.coarsen_plan(n, ia, ib, meas, kind, S)
    keep = want["origin"][want["n_poses"] - 1:]
    C_, Cend, T, Pr = run_program(exe, tmp_path, n, S, ia[:n - 1] > ib[:n - 1], meas[:n - 1], ia[keep], ib[keep], meas[keep], X)
    assert C_.tobytes() == want["C"].tobytes() and Cend.tobytes() == want["Cend"].tobytes()
    assert T.tobytes() == want["meas"][want["n_poses"] - 1:].tobytes()
    assert Pr.tobytes() == pgo.prolong_eval(n, S, want["C"], want["Cend"], X).tobytes()
