"""csrc/loop_support.h as a program of its own, tests/native/loop_support_main.cpp, built by g++ under ASan + UBSan: the run is
clean and its output is bitwise what the library's host entry point, pgo_loop_support_plan, returns (the same statement, the
same serial order)."""
import os

import numpy as np
import pytest

import _native_san as NS
import _support_cases as SC


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("loop_support_native"), "loop_support_main")


def run_program(exe, tmp, n, ia, ib, meas, sel, window, tol_xy, tol_th, min_support):
    src, dst = os.path.join(str(tmp), "in.txt"), os.path.join(str(tmp), "out.txt")
    with open(src, "w") as f:
        f.write("%d %d %d %.17g %.17g %d\n" % (n, len(ia), window, tol_xy, tol_th, min_support))
        for a, b, m, s in zip(ia, ib, meas, sel):
            f.write("%d %d %s %d\n" % (a, b, " ".join("%.17g" % v for v in m), s))
    out = NS.run([exe, src, dst])
    assert "loop support ok: %d poses, %d edges" % (n, len(ia)) in out
    with open(dst) as f:
        lines = f.read().split("\n")
    T = np.array([[float(v) for v in ln.split()] for ln in lines[:n]])
    rec = [ln.split() for ln in lines[n:n + len(ia)]]
    ints = np.array([[int(v) for v in r[:4]] for r in rec], np.int32)
    q = np.array([float(r[4]) for r in rec])
    return T, ints, q, [int(v) for v in lines[n + len(ia)].split()]


@pytest.mark.parametrize("n,opt", [(65, {}), (257, dict(window=1)), (513, dict(window=256, min_support=2)), (1000, dict(tol_xy=0.05, tol_th=0.02)),
                                   (500, {})], ids=["65", "257-w1", "513-w256", "1000-tight", "fixture-500"])
def test_sanitized_program_is_bitwise_the_library(pgo, exe, tmp_path, n, opt):
    if n == 500:
        N, ia, ib, meas, kind = SC.fixture(500)
        select = None
    else:
        c = SC.planted(n)
        N, ia, ib, meas, kind, select = c["n"], c["ia"], c["ib"], c["meas"], c["kind"], c["select"]
    kw = dict(SC.DEFAULTS, **opt)
    want, stats, wT = pgo.loop_support_plan(N, ia, ib, meas, kind, select=select, want_T=True, **kw)
    sel = (kind != 0) if select is None else select
    T, ints, q, tot = run_program(exe, tmp_path, N, ia, ib, meas, sel, kw["window"], kw["tol_xy"], kw["tol_th"], kw["min_support"])
    assert T.tobytes() == wT.tobytes()
    for k, name in enumerate(("selected", "n_pairs", "n_consistent", "best")):
        assert np.array_equal(ints[:, k], want[name]), name
    assert q.tobytes() == np.ascontiguousarray(want["q_min"]).tobytes()
    assert tot == [stats["n_selected"], stats["n_supported"], stats["n_pairs_total"], stats["max_pairs"]]
    assert stats["n_selected"] > 0 and stats["n_pairs_total"] > 0
