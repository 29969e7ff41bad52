"""csrc/chordal.h as a program of its own, tests/native/chordal_main.cpp, built by g++ under ASan + UBSan: the run is clean and
its output is bitwise what the library's host entry point, pgo_chordal_plan, returns (the same statement, the same serial
order) -- slot table, assembly, Jacobi-PCG, headings, report and reject rounds.  Nothing is loaded into Python."""
import os

import numpy as np
import pytest

import _chordal_cases as CC
import _native_san as NS


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("chordal_native"), "chordal_main")


def run_program(exe, tmp, c, rtol=1e-8, max_iters=20000, mag_min=1e-3, rounds=0, reject_xy=2.0, reject_th=0.35):
    n, E = c["n"], len(c["ia"])
    const = np.arange(n) == 0 if c["constant"] is None else np.asarray(c["constant"], bool)
    src, dst = os.path.join(str(tmp), "in.txt"), os.path.join(str(tmp), "out.txt")
    with open(src, "w") as f:
        f.write("%d %d %.17g %d %.17g %d %.17g %.17g\n" % (n, E, rtol, max_iters, mag_min, rounds, reject_xy, reject_th))
        for p, k in zip(c["poses"], const):
            f.write("%.17g %.17g %.17g %d\n" % (p[0], p[1], p[2], k))
        for a, b, m, w in zip(c["ia"], c["ib"], c["meas"], c["w"]):
            f.write("%d %d %.17g %.17g %.17g %.17g\n" % (a, b, m[0], m[1], m[2], w))
    out = NS.run([exe, src, dst])
    assert "chordal ok: %d poses, %d edges" % (n, E) in out
    with open(dst) as f:
        lines = f.read().split("\n")
    P = np.array([[float(v) for v in ln.split()] for ln in lines[:n]])
    R = np.array([[float(v) for v in ln.split()] for ln in lines[n:n + E]])
    head = lines[n + E].split()
    solves = [ln.split() for ln in lines[n + E + 1:n + E + 1 + int(head[0])]]
    return P, R[:, :2], R[:, 2], head, solves


CASES = {"planted-65-two": (lambda: CC.planted_case(65, "two"), {}), "planted-257-weights": (lambda: CC.planted_case(257, "weights"), {}),
         "planted-513-const": (lambda: CC.planted_case(513, "const"), dict(rtol=1e-10)), "fixture-257": (lambda: CC.fixture_case(257), {}),
         "degenerate-65": (lambda: CC.degenerate_case(65), {}), "reject-257": (lambda: CC.reject_case(257), dict(rounds=3))}


@pytest.mark.parametrize("name", sorted(CASES))
def test_sanitized_program_is_bitwise_the_library(pgo, exe, tmp_path, name):
    make, opt = CASES[name]
    c = make()
    want, wres, w_out, summ = pgo.chordal_plan(*CC.plan_args(c), w=c["w"], constant=c["constant"], **opt)
    P, res, wo, head, solves = run_program(exe, tmp_path, c, **opt)
    assert P.tobytes() == want.tobytes()
    assert res.tobytes() == wres.tobytes() and wo.tobytes() == w_out.tobytes()
    assert [int(v) for v in head[:3]] == [summ["n_solves"], summ["n_rejected"], summ["n_degenerate"]] and float(head[3]) == summ["min_mag"]
    for got, s in zip(solves, summ["solves"]):
        assert [int(v) for v in got[:4]] == s["iters"] + s["converged"] and [float(v) for v in got[4:]] == s["rel_residual"]
    assert summ["solves"][0]["iters"][0] > 0
    if name.startswith("reject"):
        assert summ["n_rejected"] == len(c["bad"]) > 0
    if name.startswith("degenerate"):
        assert summ["n_degenerate"] > 0
