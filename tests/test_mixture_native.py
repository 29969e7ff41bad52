"""csrc/mixture.h as a program of its own, tests/native/mixture_main.cpp, built by g++ under ASan + UBSan: the run is clean, and
its selections, q and constants are those of the numpy restatement (tests/_mixture_cases.py) and of the library's host entry
point pgo_mixture_eval, over K = 1..8 under every loss, exact ties, non-finite s and constants across twelve decades."""
import os

import numpy as np
import pytest

import _loss_restatement as LR
import _mixture_cases as MC
import _native_san as NS


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("mixture_native"), "mixture_main")


def test_sanitized_program_against_numpy_and_the_library(pgo, exe, tmp_path):
    cases = MC.eval_cases()
    src, dst = os.path.join(str(tmp_path), "in.txt"), os.path.join(str(tmp_path), "out.txt")
    with open(src, "w") as f:
        f.write("%d\n" % len(cases))
        for comps, s, loss in cases:
            f.write("%d %d %.17g\n" % (len(comps), LR.TYPES[loss[0]], loss[1]))
            for c, sk in zip(comps, s):
                f.write("%.17g %.17g %.17g\n" % (c[3], c[4], sk))
    assert "mixture ok: %d cases" % len(cases) in NS.run([exe, src, dst])
    lines = [ln.split() for ln in open(dst).read().split("\n") if ln]
    assert len(lines) == len(cases)
    seen_k, n_none, n_single = set(), 0, 0
    for (comps, s, loss), ln in zip(cases, lines):
        K = len(comps)
        k, qb, mg = int(ln[0]), float(ln[1]), float(ln[2])
        c = np.array([float(v) for v in ln[3:]])
        assert c.shape == (K,)
        # the constants: two logarithms and two roundings
        ref_c = MC.const(comps[:, 3], comps[:, 4])
        assert np.all(np.abs(c - ref_c) <= 4e-16 * (np.abs(np.log(comps[:, 3])) + 1.5 * np.abs(np.log(comps[:, 4])) + 1.0))
        q = MC.q_of(comps, s, loss)
        rk, rq, rm = MC.pick(q)
        what = (K, loss, s.tolist())
        # q_k = w 1/2 rho + c: rho to a few ulp of libm, one product, one sum
        tol = 1e-14 * (np.nanmax(np.abs(q)) if rk >= 0 else 1.0)
        if rk >= 0 and not (rm <= 2.0 * tol):
            assert k == rk, what
        if rk < 0:
            assert k == -1 and np.isnan(qb) and np.isnan(mg), what
            n_none += 1
        else:
            assert abs(qb - rq) <= tol, what
            assert (mg == np.inf and rm == np.inf) or abs(mg - rm) <= 2.0 * tol, what
            n_single += int(mg == np.inf)
            seen_k.add(k)
        # the library's host entry point runs the same statement: bitwise
        lk, lq, lm = pgo.mixture_eval(comps, s, pgo.Loss(*loss))
        assert lk == k and np.array([lq, lm]).tobytes() == np.array([qb, mg]).tobytes(), what
    assert seen_k == set(range(MC.MAX_K)) and n_none >= 12 and n_single >= 6


def test_ties_go_to_the_lower_index(pgo):
    for comps, s, loss in MC.eval_cases():
        if len(comps) >= 2 and np.all(np.isfinite(s)) and (comps[:, 3] == 1e6).sum() == 2:
            i, j = np.nonzero(comps[:, 3] == 1e6)[0]
            assert np.array_equal(comps[i], comps[j]) and s[i] == s[j]
            k, qb, mg = pgo.mixture_eval(comps, s, pgo.Loss(*loss))
            assert k == i and mg == 0.0, (loss, i, j, k)
