"""CPU: the numpy restatement of the direct solve (_direct_restatement.restate) alone, on every case of test_gpu_direct.py's
table with N <= 5000, at the initial poses and radii 1e4 and 1e12 -- the conditions the GPU test relies on: the Cholesky
factorisation of I + V Z does not fail and one refinement step reaches eta_restate <= 10 x floor for every right-hand side
(floor: _direct_restatement.rounding_floor).  A case the reference cannot solve does not belong in the table."""
import time

import numpy as np
import pytest

from _direct_restatement import backward_error, restate, rounding_floor, system_matrix
from test_gpu_direct import CASES, build_case, layout, right_hand_sides

SMALL = [k for k, c in CASES.items() if c["dataset"] or c["n"] <= 5000]


def test_case_table_covers_both_sides_of_every_switch():
    """every structural switch of direct_setup() / the kernels has a case on either side"""
    sizes = {c["n"] for c in CASES.values() if not c["dataset"]}
    assert {2, 3, 31, 32, 33, 255, 256, 257, 512, 516, 2048, 2049, 4096, 4097, 4799, 4800, 17999, 18000, 19201, 65536} <= sizes
    for n in (40, 300):
        assert {0, 1, 10, 11, 21, 22, 32, 43} <= {len(c["loops"]) for c in CASES.values() if c["n"] == n}
    assert 2047 in {len(c["loops"]) for c in CASES.values() if c["n"] == 300}
    assert [len(layout(n)[0]) for n in (255, 256, 4799, 4800, 17999, 18000, 19201)] == [0, 3, 3, 4, 14, 15, 15]
    assert [layout(n)[3] for n in (4096, 4097)] == [1, 2]


@pytest.mark.parametrize("case", SMALL)
def test_restatement_solves_every_case(oracle, case):
    c = CASES[case]
    t0 = time.perf_counter()
    ag, og = build_case(case, oracle)
    n, fixed = ag.n_poses, c["fixed"]
    first = (int(ag.ia[n - 1]), int(ag.ib[n - 1])) if ag.n_edges > n - 1 and not c["dataset"] else ()
    for radius in (1e4, 1e12):
        sysm = oracle.lm_system(og, ag.poses, ag.poses, radius, method=min(c["opts"].get("method", 1), 1), fixed_pose=fixed)
        A = system_matrix(sysm)
        floor = rounding_floor(A)
        B, names = right_hand_sides(sysm, n, fixed, first, c["rhs"] == "few", np.random.default_rng(7))
        Y = restate(sysm, og, fixed, B, (0, 1))
        eta = {k: max(backward_error(A, Y[k][:, j], B[:, j]) for j in range(B.shape[1])) for k in (0, 1)}
        print("%s radius %.0e: %d right-hand sides, eta_restate raw %.1e, one step %.1e, floor %.1e" % (
            case, radius, len(names), eta[0], eta[1], floor))
        assert np.isfinite(Y[1]).all()
        if fixed >= 0:
            assert not Y[1][3 * fixed:3 * fixed + 3].any()
        assert eta[1] <= 10.0 * floor, (case, radius, eta, floor)
    print("%s: %.1f s" % (case, time.perf_counter() - t0))
