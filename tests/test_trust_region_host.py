"""CPU: the trust-region step policy (csrc/trust_region.h, what pgo_handle::lm_iteration, pgo_batch::iterate and
k_window_solve decide with) through tests/native/trust_region_main.cpp under ASan + UBSan: the recorded radii of every
golden LM trajectory replayed step by step, and by hand the cases the fixtures do not hold."""
import glob
import json
import os

import pytest

import _native_san as NS
from conftest import GOLDEN

TOLERANCE_TERMINATIONS = (1, 3)   # PGO_TERM_CONVERGENCE_FTOL, _PTOL: the last record is the candidate that ended the solve


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("trust_region"), "trust_region_main")


def test_golden_radii_replayed(exe, tmp_path):
    """every record after the first: the previous record's radius and the recorded relative_decrease / step_ok through
    tr_accept / tr_reject give the recorded radius to 1e-15 relative (rho went through JSON; measured maximum 3.9e-16)"""
    src, dst = str(tmp_path / "replay_in.txt"), str(tmp_path / "replay_out.txt")
    expect, n_acc, n_rej = [], 0, 0
    files = sorted(glob.glob(os.path.join(GOLDEN, "lm_*.json")))
    assert len(files) == 22
    with open(src, "w") as f:
        for path in files:
            fx = json.load(open(path))
            recs = fx["records"]
            f.write("seq %d\n" % (len(recs) - 1))
            for i in range(1, len(recs)):
                code = recs[i]["step_ok"]
                if i == len(recs) - 1 and code == 0 and fx["termination"] in TOLERANCE_TERMINATIONS:
                    code = 2
                n_acc += code == 1
                n_rej += code == 0
                assert code != -1   # (the fixtures hold no invalid step: test_policy_by_hand)
                f.write("%d %.17g %.17g\n" % (code, recs[i]["relative_decrease"], recs[i - 1]["radius"]))
                expect.append(recs[i]["radius"])
    out = NS.run([exe, "replay", src, dst])
    assert "replay ok: %d steps" % len(expect) in out
    got = [float(x) for x in open(dst).read().split()]
    assert len(got) == len(expect)
    assert (n_acc, n_rej) == (878, 136)
    worst = max(abs(g - e) / e for g, e in zip(got, expect))
    print("largest relative difference from the recorded radius: %.3g over %d steps" % (worst, len(expect)))
    assert worst <= 1e-15


def test_policy_by_hand(exe):
    v = dict(line.split() for line in NS.run([exe, "drive"]).splitlines())
    f = lambda k: float(v[k])
    # five invalid steps in a row: 1/2, 1/8, 1/64, 1/1024 of the start, failure on the fifth (which changes nothing)
    for k, radius in ((1, 512.0), (2, 128.0), (3, 16.0), (4, 1.0), (5, 1.0)):
        assert v["invalid%d_usable" % k] == "0"
        assert v["invalid%d_failed" % k] == ("1" if k == 5 else "0")
        assert f("invalid%d_radius" % k) == radius
        assert v["invalid%d_prev_success" % k] == "0"
    assert v["run_reset_failures"] == "0"
    # reject, reject: / 2, / 4; accept resets the factor; the next reject divides by 2 again
    assert f("reject2_radius") == 12.5 and f("reject2_factor") == 8.0
    assert f("accept_half_radius") == 12.5 and f("accept_factor") == 2.0 and v["accept_prev_success"] == "1"
    assert f("reject_after_accept_radius") == 6.25 and f("reject_after_accept_factor") == 4.0 and v["reject_prev_success"] == "0"
    assert f("accept_one_radius") == 10.0 / (1.0 / 3.0)
    assert f("accept_capped_radius") == 50.0
    assert f("accept_quarter_radius") == 10.0 / 1.125
    # PGO_TERM_*: FTOL 1, GTOL 2, PTOL 3, NO_CONVERGENCE 4, MIN_RADIUS 5
    assert (v["tol_both"], v["tol_ptol"], v["tol_ftol"], v["tol_none"]) == ("3", "3", "1", "0")
    assert v["stop_none"] == "0" and v["stop_iters"] == "4" and v["stop_gtol"] == "2"
    assert v["stop_gtol_before_radius"] == "2" and v["stop_min_radius"] == "5" and v["stop_gtol_after_reject"] == "0"
    assert f("rho_plain") == 0.75 and v["rho_dbl_max_is_minus_dbl_max"] == "1"
