"""pgo_chordal_plan (include/pgo.h, "chordal initialisation"; csrc/chordal.h) on the host against the numpy / scipy restatement
of tests/_chordal_cases.py, which solves both Hermitian systems directly: agreement within what rtol and the systems' smallest
eigenvalues imply (the bound is derived in _chordal_cases.bounds and printed beside the measured difference), exactness on a
noise-free graph, the errors, the degenerate poses and the reject rounds.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import _chordal_cases as CC
from _coarsen_cases import wrap

INVALID_ARG, NUMERIC, UNSUPPORTED = -1, -7, -8
RTOL = 1e-8   # the default

CASES = {"fixture-2000": lambda: CC.fixture_case(), "fixture-65": lambda: CC.fixture_case(65), "fixture-257": lambda: CC.fixture_case(257)}
for _n in CC.SC.PLANTED_N:
    for _v in ("plain", "const", "two", "weights"):
        CASES["planted-%d-%s" % (_n, _v)] = (lambda n=_n, v=_v: CC.planted_case(n, v))


def run(pgo, c, **kw):
    return pgo.chordal_plan(*CC.plan_args(c), w=c["w"], constant=c["constant"], **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_equals_the_restatement(pgo, name):
    c = CASES[name]()
    want, wres, ww, info = CC.restate(*CC.plan_args(c), w=c["w"], constant=c["constant"])
    got, res, w_out, summ = run(pgo, c)
    s = summ["solves"][0]
    assert summ["n_solves"] == 1 and s["converged"] == [1, 1] and max(s["rel_residual"]) <= RTOL and min(s["iters"]) > 0
    CC.compare(got, want, info, RTOL, name)
    C_ = np.zeros(c["n"], bool) if c["constant"] is not None else np.arange(c["n"]) == 0
    if c["constant"] is not None:
        C_ = np.asarray(c["constant"], bool)
    assert got[C_].tobytes() == np.ascontiguousarray(c["poses"][C_]).tobytes()           # constant poses keep their values
    assert summ["n_degenerate"] == info["n_degenerate"] == 0 and summ["n_rejected"] == 0
    assert abs(summ["min_mag"] - info["min_mag"]) <= CC.bounds(info, RTOL)[0]           # (|z| moves by at most dz < the heading bound)
    assert np.array_equal(w_out, c["w"])
    # the report is the definition evaluated at the plan's own poses
    t, th = got[:, 0] + 1j * got[:, 1], got[:, 2]
    ia, ib, m = c["ia"], c["ib"], c["meas"]
    r_th = np.abs(wrap(th[ib] - th[ia] - m[:, 2]))
    assert np.abs(res[:, 1] - r_th).max() <= 1e-12
    b_th, b_xy = CC.bounds(info, RTOL)
    assert np.abs(res[:, 0] - wres[:, 0]).max() <= 2 * b_xy + np.hypot(m[:, 0], m[:, 1]).max() * 2 * b_th
    if name.startswith("planted") and name.endswith("plain"):   # a hub row with more than 64 slots is among them
        assert np.bincount(np.r_[ia, ib]).max() > 64


@pytest.mark.parametrize("n,variant,rtol", [(65, "plain", 1e-13), (65, "const", 1e-13), (65, "two", 1e-13), (65, "weights", 1e-13), (257, "weights", 1e-13),
                                            (1000, "plain", 1e-14)])
def test_exact_on_a_noise_free_graph(pgo, n, variant, rtol):
    """every positive-weight measurement comes from the true poses, the start (a noisy chain at weight 0) does not: the truth
    comes back to 1e-9 m once rtol asks for it -- with pose 0, another pose or two poses constant, unit and fractional weights"""
    c = CC.exact_case(n, variant)
    start = run(pgo, c, max_iters=1)[0]
    got, res, _, summ = run(pgo, c, rtol=rtol)
    (d_xy, d_th), d0 = CC.from_truth(got, c), CC.from_truth(start, c)[0]
    print("noise-free %d-%s: %.3e m, %.3e rad from the truth after %s iterations (one iteration from the start: %.3e m)" % (n, variant, d_xy, d_th, summ["solves"][0]["iters"], d0))
    assert d0 > 1e-3                       # the start is not the answer
    assert summ["solves"][0]["converged"] == [1, 1]
    assert d_xy <= 1e-9 and d_th <= 1e-9
    assert res[c["w"] > 0].max() <= 1e-9


def test_errors(pgo):
    c = CC.planted_case(65)
    n, ia, ib, meas, poses = CC.plan_args(c)
    E = len(ia)
    plan = lambda *a, **kw: pgo.chordal_plan(*a, **kw)
    for kw in (dict(rtol=0.0), dict(rtol=np.nan), dict(rtol=np.inf), dict(max_iters=0), dict(check_every=0), dict(mag_min=-1.0), dict(mag_min=np.nan),
               dict(rounds=-1), dict(rounds=pgo.CHORDAL_MAX_ROUNDS + 1), dict(reject_xy=0.0), dict(reject_th=np.nan)):
        with pytest.raises(pgo.PgoError) as e:
            plan(n, ia, ib, meas, poses, w=c["w"], **kw)
        assert e.value.status == INVALID_ARG, kw
    for bad_w in (-0.1, 1.5, np.nan):
        w = c["w"].copy()
        w[9] = bad_w
        with pytest.raises(pgo.PgoError) as e:
            plan(n, ia, ib, meas, poses, w=w)
        assert e.value.status == INVALID_ARG and "edge 9" in str(e.value)
    with pytest.raises(pgo.PgoError) as e:
        plan(1, ia[:0], ib[:0], meas[:0], poses[:1])
    assert e.value.status == INVALID_ARG
    bad_ib = ib.copy()
    bad_ib[70] = n
    with pytest.raises(pgo.PgoError) as e:
        plan(n, ia, bad_ib, meas, poses, w=c["w"])
    assert e.value.status == INVALID_ARG and "edge 70" in str(e.value)
    # null pointers, through the library itself
    L = pgo.lib()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    o, summ = pgo.ChordalOptions(), pgo.ChordalSummary()
    out, res = np.zeros((n, 3)), np.zeros((E, 2))
    m_, p_ = np.ascontiguousarray(meas), np.ascontiguousarray(poses)
    full = [n, E, ia.ctypes.data_as(ip), ib.ctypes.data_as(ip), m_.ctypes.data_as(dp), None, None, p_.ctypes.data_as(dp), C.byref(o),
            out.ctypes.data_as(dp), res.ctypes.data_as(dp), None, C.byref(summ)]
    assert L.pgo_chordal_plan(*full) == 0
    for k in (2, 3, 4, 7, 8, 9, 10, 12):
        args = list(full)
        args[k] = None
        assert L.pgo_chordal_plan(*args) == INVALID_ARG, k
    # a pair without a chain edge, named
    keep = np.ones(E, bool)
    keep[[7, 12]] = False
    with pytest.raises(pgo.PgoError) as e:
        plan(n, ia[keep], ib[keep], meas[keep], poses, w=c["w"][keep])
    assert e.value.status == UNSUPPORTED and "poses 7 and 8" in str(e.value)
    # a component with positive-weight edges and no constant pose: no constant at all, then a half cut off
    with pytest.raises(pgo.PgoError) as e:
        plan(n, ia, ib, meas, poses, w=c["w"], constant=np.zeros(n, bool))
    assert e.value.status == UNSUPPORTED
    h = n // 2
    w = np.where((np.minimum(ia, ib) < h) & (np.maximum(ia, ib) >= h), 0.0, c["w"])
    with pytest.raises(pgo.PgoError) as e:
        plan(n, ia, ib, meas, poses, w=w)
    assert e.value.status == UNSUPPORTED and "pose %d " % h in str(e.value)
    both = np.zeros(n, bool)
    both[[0, n - 1]] = True
    plan(n, ia, ib, meas, poses, w=w, constant=both)              # a constant pose in each half: fine
    w_iso = w.copy()
    w_iso[(ia >= h) | (ib >= h)] = 0.0                            # the second half without any edge: every pose keeps its start
    got = plan(n, ia, ib, meas, poses, w=w_iso)[0]
    X = CC.restate(n, ia, ib, meas, poses, w=w_iso)[3]["X"]
    assert np.abs(got[h:, :2] - X[h:, :2]).max() <= 1e-9 and np.abs(wrap(got[h:, 2] - X[h:, 2])).max() <= 1e-9
    # a measurement that is not finite: on a positive-weight edge or a chain edge -> the smallest such edge; else not looked at
    fam, chain_e = int(c["planted"]["families"][2]), 11
    m = meas.copy()
    m[[fam, chain_e], [0, 2]] = [np.inf, np.nan]
    with pytest.raises(pgo.PgoError) as e:
        plan(n, ia, ib, m, poses, w=c["w"])
    assert e.value.status == NUMERIC and "edge %d " % chain_e in str(e.value)
    m = meas.copy()
    m[fam, 1] = np.nan
    with pytest.raises(pgo.PgoError) as e:
        plan(n, ia, ib, m, poses, w=c["w"])
    assert e.value.status == NUMERIC and "edge %d " % fam in str(e.value)
    w0 = c["w"].copy()
    w0[fam] = 0.0
    got = plan(n, ia, ib, m, poses, w=w0)[0]                      # the same edge at weight 0: fine
    assert np.isfinite(got).all()
    w0 = c["w"].copy()
    w0[chain_e] = 0.0
    m = meas.copy()
    m[chain_e, 0] = np.nan
    with pytest.raises(pgo.PgoError) as e:                        # a chain edge carries the trajectory whatever its weight
        plan(n, ia, ib, m, poses, w=w0)
    assert e.value.status == NUMERIC and "edge %d " % chain_e in str(e.value)


def test_degenerate_poses_fall_back_to_the_trajectory(pgo):
    c = CC.degenerate_case(65)
    h = c["half"]
    want, _, _, info = CC.restate(*CC.plan_args(c), w=c["w"])
    assert info["n_degenerate"] == c["n"] - h and info["min_mag"] < 1e-9 and np.array_equal(info["fallback"], np.arange(h, c["n"]))
    got, res, _, summ = pgo.chordal_plan(*CC.plan_args(c), w=c["w"])
    print("degenerate: min |z| %.3e (restatement %.3e), %d poses" % (summ["min_mag"], info["min_mag"], summ["n_degenerate"]))
    assert summ["n_degenerate"] == c["n"] - h > 0 and summ["min_mag"] < 1e-3
    assert np.abs(got[h:, 2] - info["X"][h:, 2]).max() <= 1e-12     # the headings of the moved trajectory, not wrapped
    assert np.abs(wrap(got[:h, 2] - want[:h, 2])).max() <= 1e-6      # the first half is an ordinary solve
    assert np.isfinite(got).all()
    # a larger floor makes more poses degenerate, none makes none
    assert pgo.chordal_plan(*CC.plan_args(c), w=c["w"], mag_min=0.0)[3]["n_degenerate"] == 0


@pytest.mark.parametrize("n", [65, 257])
def test_reject_rounds_drop_exactly_the_planted_loops(pgo, n):
    c = CC.reject_case(n)
    want, wres, ww, info = CC.restate(*CC.plan_args(c), w=c["w"], rounds=3)
    # the restatement alone, first: exactly the planted loops, no family loop, and the second solve rejects nothing
    assert np.array_equal(info["rejected"], c["bad"]) and info["n_solves"] == 2
    assert not np.isin(c["planted"]["families"], info["rejected"]).any()
    first = CC.restate(*CC.plan_args(c), w=c["w"])[1]
    good = np.ones(len(c["w"]), bool)
    good[c["bad"]] = False
    print("reject-%d: residuals of the planted loops >= %.1f m / %.2f rad, of every other edge <= %.3f m / %.4f rad (thresholds 2 m, 0.35 rad)"
          % (n, first[c["bad"], 0].min(), first[c["bad"], 1].min(), first[good, 0].max(), first[good, 1].max()))
    assert first[c["bad"], 0].min() > 10 * 2.0 and first[good, 0].max() < 2.0 / 5 and first[good, 1].max() < 0.35 / 5
    got, res, w_out, summ = pgo.chordal_plan(*CC.plan_args(c), w=c["w"], rounds=3)
    assert summ["n_solves"] == 2 and summ["n_rejected"] == len(c["bad"])
    assert [s["n_rejected"] for s in summ["solves"]] == [len(c["bad"]), 0]
    assert np.array_equal(w_out, ww) and np.array_equal(np.nonzero(w_out == 0.0)[0], c["bad"])
    CC.compare(got, want, info, RTOL, "reject-%d" % n)
    # rounds = 0 rejects nothing; one round stops after the second solve as well
    assert pgo.chordal_plan(*CC.plan_args(c), w=c["w"])[3]["n_rejected"] == 0
    one = pgo.chordal_plan(*CC.plan_args(c), w=c["w"], rounds=1)
    assert one[3]["n_solves"] == 2 and one[0].tobytes() == got.tobytes()
    # a chain edge is never rejected, whatever its residual
    tiny = pgo.chordal_plan(*CC.plan_args(c), w=c["w"], rounds=1, reject_xy=1e-6, reject_th=1e-6)
    assert (tiny[2][:n - 1] == c["w"][:n - 1]).all() and tiny[3]["n_rejected"] > len(c["bad"])


def test_defaults(pgo):
    o = pgo.ChordalOptions()
    assert (o.rtol, o.max_iters, o.check_every, o.mag_min, o.rounds, o.commit, o.apply_weights) == (1e-8, 20000, 50, 1e-3, 0, 0, 0)
    assert o.reject_xy > 0 and o.reject_th > 0 and pgo.CHORDAL_MAX_ROUNDS == 8
