"""pgo_loop_support_plan (host only), the serial statement of the loop support test (include/pgo.h, "loop support";
csrc/loop_support.h), against the numpy restatement of tests/_support_cases.py: on the synthetic fixture, whole and restricted
to its first 500 poses, with what the test finds there pinned; on planted graphs with every shape the definition names; and
every error of its list."""
import ctypes as C

import numpy as np
import pytest

import _support_cases as SC

INVALID_ARG, NUMERIC, UNSUPPORTED = -1, -7, -8
EPS = np.finfo(np.float64).eps


def check(pgo, n, ia, ib, meas, kind, what, select=None, **opt):
    kw = dict(SC.DEFAULTS, **opt)
    got, gstats, T = pgo.loop_support_plan(n, ia, ib, meas, kind, select=select, want_T=True, **kw)
    want, wstats, info = SC.restate(n, ia, ib, meas, kind, select=select, **kw)
    SC.assert_same(got, want, info, what)
    assert gstats == wstats, (what, gstats, wstats)
    # T: n compositions, each rounding a pose of size <= |T|max a few times, and turning what follows by the angle's rounding
    tol = 8 * n * EPS * max(1.0, np.abs(info["T"]).max())
    assert np.abs(T - info["T"]).max() <= tol, (what, np.abs(T - info["T"]).max(), tol)
    assert T[0].tobytes() == np.zeros(3).tobytes()
    return got, gstats


@pytest.mark.parametrize("n", [None, 500], ids=["whole", "first-500"])
def test_fixture_against_restatement_and_pins(pgo, n):
    N, ia, ib, meas, kind = SC.fixture(n)
    got, stats = check(pgo, N, ia, ib, meas, kind, "fixture %s" % n)
    bogus, closure = kind == 2, kind == 1
    assert (got["selected"][kind != 0] == 1).all() and (got["selected"][kind == 0] == 0).all()
    if n is None:
        assert stats["n_selected"] == 5845 and bogus.sum() == 531 and closure.sum() == 5314
        assert (got["n_consistent"][bogus] > 0).sum() == 0
        assert (got["n_consistent"][closure] == 0).sum() == 9
        assert stats["max_pairs"] == 143
        assert stats["n_supported"] == 5314 - 9
    else:
        assert bogus.sum() == 35 and closure.sum() == 921
        assert (got["n_consistent"][bogus] > 0).sum() == 0
        assert (got["n_consistent"][closure] == 0).sum() == 2
        assert stats["n_supported"] == 921 - 2


@pytest.fixture(scope="module", params=SC.PLANTED_N)
def case(request):
    return SC.planted(request.param)


def arrays(c):
    return c["n"], c["ia"], c["ib"], c["meas"], c["kind"]


def test_planted_defaults(pgo, case):
    c = case
    got, stats = check(pgo, *arrays(c), "planted %d" % c["n"])
    chain = np.arange(c["n"] - 1)
    assert (got["selected"][chain] == 0).all() and (got["selected"][c["odo"]] == 0).all()
    assert (got["n_consistent"][c["wrong"]] == 0).all() and (got["n_pairs"][c["wrong"][:2]] > 0).all()
    for g in ("families", "low", "high", "hub"):
        assert (got["n_consistent"][c[g]] >= 1).all(), g
    # loops stored with a > b take part like the others
    back = c["families"][c["ia"][c["families"]] > c["ib"][c["families"]]]
    assert len(back) >= 3 and (got["n_consistent"][back] >= 1).all()
    # the exact duplicates: each supports the other, q = 0 up to the rounding of M o M^-1
    d0, d1 = c["dup"]
    assert got["best"][d0] == d1 and got["best"][d1] == d0
    assert 0.0 <= got["q_min"][d0] <= SC.Q_NOISE and 0.0 <= got["q_min"][d1] <= SC.Q_NOISE
    assert got["n_consistent"][d0] == 1 and got["n_consistent"][d1] == 1
    # an unselected edge's record
    for k, v in (("n_pairs", 0), ("n_consistent", 0), ("best", -1), ("q_min", -1.0)):
        assert (got[k][chain] == v).all(), k


@pytest.mark.parametrize("window", [1, 256])
def test_planted_windows(pgo, case, window):
    c = case
    got, stats = check(pgo, *arrays(c), "planted %d window %d" % (c["n"], window), window=window)
    if window == 256:   # the hub: every loop of it sees the 69 others
        assert len(c["hub"]) == 70 and (got["n_pairs"][c["hub"]] >= 69).all() and stats["max_pairs"] >= 69
    else:               # window 1: only loops whose ends are both within one pose
        lo, hi = np.minimum(c["ia"], c["ib"]), np.maximum(c["ia"], c["ib"])
        for e in np.nonzero(got["n_pairs"] > 0)[0]:
            f = got["best"][e]
            assert f < 0 or (abs(lo[e] - lo[f]) <= 1 and abs(hi[e] - hi[f]) <= 1)
    # clipped ranges at pose 0 and pose n - 1 are in the comparison above; they hold loops
    assert (got["n_pairs"][c["low"]] > 0).any() or window == 1
    assert (got["selected"][c["low"]] == 1).all() and (got["selected"][c["high"]] == 1).all()


def test_planted_explicit_selection_and_min_support(pgo, case):
    c = case
    got, stats = check(pgo, *arrays(c), "planted %d select" % c["n"], select=c["select"], min_support=2)
    n = c["n"]
    assert (got["selected"][[0, 3, n - 2]] == 0).all()            # chain edges named by the mask: not selected, no error
    assert (got["selected"][c["odo"]] == 1).all()                 # odometry-kind edges off the chain: selected by the mask
    assert got["selected"][c["families"][0]] == 0                 # a loop the mask leaves out
    assert not np.isin(got["best"], [c["families"][0]]).any()     # ... is nobody's neighbour
    want_supported = int(((got["n_consistent"] >= 2) & (got["selected"] == 1)).sum())
    assert stats["n_supported"] == want_supported
    one = pgo.loop_support_plan(*arrays(c), select=c["select"], min_support=1)[1]
    assert one["n_supported"] == int(((got["n_consistent"] >= 1) & (got["selected"] == 1)).sum()) > want_supported


def test_errors(pgo):
    c = SC.planted(65)
    n, ia, ib, meas, kind = arrays(c)
    plan = pgo.loop_support_plan
    for kw in (dict(window=0), dict(window=257), dict(window=-3), dict(tol_xy=0.0), dict(tol_xy=-1.0), dict(tol_xy=np.nan),
               dict(tol_xy=np.inf), dict(tol_th=0.0), dict(tol_th=np.nan), dict(tol_th=np.inf), dict(min_support=0), dict(min_support=-1)):
        with pytest.raises(pgo.PgoError) as e:
            plan(n, ia, ib, meas, kind, **kw)
        assert e.value.status == INVALID_ARG, kw
    plan(n, ia, ib, meas, kind, window=1, min_support=5)
    plan(n, ia, ib, meas, kind, window=256)
    with pytest.raises(pgo.PgoError) as e:                        # n_poses < 2
        plan(1, ia[:0], ib[:0], meas[:0], kind[:0])
    assert e.value.status == INVALID_ARG
    plan(2, ia[:1], ib[:1], meas[:1], kind[:1])                   # the smallest graph
    bad_ib = ib.copy()
    bad_ib[70] = n
    with pytest.raises(pgo.PgoError) as e:
        plan(n, ia, bad_ib, meas, kind)
    assert e.value.status == INVALID_ARG and "edge 70" in str(e.value)
    # null pointers, through the library itself
    L = pgo.lib()
    E = len(ia)
    o = pgo.LoopSupportOptions()
    res, st = (pgo.LoopSupportRecord * E)(), pgo.LoopSupportStats()
    ip, dp, bp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    full = [n, E, ia.ctypes.data_as(ip), ib.ctypes.data_as(ip), np.ascontiguousarray(meas).ctypes.data_as(dp), kind.ctypes.data_as(bp), None,
            C.byref(o), res, C.byref(st), None]
    assert L.pgo_loop_support_plan(*full) == 0
    for k in (2, 3, 4, 5, 7, 8, 9):
        args = list(full)
        args[k] = None
        assert L.pgo_loop_support_plan(*args) == INVALID_ARG, k
    # a pair without a chain edge, named
    keep = np.ones(E, bool)
    keep[[7, 12]] = False
    with pytest.raises(pgo.PgoError) as e:
        plan(n, ia[keep], ib[keep], meas[keep], kind[keep])
    assert e.value.status == UNSUPPORTED and "poses 7 and 8" in str(e.value)
    # a measurement that is not finite: selected or chain -> the smallest such edge; any other edge is not looked at
    sel_e, chain_e, odo_e = int(c["families"][2]), 11, int(c["odo"][1])
    m = meas.copy()
    m[odo_e, 1] = np.nan                                          # kind 0, off the chain: not selected by default
    plan(n, ia, ib, m, kind)
    with pytest.raises(pgo.PgoError) as e:                        # ... selected by a mask
        plan(n, ia, ib, m, kind, select=c["select"])
    assert e.value.status == NUMERIC and "edge %d " % odo_e in str(e.value)
    m = meas.copy()
    m[[sel_e, chain_e], [0, 2]] = [np.inf, np.nan]
    with pytest.raises(pgo.PgoError) as e:
        plan(n, ia, ib, m, kind)
    assert e.value.status == NUMERIC and "edge %d " % chain_e in str(e.value)
    m = meas.copy()
    m[sel_e, 0] = np.inf
    with pytest.raises(pgo.PgoError) as e:
        plan(n, ia, ib, m, kind)
    assert e.value.status == NUMERIC and "edge %d " % sel_e in str(e.value)
    unsel = np.ones(E, bool)
    unsel[sel_e] = False
    plan(n, ia, ib, m, kind, select=unsel)                        # the same edge left out of the selection: fine


def test_defaults(pgo):
    o = pgo.LoopSupportOptions()
    assert (o.window, o.min_support, o.apply, o.tol_xy, o.tol_th) == (32, 1, 0, 0.1, 0.05)
    assert pgo.LOOP_SUPPORT_MAX_WINDOW == 256
