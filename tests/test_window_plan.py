"""pgo_window_plan (host only): the layer managers' window rule against a numpy restatement, on INTEL + 50 bogus loops (seed 1)."""
import ctypes as C

import numpy as np
import pytest

import _active_cases as AC
import _window_cases as WC


@pytest.fixture(scope="module")
def a(pgo):
    return WC.graph(pgo)[1]


def _same(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert got[0].tolist() == want[0].tolist()
    assert got[1].tolist() == want[1].tolist()
    assert got[2] == want[2]


def test_one_focus_edge_is_the_active_set_window(pgo, a):
    """radius 5 around edge 1233 is _active_cases.window_masks: 22 poses, 21 edges, anchor 39"""
    got = WC.plan(pgo, a, [AC.WINDOW_EDGE], AC.WINDOW_RADIUS)
    _same(got, WC.np_window_plan(a, [AC.WINDOW_EDGE], AC.WINDOW_RADIUS))
    m, pc, anchor = AC.window_masks(a)
    assert len(got[0]) == 22 and len(got[1]) == 21
    assert sorted(got[1].tolist()) == np.nonzero(m)[0].tolist() and got[1][-1] == AC.WINDOW_EDGE
    assert got[0].tolist() == np.unique(np.concatenate([a["ia"][m], a["ib"][m]])).tolist()
    assert got[2] == anchor == AC.WINDOW_ANCHOR


@pytest.mark.parametrize("e", [1227, 1300, 1501, 1532])
def test_radius_10(pgo, a, e):
    got = WC.plan(pgo, a, [e], 10)
    _same(got, WC.np_window_plan(a, [e], 10))
    assert (len(got[0]), len(got[1])) == ((33, 33) if e == 1501 else (42, 41))
    assert np.all(np.diff(got[0]) > 0)


def test_clipping_at_both_ends(pgo, a):
    """no loop edge of this graph ends within 10 poses of pose 0 or N - 1: odometry focus edges there"""
    n = len(a["poses"])
    assert (a["ia"][2], a["ib"][2]) == (2, 3) and (a["ia"][1224], a["ib"][1224]) == (1224, 1225)
    for e in (0, 2, 1224, 1226):
        got = WC.plan(pgo, a, [e], 10)
        _same(got, WC.np_window_plan(a, [e], 10))
        assert len(set(got[1].tolist())) == len(got[1])      # the focus edge is an odometry edge: listed once
    p, ed, an = WC.plan(pgo, a, [2], 10)
    assert p.tolist() == list(range(0, 14)) and an == 0 and ed.tolist() == list(range(0, 13))
    p, ed, an = WC.plan(pgo, a, [1224], 10)
    assert p.tolist() == list(range(1214, n)) and an == 1214 and ed.tolist() == list(range(1214, 1227))


def test_two_focus_edges_with_overlapping_ranges(pgo, a):
    got = WC.plan(pgo, a, [1500, 1501], 10)
    _same(got, WC.np_window_plan(a, [1500, 1501], 10))
    assert len(got[0]) == 75 and got[1][-2:].tolist() == [1500, 1501]
    got = WC.plan(pgo, a, [1501, 1500], 10)
    assert got[1][-2:].tolist() == [1501, 1500]
    near = [e for e in WC.LOOP_EDGES if e != 1233 and abs(int(a["ia"][e]) - int(a["ia"][1233])) <= 4]
    if near:
        _same(WC.plan(pgo, a, [1233, near[0]], 5), WC.np_window_plan(a, [1233, near[0]], 5))


def test_repeated_focus_edge(pgo, a):
    _same(WC.plan(pgo, a, [1300, 1300, 1300], 10), WC.plan(pgo, a, [1300], 10))
    _same(WC.plan(pgo, a, [1300, 1233, 1300], 7), WC.np_window_plan(a, [1300, 1233, 1300], 7))


def test_no_focus_edge_is_an_empty_window(pgo, a):
    p, e, an = WC.plan(pgo, a, [], 10)
    assert len(p) == 0 and len(e) == 0 and an == -1


@pytest.mark.parametrize("pose_cap,edge_cap", [(41, 41), (42, 40), (0, 0)])
def test_caps_too_small_return_the_counts_and_the_error(pgo, a, pose_cap, edge_cap):
    with pytest.raises(pgo.PgoError) as ei:
        pgo.window_plan(len(a["poses"]), a["ia"], a["ib"], a["kind"], [1300], 10, pose_cap=pose_cap, edge_cap=edge_cap)
    assert ei.value.status == -1 and (ei.value.n_poses, ei.value.n_edges) == (42, 41)
    p, e, an = pgo.window_plan(len(a["poses"]), a["ia"], a["ib"], a["kind"], [1300], 10, pose_cap=42, edge_cap=41)
    assert len(p) == 42 and len(e) == 41


def test_caps_at_the_c_abi_leave_the_lists_alone(pgo, a):
    L = pgo.lib()
    ia, ib, kind = (np.ascontiguousarray(a[k]) for k in ("ia", "ib", "kind"))
    fe = np.array([1300], np.int32)
    po, eo = np.full(64, -7, np.int32), np.full(64, -7, np.int32)
    npo, neo, an = C.c_int32(), C.c_int32(), C.c_int32(-7)
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
    st = L.pgo_window_plan(len(a["poses"]), len(ia), ip(ia), ip(ib), kind.ctypes.data_as(C.POINTER(C.c_uint8)), 1, ip(fe), 10,
                           41, ip(po), C.byref(npo), 64, ip(eo), C.byref(neo), C.byref(an))
    assert st == -1 and (npo.value, neo.value) == (42, 41)
    assert (po == -7).all() and (eo == -7).all() and an.value == -7


def test_bad_arguments(pgo, a):
    n = len(a["poses"])
    for focus, radius in (([len(a["ia"])], 10), ([-1], 10), ([1300], -1)):
        with pytest.raises(pgo.PgoError) as ei:
            pgo.window_plan(n, a["ia"], a["ib"], a["kind"], focus, radius)
        assert ei.value.status == -1


def test_binding_reads_the_caps_from_the_header(pgo):
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "pgo.h")).read()
    caps = {k: int(v) for k, v in re.findall(r"#define PGO_WINDOW_MAX_(\w+)\s+(\d+)", text)}
    assert (pgo.WINDOW_MAX_POSES, pgo.WINDOW_MAX_EDGES, pgo.WINDOW_MAX_ITERS) == (caps["POSES"], caps["EDGES"], caps["ITERS"])
    assert pgo.WINDOW_MAX_POSES >= 48
