"""pgo_active_plan (host logic of pgo_set_active / pgo_batch_set_active) against a numpy restatement, and the exported
surface of the active-set feature.  No GPU."""
import ctypes

import numpy as np
import pytest

import _active_cases as AC


def _check(pgo, n, ia, ib, ea, pc, fixed):
    const, n_act, n_free = pgo.active_plan(n, ia, ib, ea, pc, fixed)
    rc, ra, rf = AC.plan(n, ia, ib, ea, pc, fixed)
    np.testing.assert_array_equal(const, rc)
    assert (n_act, n_free) == (ra, rf)
    assert n_free == n - int(const.sum())
    return const, n_act, n_free


def test_new_symbols_are_exported(pgo):
    for sym in ("pgo_set_active", "pgo_batch_set_active", "pgo_active_plan"):
        assert sym in pgo.EXPORTS and getattr(pgo.lib(), sym) is not None
    assert callable(pgo.active_plan) and "active_plan" in pgo.__all__
    assert callable(pgo.Solver.set_active) and callable(pgo.Batch.set_active)
    names = [f[0] for f in pgo.HandleInfo._fields_]
    assert names[-2:] == ["n_active_edges", "n_constant_poses"]      # appended at the end
    assert ctypes.sizeof(pgo.HandleInfo) % 8 == 0


def test_plan_on_the_intel_cases(pgo):
    a = AC.arrays(AC.intel(pgo))
    n, ia, ib = len(a["poses"]), a["ia"], a["ib"]
    assert (n, len(ia)) == (AC.N_INTEL, AC.E_INTEL)
    assert [int((a["kind"] == k).sum()) for k in (0, 1, 2)] == [1227, 256, 50]
    # layer: 1363 edges, every pose used -> only opt.fixed_pose is constant
    lm = AC.layer_mask(a["kind"])
    const, n_act, n_free = _check(pgo, n, ia, ib, lm, None, 0)
    assert n_act == 1363 and n_free == n - 1 and const[0] == 1
    # window: 22 poses in two fragments joined by the loop alone, 21 edges, anchor 39; fixed_pose 0 lies outside
    wm, pc, anchor = AC.window_masks(a)
    assert anchor == AC.WINDOW_ANCHOR and (int(ia[AC.WINDOW_EDGE]), int(ib[AC.WINDOW_EDGE])) == (44, 189)
    const, n_act, n_free = _check(pgo, n, ia, ib, wm, pc, 0)
    used = np.nonzero(const == 0)[0]
    assert n_act == 21 and n_free == 21
    assert set(used) == (set(range(39, 50)) | set(range(184, 195))) - {39}
    # the layer mask with more constant poses
    pc2 = np.zeros(n, np.uint8)
    pc2[[5, 64, 600, 1227]] = 1
    const, _, n_free = _check(pgo, n, ia, ib, lm, pc2, 0)
    assert n_free == n - 5
    # all-NULL, nothing active, no constant pose at all
    const, n_act, n_free = _check(pgo, n, ia, ib, None, None, 0)
    assert n_act == len(ia) and n_free == n - 1
    const, n_act, n_free = _check(pgo, n, ia, ib, np.zeros(len(ia), np.uint8), None, 0)
    assert n_act == 0 and n_free == 0 and const.all()
    _, _, n_free = _check(pgo, n, ia, ib, None, None, -1)
    assert n_free == n


def test_plan_on_a_toy_graph(pgo):
    ia, ib = np.array([0, 1, 2, 0], np.int32), np.array([1, 2, 3, 3], np.int32)
    for ea in (None, [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 1, 1], [0, 0, 0, 0], [2, 0, 255, 0]):
        for pc in (None, [0, 0, 0, 0], [0, 1, 0, 0], [1, 1, 1, 1]):
            for fixed in (-1, 0, 3):
                _check(pgo, 4, ia, ib, ea, pc, fixed)
    const, n_act, n_free = pgo.active_plan(4, ia, ib, [1, 0, 0, 0], None, 0)
    assert list(const) == [1, 0, 1, 1] and (n_act, n_free) == (1, 1)
    # an isolated pose is constant without any mask
    const, _, _ = pgo.active_plan(5, ia, ib, None, None, 0)
    assert list(const) == [1, 0, 0, 0, 1]


def test_plan_rejects_bad_arguments(pgo):
    ia, ib = np.array([0, 1], np.int32), np.array([1, 2], np.int32)
    for args in ((0, ia[:0], ib[:0], None, None, 0), (3, ia, ib, None, None, 3), (2, ia, ib, None, None, 0)):
        with pytest.raises(pgo.PgoError) as e:
            pgo.active_plan(*args)
        assert e.value.status == -1
    with pytest.raises(ValueError):
        pgo.active_plan(3, ia, ib, [1], None, 0)
