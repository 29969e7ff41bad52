"""Shared inputs of the window-solve tests (pgo_window_plan / pgo_window_solve): INTEL + 50 bogus loops (seed 1, the graph of
_active_cases), the numpy restatement of the window rule, and the CPU oracle on the EXTRACTED problem -- the listed poses
renumbered by list position, the listed edges in list order -- which is what the window kernel is compared with (never with
itself).  Oracle results are computed once per process and shared."""
import numpy as np

import _active_cases as AC

LOOP_EDGES = range(1227, 1533)        # the closure and bogus edges of INTEL + 50
SWEEP_RADIUS, SWEEP_ITERS = 10, 4

_cache = {}


def graph(pgo):
    """(Graph, arrays) of INTEL + 50, once per process"""
    if "g" not in _cache:
        g = AC.intel(pgo)
        _cache["g"] = (g, AC.arrays(g))
    return _cache["g"]


def np_window_plan(a, focus, radius):
    """numpy restatement of pgo_window_plan: (pose_idx, edge_idx, anchor)"""
    ia, ib, kind = a["ia"], a["ib"], a["kind"]
    n = len(a["poses"])
    act = np.zeros(n, bool)
    for e in focus:
        for c in (int(ia[e]), int(ib[e])):
            act[max(0, c - radius):min(n - 1, c + radius) + 1] = True
    edges = list(np.nonzero((kind == 0) & act[ia] & act[ib])[0])
    for e in focus:
        if ia[e] != ib[e] and e not in edges:
            edges.append(int(e))
    edges = np.array(edges, np.int64)
    poses = np.unique(np.concatenate([ia[edges], ib[edges]])) if len(edges) else np.zeros(0, np.int64)
    anchor = -1 if len(poses) == 0 else (0 if poses[0] == 0 else int(poses[0]))
    return poses.astype(np.int32), edges.astype(np.int32), anchor


def plan(pgo, a, focus, radius):
    return pgo.window_plan(len(a["poses"]), a["ia"], a["ib"], a["kind"], focus, radius)


def extracted(O, a, win, poses=None):
    """(oracle Graph of the window in list numbering, constant mask): pose k = the k-th listed pose, edge k = the k-th listed
    edge (a twice-listed edge is two residual blocks); constant = the anchor and the listed poses without a listed edge"""
    pidx, eidx, anchor = (np.asarray(win[0], np.int64), np.asarray(win[1], np.int64), int(win[2]))
    x = a["poses"] if poses is None else poses
    pos = -np.ones(len(a["poses"]), np.int64)
    pos[pidx] = np.arange(len(pidx))
    ia, ib = pos[a["ia"][eidx]], pos[a["ib"][eidx]]
    assert (ia >= 0).all() and (ib >= 0).all()
    g = O.Graph(np.arange(len(pidx), dtype=np.int32), np.array(x[pidx], np.float64), ia.astype(np.int32), ib.astype(np.int32),
                np.array(a["meas"][eidx]), np.array(a["info"][eidx]), np.array(a["kind"][eidx]))
    const = np.ones(len(pidx), bool)
    const[ia] = False
    const[ib] = False
    const[pos[anchor]] = True
    return g, const


def oracle_window(O, a, win, method, max_iters, poses=None):
    """the oracle's LM on the extracted window: dict(poses (list order), termination, iterations, successful_steps, initial_cost,
    final_cost, hist (step_ok per record), records or None)"""
    g, const = extracted(O, a, win, poses)
    if const.sum() == 1:
        r = O.lm_direct(g, O.Options(method=method, max_iters=max_iters, fixed_pose=int(np.nonzero(const)[0][0])))
        return dict(poses=r.poses, termination=r.termination, iterations=r.iterations, successful_steps=r.successful_steps,
                    initial_cost=r.initial_cost, final_cost=r.final_cost, hist=[q["step_ok"] for q in r.records], records=r.records)
    opt = O.Options(method=method, max_iters=max_iters, fixed_pose=-1)
    x, term, it, cost, hist = AC.lm_direct_const(O, g, opt, const)
    c0 = O.evaluate(g, None, method, opt.phi, opt.huber_delta, True, False, False)[0]
    return dict(poses=x, termination=term, iterations=it, successful_steps=int(sum(1 for h in hist[1:] if h == 1)),
                initial_cost=c0, final_cost=cost, hist=list(hist), records=None)


def sweep(pgo, O, method):
    """the 306 loop windows window_plan([e], 10) and the oracle's result for each (max_iters 4), once per process"""
    key = ("sweep", method)
    if key not in _cache:
        _, a = graph(pgo)
        if "sweep_windows" not in _cache:
            _cache["sweep_windows"] = [plan(pgo, a, [e], SWEEP_RADIUS) for e in LOOP_EDGES]
        wins = _cache["sweep_windows"]
        _cache[key] = (wins, [oracle_window(O, a, w, method, SWEEP_ITERS) for w in wins])
    return _cache[key]


def check_against_oracle(got_poses, got, recs, ref, what=""):
    """the issue's bounds (test_gpu_active.py::test_lm_parity's): decisions equal, initial cost 1e-12 relative, poses 1e-6, final
    cost 1e-7 relative with an absolute floor of 1e-9 x the initial cost.  Returns (|d pose|, |d final cost| / scale)."""
    assert [r["step_ok"] for r in recs] == ref["hist"], what
    assert (got.termination, got.iterations, got.successful_steps) == (ref["termination"], ref["iterations"], ref["successful_steps"]), what
    assert got.n_records == len(ref["hist"]), what
    assert abs(got.initial_cost - ref["initial_cost"]) <= 1e-12 * abs(ref["initial_cost"]), what
    dp = float(np.abs(got_poses - ref["poses"]).max())
    assert dp < 1e-6, what
    tol = max(1e-7 * abs(ref["final_cost"]), 1e-9 * abs(ref["initial_cost"]))
    dc = abs(got.final_cost - ref["final_cost"])
    assert dc <= tol, f"{what}: final cost {got.final_cost!r} vs {ref['final_cost']!r}"
    return dp, dc / tol
