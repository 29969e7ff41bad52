"""Shared by test_loop_support_host.py, test_loop_support_native.py and test_gpu_loop_support.py: the loop support test of
include/pgo.h ("loop support") restated in numpy straight from its definition -- every pair of selected loops at once,
Err = M_e o O(hi_e, hi_f) o M_f^-1 o O(lo_f, lo_e) in that association, rotations from the angle at every composition --, the
graphs the tests run on, and the comparison of two evaluations."""
import os

import numpy as np

from _coarsen_cases import chain_edges, compose, inverse, relative, wrap
from conftest import GOLDEN

DEFAULTS = dict(window=32, tol_xy=0.1, tol_th=0.05, min_support=1)
PLANTED_N = (65, 257, 513, 1000)
MARGIN = 1e-9    # the smallest |q - 1| over all pairs must exceed this for two evaluations to count the same pairs
# Two evaluations of q differ in rounding and in the association of the compositions: an absolute error d in Err, a few eps
# times the size of the trajectory (<= 1e-12 m on the graphs here), i.e. 2 sqrt(q) d / (tol sqrt(2 + L)) in q.  Relative to q
# that is below 1e-9 for every q above ~1e-6 and meaningless for a q that is itself rounding residue: the planted exact
# duplicates have Err = M o M^-1 = a few eps |M| <= 1e-13 m, q <= 1e-24.  Q_NOISE separates the two: values below it on both
# sides count as the same zero.
Q_NOISE = 1e-20
Q_RTOL = 1e-9


def fixture(n=None):
    """(n_poses, ia, ib, meas, kind) of tests/golden/synth_manhattan_2000_s7.npz, or of its sub-graph "poses < n" """
    z = np.load(os.path.join(GOLDEN, "synth_manhattan_2000_s7.npz"))
    ia, ib, meas, kind = z["ia"], z["ib"], z["meas"], z["kind"]
    if n is None:
        return len(z["poses"]), ia, ib, meas, kind
    keep = (ia < n) & (ib < n)
    return n, ia[keep], ib[keep], meas[keep], kind[keep]


def fixture_graph(pgo, n=None):
    z = np.load(os.path.join(GOLDEN, "synth_manhattan_2000_s7.npz"))
    N, ia, ib, meas, kind = fixture(n)
    return pgo.Graph.from_arrays(z["poses"][:N], ia, ib, meas, kind)


def trajectory(n, ia, ib, meas):
    chain, gap = chain_edges(n, ia, ib)
    assert gap < 0
    T = np.zeros((n, 3))
    for i in range(n - 1):
        e = chain[i]
        T[i + 1] = compose(T[i], meas[e] if ia[e] == i else inverse(meas[e]))
    return chain, T


def restate(n, ia, ib, meas, kind, select=None, window=32, tol_xy=0.1, tol_th=0.05, min_support=1):
    """(records, stats, info): records = a dict of arrays over the edges (selected, n_pairs, n_consistent, best, q_min), stats the
    totals, info = {"margin": the smallest |q - 1| over all pairs, "best_gap": the smallest relative distance between an edge's
    two smallest distinct q (inf with fewer than two), "T": the trajectory}"""
    ia, ib, meas, kind = np.asarray(ia, np.int64), np.asarray(ib, np.int64), np.asarray(meas, np.float64).reshape(-1, 3), np.asarray(kind)
    E = len(ia)
    chain, T = trajectory(n, ia, ib, meas)
    sel = (kind != 0) if select is None else (np.asarray(select).reshape(-1) != 0)
    sel = sel.copy()
    sel[chain[:n - 1]] = False
    idx = np.nonzero(sel)[0]
    lo, hi = np.minimum(ia, ib)[idx], np.maximum(ia, ib)[idx]
    M = np.where((ia[idx] < ib[idx])[:, None], meas[idx], inverse(meas[idx]))
    # every ordered pair (e, f) of selected loops with |lo_e - lo_f| <= window, through the loops sorted by lo
    order = np.argsort(lo, kind="stable")
    slo = lo[order]
    r0, r1 = np.searchsorted(slo, lo - window, "left"), np.searchsorted(slo, lo + window, "right")
    cnt = r1 - r0
    pe = np.repeat(np.arange(len(idx)), cnt)
    pf = order[np.concatenate([np.arange(a, b) for a, b in zip(r0, r1)])] if len(idx) else np.zeros(0, np.int64)
    ok = (pe != pf) & (np.abs(hi[pe] - hi[pf]) <= window)
    pe, pf = pe[ok], pf[ok]

    def O(p, q):
        return compose(inverse(T[p]), T[q])

    Err = compose(compose(compose(M[pe], O(hi[pe], hi[pf])), inverse(M[pf])), O(lo[pf], lo[pe]))
    L = np.abs(lo[pe] - lo[pf]) + np.abs(hi[pe] - hi[pf])
    q = np.maximum((Err[:, 0] ** 2 + Err[:, 1] ** 2) / (tol_xy ** 2 * (2 + L)), wrap(Err[:, 2]) ** 2 / (tol_th ** 2 * (2 + L)))
    fin = np.isfinite(q)
    S = len(idx)
    n_pairs = np.bincount(pe, minlength=S)
    n_cons = np.bincount(pe[fin & (q <= 1.0)], minlength=S)
    q_min, best, gap = np.full(S, -1.0), np.full(S, -1, np.int64), np.full(S, np.inf)
    o2 = np.lexsort((idx[pf[fin]], q[fin], pe[fin]))
    se, sq, sf = pe[fin][o2], q[fin][o2], idx[pf[fin]][o2]
    head = np.nonzero(np.r_[True, se[1:] != se[:-1]])[0] if len(se) else np.zeros(0, np.int64)
    q_min[se[head]], best[se[head]] = sq[head], sf[head]
    # the distance from an edge's smallest q to its next larger one (equal values come from bitwise equal loops -- the planted
    # duplicates -- and are equal in every evaluation: the smaller index wins)
    if len(se):
        grp = np.cumsum(np.r_[True, se[1:] != se[:-1]]) - 1
        larger = np.nonzero(sq > sq[head][grp])[0]
        g2, at = np.unique(grp[larger], return_index=True)
        nxt = sq[larger[at]]
        gap[se[head][g2]] = (nxt - sq[head][g2]) / np.maximum(nxt, Q_NOISE)
    rec = {"selected": np.zeros(E, np.int32), "n_pairs": np.zeros(E, np.int32), "n_consistent": np.zeros(E, np.int32),
           "best": np.full(E, -1, np.int32), "q_min": np.full(E, -1.0)}
    rec["selected"][idx] = 1
    rec["n_pairs"][idx], rec["n_consistent"][idx], rec["best"][idx], rec["q_min"][idx] = n_pairs, n_cons, best, q_min
    stats = {"n_pairs_total": int(n_pairs.sum()), "n_selected": S, "n_supported": int((n_cons >= min_support).sum()),
             "max_pairs": int(n_pairs.max()) if S else 0}
    info = {"margin": float(np.abs(q[fin] - 1.0).min()) if fin.any() else np.inf, "best_gap": float(gap.min()) if S else np.inf, "T": T}
    return rec, stats, info


def assert_same(got, want, info, what=""):
    """two evaluations of the records (structured arrays or dicts of arrays): the integer fields and `best` equal -- under the
    margin conditions, asserted here from the restatement's `info` --, q_min to Q_RTOL relative (Q_NOISE: see above)"""
    print("%s: margin %.3e, best gap %.3e" % (what, info["margin"], info["best_gap"]))
    assert info["margin"] > MARGIN, (what, info["margin"])
    assert info["best_gap"] > 1e-6, (what, info["best_gap"])   # (far above any rounding of q: `best` is decided)
    for k in ("selected", "n_pairs", "n_consistent", "best"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k, np.nonzero(np.asarray(got[k]) != np.asarray(want[k]))[0][:10])
    a, b = np.asarray(got["q_min"], np.float64), np.asarray(want["q_min"], np.float64)
    big = np.maximum(np.abs(a), np.abs(b))
    bad = (np.abs(a - b) > Q_RTOL * big) & (big > Q_NOISE)
    rel = np.abs(a - b)[big > Q_NOISE] / big[big > Q_NOISE]
    print("%s: max relative q_min difference %.3e over %d values above Q_NOISE" % (what, rel.max() if len(rel) else 0.0, len(rel)))
    assert not bad.any(), (what, np.nonzero(bad)[0][:10], a[bad][:10], b[bad][:10])


def planted(n, seed=0):
    """A noisy chain (every fifth edge stored reversed) with families of mutually consistent loops and wrong ones.  Returns a dict:
    n, P (the true poses), ia, ib, meas, kind, select (an explicit selection that also names chain edges and odometry-kind edges
    off the chain), and the edge indices of the planted pieces: families, wrong, dup (an exact duplicate pair of a wrong loop,
    far from every other loop), hub (more than 64 loops at one pose), low / high (families clipped at pose 0 and pose n - 1), odo
    (kind-0 edges that are not chain edges)."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    # (a path that circles: every loop's measurement stays a few metres long, so that the heading noise below, which a long
    # measurement would lever into metres, stays well inside the tolerances)
    th = np.cumsum(0.15 + rng.normal(0, 0.05, n))
    P = np.stack([np.cumsum(np.cos(th)), np.cumsum(np.sin(th)), th], -1)
    P -= P[0]
    i = np.arange(n - 1)
    rev = i % 5 == 4
    ea, eb = list(np.where(rev, i + 1, i)), list(np.where(rev, i, i + 1))
    kind = [0] * (n - 1)
    sig = [(0.02, 0.001)] * (n - 1)
    groups = {k: [] for k in ("families", "wrong", "dup", "hub", "low", "high", "odo")}

    def add(a, b, k, group, s=(0.01, 0.001)):
        groups[group].append(len(ea))
        ea.append(int(a)), eb.append(int(b)), kind.append(k), sig.append(s)

    q = n // 8
    # families: loops between two short stretches of the chain, both orientations
    for a0, b0 in ((q, 5 * q), (2 * q + 3, 6 * q + 1), (q + 2, 3 * q)):
        for k in range(6):
            a, b = a0 + rng.integers(0, 4), b0 + rng.integers(0, 4)
            add(*((a, b) if k % 2 == 0 else (b, a)), 1, "families")
    # clipped windows: lo at 0, 1, 2 with hi in the middle; lo in the middle with hi at n - 1, n - 2, n - 3
    for k in range(3):
        add(k, 4 * q + k, 1, "low")
        add(3 * q + k, n - 1 - k, 1, "high")
    # the hub: 70 loops from one pose to a band of poses (repeats when the band is short)
    band = min(70, n - 7 * q - 1)
    for k in range(70):
        add(q // 2, 7 * q + k % band, 1, "hub")
    # kind-0 edges off the chain: a second copy of a chain pair, a skip edge
    add(q + 1, q + 2, 0, "odo", (0.02, 0.001))
    add(2 * q, 2 * q + 2, 0, "odo", (0.02, 0.001))
    ia, ib = np.array(ea, np.int32), np.array(eb, np.int32)
    meas = relative(P[ia], P[ib])
    meas += rng.normal(0, 1, meas.shape) * np.array([[s[0], s[0], s[1]] for s in sig])
    # wrong loops: beside the first family (evaluated against it, inconsistent), and alone
    extra = [(q + 1, 5 * q + 2, rng.normal(0, 3, 3)), (q + 2, 5 * q + 1, rng.normal(0, 3, 3)), (4 * q + 7, 2 * q + 1, rng.normal(0, 3, 3))]
    # the exact duplicate pair, as far from every other loop as the graph allows: more than 256 poses where it has them (then
    # the two are each other's only neighbour at every window)
    d = (int(rng.integers(3 * q + 4, 4 * q - 2)), int(rng.integers(6 * q + 5, 7 * q - 2)), rng.normal(0, 3, 3))
    ia, ib, meas = list(ia), list(ib), list(meas)
    for a, b, m in extra:
        groups["wrong"].append(len(ia))
        ia.append(a), ib.append(b), meas.append(m), kind.append(2)
    for _ in range(2):
        groups["dup"].append(len(ia))
        ia.append(d[1]), ib.append(d[0]), meas.append(d[2].copy()), kind.append(2)   # (stored with a > b)
    ia, ib, meas, kind = np.array(ia, np.int32), np.array(ib, np.int32), np.array(meas), np.array(kind, np.uint8)
    # the edges grouped by kind, as Graph.from_arrays keeps them (stable: the chain stays 0 .. n - 2)
    order = np.argsort(kind, kind="stable")
    new = np.empty(len(order), np.int64)
    new[order] = np.arange(len(order))
    ia, ib, meas, kind = ia[order], ib[order], meas[order], kind[order]
    groups = {k: [int(new[e]) for e in v] for k, v in groups.items()}
    select = kind != 0
    select[[0, 3, n - 2]] = True          # chain edges: named, never selected
    select[groups["odo"]] = True          # odometry-kind edges off the chain: selected through the mask only
    select[groups["families"][0]] = False   # and a loop left out
    out = {"n": n, "P": P, "ia": ia, "ib": ib, "meas": meas, "kind": kind, "select": select}
    out.update({k: np.array(v, np.int64) for k, v in groups.items()})
    return out


def planted_graph(pgo, c):
    # (initial poses: the truth; loop support never looks at them)
    return pgo.Graph.from_arrays(c["P"], c["ia"], c["ib"], c["meas"], c["kind"])


def as_dict(rec):
    return {k: np.asarray(rec[k]) for k in ("selected", "n_pairs", "n_consistent", "best", "q_min")}
