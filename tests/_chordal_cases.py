"""Shared by test_chordal_host.py, test_chordal_native.py and test_gpu_chordal.py: the chordal initialisation of include/pgo.h
("chordal initialisation") restated in numpy / scipy straight from its definition -- H and b of both stages built from the
edge list, the constant rows eliminated, a sparse DIRECT solve (dense numpy.linalg.solve without scipy) --, the graphs the
tests run on, and the bound within which an evaluation that stops at |r| <= rtol |b| must agree with it."""
import numpy as np

import _support_cases as SC
from _coarsen_cases import compose, inverse, relative, wrap

try:
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
except ImportError:   # pragma: no cover
    sp = spl = None

EPS = np.finfo(np.float64).eps


def _solve(H, rhs):
    """(x, smallest eigenvalue, largest eigenvalue) of the Hermitian positive definite H (dense array in, any size here)"""
    if len(rhs) == 0:
        return np.zeros(0, complex), np.inf, 0.0
    ev = np.linalg.eigvalsh(H) if len(rhs) <= 1200 else None
    if sp is not None:
        x = spl.spsolve(sp.csc_matrix(H), rhs)
        if ev is None:
            lo = spl.eigsh(sp.csc_matrix(H), k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]
            hi = spl.eigsh(sp.csc_matrix(H), k=1, which="LA", return_eigenvectors=False)[0]
            return x, float(lo), float(hi)
    else:
        x = np.linalg.solve(H, rhs)
        if ev is None:
            ev = np.linalg.eigvalsh(H)
    return x, float(ev[0]), float(ev[-1])


def _stage(n, ia, ib, u, phi, g, free, x_fixed):
    """H x = b of one stage: x on the free rows, the other rows keep x_fixed.  phi, g: per edge."""
    H = np.zeros((n, n), complex)
    b = np.zeros(n, complex)
    for e in np.nonzero(u > 0)[0]:
        a, c = ia[e], ib[e]
        H[a, a] += u[e]
        H[c, c] += u[e]
        H[c, a] -= u[e] * phi[e]
        H[a, c] -= u[e] * np.conj(phi[e])
        b[c] += g[e]
        b[a] -= g[e]
    f = np.nonzero(free)[0]
    k = np.nonzero(~free)[0]
    rhs = b[f] - H[np.ix_(f, k)] @ x_fixed[k]
    xf, lo, hi = _solve(H[np.ix_(f, f)], rhs)
    x = x_fixed.copy()
    x[f] = xf
    return x, {"lam_min": lo, "lam_max": hi, "b_norm": float(np.linalg.norm(rhs)), "x_norm": float(np.linalg.norm(xf))}


def _lever(n, ia, ib, u, meas):
    """the 2-norm of M, b_T = M zh: M[b, a] += u m, M[a, a] -= u m over the edges (a, b, m)"""
    M = np.zeros((n, n), complex)
    um = u * (meas[:, 0] + 1j * meas[:, 1])
    np.add.at(M, (ib[u > 0], ia[u > 0]), um[u > 0])
    np.add.at(M, (ia[u > 0], ia[u > 0]), -um[u > 0])
    if spl is not None and n > 400:
        return float(spl.svds(sp.csc_matrix(M), k=1, return_singular_vectors=False)[0])
    return float(np.linalg.norm(M, 2))


def restate(n, ia, ib, meas, poses, w=None, constant=None, mag_min=1e-3, rounds=0, reject_xy=2.0, reject_th=0.35):
    """(poses (n, 3), res (E, 2), w_out (E), info): info = {"R", "T": the stage dicts of the last solve, "min_mag",
    "n_degenerate", "n_rejected", "rejected": the edges the rounds dropped, "n_solves", "fallback": the degenerate poses}"""
    ia, ib = np.asarray(ia, np.int64), np.asarray(ib, np.int64)
    meas, poses = np.asarray(meas, np.float64).reshape(-1, 3), np.asarray(poses, np.float64).reshape(-1, 3)
    E = len(ia)
    w0 = np.ones(E) if w is None else np.asarray(w, np.float64).copy()
    u = np.where(ia != ib, w0, 0.0)
    C = np.zeros(n, bool)
    if constant is None:
        C[0] = True
    else:
        C[:] = np.asarray(constant).reshape(-1) != 0
    c0 = int(np.nonzero(C)[0][0])
    chain, T = SC.trajectory(n, ia, ib, meas)
    is_chain = np.zeros(E, bool)
    is_chain[chain[:n - 1]] = True
    X = compose(compose(poses[c0], inverse(T[c0]))[None, :], T)
    X[:, 2] = poses[c0, 2] - T[c0, 2] + T[:, 2]   # (the heading is a plain sum, not wrapped)
    rejected = np.zeros(E, bool)
    for r in range(rounds + 1):
        deg = np.bincount(ia[u > 0], minlength=n) + np.bincount(ib[u > 0], minlength=n)
        free = ~C & (deg > 0)
        z_fixed = np.where(C, np.exp(1j * poses[:, 2]), np.exp(1j * X[:, 2]))
        z, iR = _stage(n, ia, ib, u, np.exp(1j * meas[:, 2]), np.zeros(E, complex), free, z_fixed)
        mag = np.abs(z)
        degen = ~C & ~(mag >= mag_min)
        theta = np.where(C, poses[:, 2], np.where(degen, X[:, 2], np.angle(z)))
        zh = np.where(C | degen, np.exp(1j * theta), z / np.where(mag > 0, mag, 1.0))
        t_fixed = np.where(C, poses[:, 0] + 1j * poses[:, 1], X[:, 0] + 1j * X[:, 1])
        t, iT = _stage(n, ia, ib, u, np.ones(E, complex), u * zh[ia] * (meas[:, 0] + 1j * meas[:, 1]), free, t_fixed)
        out = np.stack([t.real, t.imag, theta], -1)
        out[C] = poses[C]
        res = np.stack([np.abs(t[ib] - t[ia] - zh[ia] * (meas[:, 0] + 1j * meas[:, 1])), np.abs(wrap(theta[ib] - theta[ia] - meas[:, 2]))], -1)
        new = np.zeros(E, bool)
        if r < rounds:
            new = (u > 0) & ~is_chain & ~((res[:, 0] <= reject_xy) & (res[:, 1] <= reject_th))
        u[new] = 0.0
        rejected |= new
        n_solves = r + 1
        if not new.any():
            break
    info = {"R": iR, "T": iT, "min_mag": float(mag[~C].min()) if (~C).any() else np.inf, "n_degenerate": int(degen.sum()),
            "n_rejected": int(rejected.sum()), "rejected": np.nonzero(rejected)[0], "n_solves": n_solves, "fallback": np.nonzero(degen)[0],
            "X": X, "u": u, "free": free, "zh_lever": _lever(n, ia, ib, u, meas)}
    return out, res, np.where(rejected, 0.0, w0), info


def bounds(info, rtol, solves=1):
    """(bound on |heading difference|, bound on |position difference|) between the restatement (a direct solve) and `solves`
    evaluations that each stop at |r| <= rtol |b| (1: an evaluation against the restatement; 2: two evaluations against each
    other), from the restatement's own figures:
      stage R   |z - z*|_2 <= |r| / lam_min <= rtol |b_R| / lam_min_R =: dz, plus the direct solve's and the products' rounding,
                64 eps (lam_max / lam_min) |z|_2;
                a heading moves by at most asin(dz / |z_i|) <= (pi / 2) dz / min_mag, zh_i by at most 2 dz / min_mag;
      stage T   |t - t*|_2 <= rtol |b_T| / lam_min_T + |db|_2 / lam_min_T + rounding, where db is what the change of zh does to b:
                b_T = M zh with M[b, a] += u m, M[a, a] -= u m over the edges, so |db|_2 <= |M|_2 |dzh|_2 <= |M|_2 2 dz / min_mag.
    A 2-norm over the poses bounds every pose.  These are worst cases -- the whole residual along the softest mode of a long
    chain -- and far above what is measured (printed by compare); the sharp checks are the noise-free graphs (exact_case: the truth
    to 1e-9 m) and, between the plan and the device, rounding_bounds()."""
    R, T = info["R"], info["T"]
    rnd = lambda S: 64 * EPS * (S["lam_max"] / S["lam_min"]) * S["x_norm"]
    dz = solves * rtol * R["b_norm"] / R["lam_min"] + rnd(R)
    mm = min(info["min_mag"], 1.0)
    assert dz < 0.5 * mm, (dz, mm)   # (the linearisations above hold)
    b_th = 0.5 * np.pi * dz / mm
    db = info["zh_lever"] * 2.0 * dz / mm
    b_xy = solves * rtol * T["b_norm"] / T["lam_min"] + db / T["lam_min"] + rnd(T)
    return float(b_th), float(b_xy)


def rounding_bounds(info):
    """(heading bound, position bound) between two evaluations of the SAME recurrence that made the same number of iterations
    in both stages -- pgo_chordal_plan and the device: one statement (csrc/chordal.h), the same operands and the same slot
    order in every row product, sums of the dot products in another order (serial against fixed trees) and another contraction
    into fused multiply-adds.  No residual enters: what differs is rounding alone, an eps-sized relative change of every scalar
    and vector of an iteration, which a system of condition lam_max / lam_min turns into at most eps (lam_max / lam_min) |x|_2
    per unit of such change.  bounds() already grants one evaluation 64 of these units for its rounding; the same 64 stand here
    for the two evaluations together:
      stage R   dz = 64 eps (lam_max / lam_min) |z|_2, a heading moves by at most (pi / 2) dz / min_mag      (as in bounds)
      stage T   is linear in zh: t = H_T^-1 M zh.  What the two evaluations' DIFFERENT headings do to the positions is therefore
                known exactly, H_T^-1 M (zh' - zh) (compare_rounding solves for it directly), and is taken out; what is left is
                stage T's own rounding, 64 eps (lam_max / lam_min) |t|_2.
    Orders below what rtol gives: 4e-10 to 2e-6 rad and 2e-9 to 1.3e-5 m on the graphs of the tests."""
    R, T = info["R"], info["T"]
    rnd = lambda S: 64 * EPS * (S["lam_max"] / S["lam_min"]) * S["x_norm"]
    return float(0.5 * np.pi * rnd(R) / min(info["min_mag"], 1.0)), float(rnd(T))


def _response(c, info, dzh):
    """H_T^-1 M dzh on the free rows of the restatement's last solve, 0 elsewhere (a direct solve)"""
    n, ia, ib, u = c["n"], np.asarray(c["ia"], np.int64), np.asarray(c["ib"], np.int64), info["u"]
    g = u * dzh[ia] * (c["meas"][:, 0] + 1j * c["meas"][:, 1])
    H = np.zeros((n, n))
    b = np.zeros(n, complex)
    k = u > 0
    np.add.at(H, (ia[k], ia[k]), u[k])
    np.add.at(H, (ib[k], ib[k]), u[k])
    np.add.at(H, (ib[k], ia[k]), -u[k])
    np.add.at(H, (ia[k], ib[k]), -u[k])
    np.add.at(b, ib[k], g[k])
    np.add.at(b, ia[k], -g[k])
    f = np.nonzero(info["free"])[0]
    Hff = H[np.ix_(f, f)]
    out = np.zeros(n, complex)
    out[f] = spl.spsolve(sp.csc_matrix(Hff), b[f]) if sp is not None else np.linalg.solve(Hff, b[f])
    return out


def compare_rounding(got, want, info, c, what):
    """poses of two evaluations of the same recurrence on the case c (info: its restatement), printed, then asserted within
    rounding_bounds(): the headings against each other, the positions against each other once the response of stage T to the
    heading difference is taken out.  Constant and degenerate poses carry no heading difference (nothing is degenerate here)."""
    b_th, b_xy = rounding_bounds(info)
    assert info["n_degenerate"] == 0
    d_th = np.abs(wrap(got[:, 2] - want[:, 2])).max()
    resp = _response(c, info, np.exp(1j * got[:, 2]) - np.exp(1j * want[:, 2]))
    dt = (got[:, 0] - want[:, 0]) + 1j * (got[:, 1] - want[:, 1])
    d_raw, d_xy = np.abs(dt).max(), np.abs(dt - resp).max()
    print("%s: same recurrence: heading difference %.3e (rounding bound %.3e); position difference %.3e m, %.3e m beside the response to the "
          "heading difference (rounding bound %.3e)" % (what, d_th, b_th, d_raw, d_xy, b_xy))
    assert d_th <= b_th, (what, d_th, b_th)
    assert d_xy <= b_xy, (what, d_xy, b_xy)


def from_truth(got, c):
    """(largest position error in metres, largest heading error in radians) of poses against the case's true poses"""
    P = c["poses"]
    return float(np.hypot(got[:, 0] - P[:, 0], got[:, 1] - P[:, 1]).max()), float(np.abs(wrap(got[:, 2] - P[:, 2])).max())


def compare(got, want, info, rtol, what, solves=1):
    """poses of an evaluation against the restatement's (or another evaluation's), printed, then asserted within bounds()"""
    b_th, b_xy = bounds(info, rtol, solves)
    d_th = np.abs(wrap(got[:, 2] - want[:, 2])).max()
    d_xy = np.hypot(got[:, 0] - want[:, 0], got[:, 1] - want[:, 1]).max()
    print("%s: heading difference %.3e (bound %.3e), position difference %.3e m (bound %.3e); lam_min R %.3e T %.3e, min |z| %.3e"
          % (what, d_th, b_th, d_xy, b_xy, info["R"]["lam_min"], info["T"]["lam_min"], info["min_mag"]))
    assert d_th <= b_th, (what, d_th, b_th)
    assert d_xy <= b_xy, (what, d_xy, b_xy)


# ---------------------------------------------------------------------------------------------------------------- the graphs
def fixture_case(n=None):
    """the 2000-pose fixture (or its sub-graph "poses < n") with its bogus loops at weight 0: a dict n, ia, ib, meas, kind, poses
    (the file's dead-reckoned poses), w, constant (None: pose 0)"""
    import os
    from conftest import GOLDEN
    N, ia, ib, meas, kind = SC.fixture(n)
    poses = np.load(os.path.join(GOLDEN, "synth_manhattan_2000_s7.npz"))["poses"][:N]
    return {"n": N, "ia": ia, "ib": ib, "meas": meas, "kind": kind, "poses": np.array(poses), "w": np.where(kind == 2, 0.0, 1.0), "constant": None}


def planted_case(n, variant="plain"):
    """_support_cases.planted(n) -- reversed chain edges, duplicates, a hub row of more than 64 slots -- with its wrong loops at
    weight 0 and
      plain      pose 0 constant
      const      pose n // 3 constant alone (poses: the truth moved rigidly, so that the constant is not at the origin)
      two        poses 2 and n - 5 constant
      weights    a fractional weight plane, an edge made inactive (weight 0), a zero-weight chain edge next to a loop that
                 keeps the graph connected"""
    c = SC.planted(n)
    E = len(c["ia"])
    w = np.ones(E)
    w[c["wrong"]] = 0.0
    w[c["dup"]] = 0.0
    P = c["P"].copy()
    constant = None
    if variant == "const":
        P = compose(np.array([3.0, -2.0, 0.7])[None, :], P)
        constant = np.zeros(n, bool)
        constant[n // 3] = True
    elif variant == "two":
        constant = np.zeros(n, bool)
        constant[[2, n - 5]] = True
    elif variant == "weights":
        rng = np.random.default_rng(n)
        w = np.where(w > 0, 0.25 + 0.75 * rng.random(E), 0.0)
        w[c["families"][1]] = 0.0          # "inactive"
        q = n // 8
        w[q + 1] = 0.0                     # the chain edge (q + 1, q + 2): its copy among the `odo` edges keeps the pair joined
    return {"n": n, "ia": c["ia"], "ib": c["ib"], "meas": c["meas"], "kind": c["kind"], "poses": P, "w": w, "constant": constant, "planted": c}


def exact_case(n=65, variant="plain"):
    """a noise-free graph whose start is NOT the answer: every edge of planted_case(n, variant) measured from the true poses,
    and in front of them a noisy odometry chain at weight 0 -- the chain edges, hence T and x0, are the noisy ones.  The
    `weights` variant keeps its plane (fractions and zeros); the others weigh every noise-free edge 1, the once wrong loops
    included.  The truth is the minimiser of both stages at cost 0, whatever the weights and the constant poses."""
    c = planted_case(n, variant)
    i = np.arange(n - 1, dtype=np.int32)
    noisy = relative(c["poses"][i], c["poses"][i + 1]) + np.random.default_rng(n).normal(0, 1, (n - 1, 3)) * np.array([0.05, 0.05, 0.02])
    c.update(ia=np.r_[i, c["ia"]].astype(np.int32), ib=np.r_[i + 1, c["ib"]].astype(np.int32),
             meas=np.vstack([noisy, relative(c["poses"][c["ia"]], c["poses"][c["ib"]])]), kind=np.r_[np.zeros(n - 1, np.uint8), c["kind"]],
             w=np.r_[np.zeros(n - 1), c["w"] if variant == "weights" else np.ones(len(c["ia"]))])
    return c


def degenerate_case(n=65):
    """two halves joined only by contradictory loops: the chain edge between them has weight 0, and the loops across come in
    pairs whose headings differ by pi, so that their pulls on the second half cancel and its z collapses"""
    c = planted_case(n)
    h = n // 2
    ia, ib, meas, w, P = c["ia"], c["ib"], c["meas"], c["w"], c["poses"]
    lo, hi = np.minimum(ia, ib), np.maximum(ia, ib)
    w = np.where((lo < h) & (hi >= h), 0.0, np.where(w > 0, 1.0, 0.0))   # nothing crosses ...
    add_a, add_b, add_m = [], [], []
    for k in range(3):                                                    # ... but these
        a, b = 3 + k, h + 4 + 2 * k
        m = relative(P[a][None, :], P[b][None, :])[0]
        for flip in (0.0, np.pi):
            add_a.append(a), add_b.append(b), add_m.append(m + np.array([0.0, 0.0, flip]))
    c.update(ia=np.r_[ia, add_a].astype(np.int32), ib=np.r_[ib, add_b].astype(np.int32), meas=np.vstack([meas, add_m]),
             kind=np.r_[c["kind"], np.full(len(add_a), 2, np.uint8)], w=np.r_[w, np.ones(len(add_a))], half=h)
    return c


def reject_case(n=257):
    """planted(n) with its wrong loops and the duplicate pair far beyond any threshold (tens of metres, radians) at the weight
    0.002, every other edge at weight 1: outvoted, so that the first solve stays near the truth and their residuals show"""
    c = planted_case(n)
    p = c["planted"]
    bad = np.r_[p["wrong"], p["dup"]]
    meas = c["meas"].copy()
    true = relative(c["poses"][c["ia"][bad]], c["poses"][c["ib"][bad]])
    meas[bad] = true + np.array([40.0, -30.0, 2.5])
    w = np.ones(len(c["ia"]))
    w[bad] = 0.002
    c.update(meas=meas, w=w, bad=np.sort(bad))
    return c


def plan_args(c):
    return (c["n"], c["ia"], c["ib"], c["meas"], c["poses"])


def graph_of(pgo, c):
    return pgo.Graph.from_arrays(c["poses"], c["ia"], c["ib"], c["meas"], c["kind"])
