"""pgo_gate_joint_evaluate (host): candidates decided one after the other on their joint covariance P, every accepted one
conditioning the rest (csrc/gate.h: gate_joint_decide, gate_pivot_row, gate_downdate -- what k_gate_joint_step runs on the
device), against the same elimination written in numpy.

Tolerance rule (none is fitted to the code under test): per case and per field, 8 x the largest difference between numpy's
float64 and numpy's longdouble elimination of the SAME input -- the reference's own rounding error, with a margin for another
summation order -- with a floor of 64 eps |P|_2.  The worst ratio is printed."""
import numpy as np
import pytest

from test_gate_host import EPS, draws, info6, spd

CHI2_95 = 7.814727903251179
FIELDS = ("r_cond", "P_cond", "chi2_cond", "info_gain_cond")


# ------------------------------------------------------------------------------------------- the reference elimination
def chol3(A):
    """lower Cholesky factor of a 3x3 matrix in A's own dtype (numpy.linalg has no longdouble)"""
    L = np.zeros((3, 3), A.dtype)
    for i in range(3):
        for j in range(i + 1):
            s = A[i, j] - L[i, :j] @ L[j, :j]
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    return L


def solve_lower(L, b):
    """L^-1 b, b of shape (3, m)"""
    x = np.zeros_like(b)
    for i in range(3):
        x[i] = (b[i] - L[i, :i] @ x[:i]) / L[i, i]
    return x


def accept(force, chi2, gain, chi2_gate, min_gain):
    return bool(force == 1) if force >= 0 else bool(chi2 <= chi2_gate and gain >= min_gain)


def eliminate(r, P, W, status=None, force=None, chi2_gate=CHI2_95, min_gain=0.0, dtype=np.float64):
    """the mathematics of include/pgo.h, "joint edge gate"; W: list of 3x3 information matrices"""
    n = len(W)
    M = np.array(P, dtype).copy()
    rho = np.array(r, dtype).reshape(-1).copy()
    out = {"r_cond": np.full((n, 3), np.nan, dtype), "P_cond": np.full((n, 3, 3), np.nan, dtype), "chi2_cond": np.full(n, np.nan, dtype),
           "info_gain_cond": np.full(n, np.nan, dtype), "accepted": np.zeros(n, np.int32)}
    eye = np.eye(3, dtype=dtype)
    for k in range(n):
        if status is not None and status[k]:
            continue
        s, lo = slice(3 * k, 3 * k + 3), 3 * k + 3
        Lw = chol3(np.array(W[k], dtype))
        C = chol3(eye + Lw.T @ M[s, s] @ Lw)
        y = solve_lower(C, (Lw.T @ rho[s])[:, None])[:, 0]
        out["r_cond"][k], out["P_cond"][k] = rho[s], M[s, s]
        out["chi2_cond"][k], out["info_gain_cond"][k] = y @ y, np.log(np.diag(C)).sum()
        out["accepted"][k] = accept(-1 if force is None else force[k], y @ y, out["info_gain_cond"][k], chi2_gate, min_gain)
        if out["accepted"][k] and lo < 3 * n:
            B = solve_lower(C, (M[lo:, s] @ Lw).T).T
            rho[lo:] -= B @ y
            M[lo:, lo:] -= B @ B.T
    return out


def problem(n, seed, frac_dup=0.0):
    """n correlated candidates: P = J Sigma J' from a random SPD Sigma over a few poses and two 3x3 blocks per row block of J;
    Omega in the ranges of test_gate_host.draws; r on the scale of (P_kk + Omega^-1)^(1/2), so that the default gate splits them"""
    rng = np.random.default_rng(seed)
    m = max(3, n // 2 + 2)
    A = rng.standard_normal((3 * m, 3 * m))
    Sigma = A @ A.T / (3 * m) * np.exp(rng.uniform(-4, 2)) + 1e-6 * np.eye(3 * m)
    J = np.zeros((3 * n, 3 * m))
    for k in range(n):
        a, b = rng.choice(m, 2, replace=False)
        J[3 * k:3 * k + 3, 3 * a:3 * a + 3] = rng.standard_normal((3, 3))
        J[3 * k:3 * k + 3, 3 * b:3 * b + 3] = rng.standard_normal((3, 3))
    P = J @ Sigma @ J.T
    P = 0.5 * (P + P.T)
    W = [spd(rng, 1e-2, 1e3) for _ in range(n)]
    r = np.zeros((n, 3))
    for k in range(n):
        S = P[3 * k:3 * k + 3, 3 * k:3 * k + 3] + np.linalg.inv(W[k])
        r[k] = np.linalg.cholesky(S) @ rng.standard_normal(3) * np.exp(rng.uniform(-1.0, 1.5))
    return r, P, W


def info_rows(W):
    return np.array([info6(w) for w in W])


def tolerances(ref64, refld, P):
    floor = 64 * EPS * np.linalg.norm(P, 2)
    return {f: max(8 * float(np.nanmax(np.abs(ref64[f].astype(np.longdouble) - refld[f]))), floor) for f in FIELDS}


def compare(got, ref64, tol, label):
    worst = 0.0
    for f in FIELDS:
        d = np.abs(got[f] - ref64[f])
        assert np.array_equal(np.isnan(got[f]), np.isnan(ref64[f])), (label, f)
        worst = max(worst, float(np.nanmax(d)) / tol[f]) if d.size and not np.isnan(d).all() else worst
        assert not (d > tol[f]).any(), (label, f, float(np.nanmax(d)), tol[f])
    print(f"{label}: worst |got - numpy| / tolerance = {worst:.3e}")
    return worst


def clear_of_the_gates(ref, chi2_gate, min_gain, force=None):
    """no decision of the reference lies within 1e-6 relative of a threshold"""
    for k in range(len(ref["chi2_cond"])):
        if np.isnan(ref["chi2_cond"][k]) or (force is not None and force[k] >= 0):
            continue
        assert abs(ref["chi2_cond"][k] - chi2_gate) > 1e-6 * chi2_gate, k
        assert abs(ref["info_gain_cond"][k] - min_gain) > 1e-6 * max(min_gain, 1e-300), k


# -------------------------------------------------------------------------------------------------- 1. against numpy
@pytest.mark.parametrize("n, seed", [(1, 101), (2, 102), (7, 103), (64, 104), (256, 105)])
def test_records_and_decisions_match_numpy(pgo, n, seed):
    r, P, W = problem(n, seed)
    rng = np.random.default_rng(seed + 1000)
    cases = [("default gate", None, CHI2_95, 0.0), ("gain threshold", None, 30.0, 0.5), ("random force", rng.integers(-1, 2, n), CHI2_95, 0.0)]
    n_acc = []
    for label, force, gate, gain in cases:
        ref64 = eliminate(r, P, W, None, force, gate, gain)
        refld = eliminate(r, P, W, None, force, gate, gain, np.longdouble)
        clear_of_the_gates(ref64, gate, gain, force)
        assert np.array_equal(ref64["accepted"], refld["accepted"])
        got = pgo.gate_joint_evaluate(r, P, info_rows(W), None, force, gate, gain)
        compare(got, ref64, tolerances(ref64, refld, P), f"n = {n}, {label}")
        assert np.array_equal(got["accepted"], ref64["accepted"]) and got["n_accepted"] == ref64["accepted"].sum()
        assert (got["status"] == 0).all()
        for k in range(n):
            assert np.array_equal(got["P_cond"][k], got["P_cond"][k].T)
        acc = got["accepted"] == 1
        assert got["chi2_joint"] == pytest.approx(got["chi2_cond"][acc].sum(), rel=n * EPS, abs=0)
        assert got["info_gain_joint"] == pytest.approx(got["info_gain_cond"][acc].sum(), rel=n * EPS, abs=1e-300)
        n_acc.append(int(acc.sum()))
    if n >= 7:
        assert 0 < n_acc[0] < n, n_acc   # the default gate does split these candidates


# -------------------------------------------------------------------------------------------------- 2. the chain rule
@pytest.mark.parametrize("n, seed", [(7, 203), (64, 204)])
def test_chain_rule(pgo, n, seed):
    """sum of chi2_cond over the accepted set A = r_A' (P_AA + Omega_A^-1)^-1 r_A, sum of info_gain_cond = 1/2 logdet(I + Omega_A P_AA).
    Tolerance 64 eps cond(S) relative, S = P_AA + Omega_A^-1 resp. I + Omega_A P_AA: the bound of a backward-stable dense solve
    / factorisation, the reference of this test (test_gate_host.py uses the same bound for the 3x3 case)."""
    r, P, W = problem(n, seed)
    got = pgo.gate_joint_evaluate(r, P, info_rows(W))
    A = np.nonzero(got["accepted"])[0]
    assert 1 < A.size < n
    rows = (3 * A[:, None] + np.arange(3)).reshape(-1)
    OmA = np.zeros((rows.size, rows.size))
    for j, a in enumerate(A):
        OmA[3 * j:3 * j + 3, 3 * j:3 * j + 3] = W[a]
    PAA, rA = P[np.ix_(rows, rows)], r[A].reshape(-1)
    S = PAA + np.linalg.inv(OmA)
    chi2 = rA @ np.linalg.solve(S, rA)
    T = np.eye(rows.size) + OmA @ PAA
    gain = 0.5 * np.linalg.slogdet(T)[1]
    print(f"n = {n}: chi2_joint {got['chi2_joint']:.12g} against {chi2:.12g}, info_gain_joint {got['info_gain_joint']:.12g} against {gain:.12g}")
    assert abs(got["chi2_joint"] - chi2) <= 64 * EPS * np.linalg.cond(S) * chi2
    assert abs(got["info_gain_joint"] - gain) <= 64 * EPS * np.linalg.cond(T) * max(1.0, gain)


# --------------------------------------------------------------------------------------------- 3. order invariance
@pytest.mark.parametrize("n, seed", [(7, 303), (64, 304)])
def test_order_invariance_with_every_candidate_forced_in(pgo, n, seed):
    r, P, W = problem(n, seed)
    rng = np.random.default_rng(seed + 1000)
    perms = [np.arange(n)] + [rng.permutation(n) for _ in range(5)]
    got, d = [], np.zeros(2)
    for p in perms:
        rows = (3 * p[:, None] + np.arange(3)).reshape(-1)
        rp, Pp, Wp = r[p], P[np.ix_(rows, rows)], [W[k] for k in p]
        force = np.ones(n, np.int8)
        g = pgo.gate_joint_evaluate(rp, Pp, info_rows(Wp), None, force, np.inf)
        assert g["n_accepted"] == n
        got.append((g["chi2_joint"], g["info_gain_joint"]))
        e64, eld = eliminate(rp, Pp, Wp, None, force), eliminate(rp, Pp, Wp, None, force, dtype=np.longdouble)
        for j, f in enumerate(("chi2_cond", "info_gain_cond")):
            d[j] = max(d[j], abs(float(e64[f].astype(np.longdouble).sum() - eld[f].sum())))
    floor = 64 * EPS * np.linalg.norm(P, 2)
    got = np.array(got)
    for j in range(2):
        spread = np.abs(got[:, j] - got[0, j]).max()
        tol = max(8 * d[j], floor)
        print(f"n = {n}: total {got[0, j]:.12g}, spread over 6 orders {spread:.3e}, tolerance {tol:.3e}")
        assert spread <= tol


# ------------------------------------------------------------------------------------------------- 4. special cases
def test_one_candidate_is_the_independent_gate(pgo):
    for r, P, W, _ in draws(20):
        g = pgo.gate_joint_evaluate(r, P, info6(W))
        chi2, cm, ig = pgo.gate_evaluate(r, P, info6(W))
        assert g["chi2_cond"][0] == cm and g["info_gain_cond"][0] == ig
        assert np.array_equal(g["r_cond"][0], r) and np.array_equal(g["P_cond"][0], P)
        assert g["accepted"][0] == int(cm <= CHI2_95 and ig >= 0.0)


def test_zero_rows(pgo):
    """a candidate between constant poses: P_cond = 0 and info_gain_cond = 0 exactly; accepted, it alters nothing"""
    r, P, W = problem(7, 401)
    P[9:12, :] = 0.0
    P[:, 9:12] = 0.0
    force = np.ones(7, np.int8)
    g = pgo.gate_joint_evaluate(r, P, info_rows(W), None, force)
    assert np.array_equal(g["P_cond"][3], np.zeros((3, 3))) and g["info_gain_cond"][3] == 0.0 and g["accepted"][3] == 1
    assert np.array_equal(g["r_cond"][3], r[3])
    assert abs(g["chi2_cond"][3] - r[3] @ W[3] @ r[3]) <= 16 * EPS * np.linalg.norm(W[3]) * (r[3] @ r[3])
    force[3] = 0
    g0 = pgo.gate_joint_evaluate(r, P, info_rows(W), None, force)
    for f in FIELDS:
        assert np.array_equal(g[f], g0[f]), f


def test_status_1_in_the_middle(pgo):
    r, P, W = problem(7, 402)
    P[9:12, :] = 0.0
    P[:, 9:12] = 0.0
    r[3] = np.nan
    status = np.array([0, 0, 0, 1, 0, 0, 0])
    force = np.ones(7, np.int8)
    g = pgo.gate_joint_evaluate(r, P, info_rows(W), status, force)
    for f in FIELDS:
        assert np.isnan(g[f][3]).all(), f
    assert g["accepted"].tolist() == [1, 1, 1, 0, 1, 1, 1] and g["status"].tolist() == status.tolist() and g["n_accepted"] == 6
    keep = np.array([0, 1, 2, 4, 5, 6])
    rows = (3 * keep[:, None] + np.arange(3)).reshape(-1)
    ref = pgo.gate_joint_evaluate(r[keep], P[np.ix_(rows, rows)], info_rows(W)[keep], None, force[keep])
    for f in FIELDS:
        assert np.array_equal(g[f][keep], ref[f]), f
    assert g["chi2_joint"] == ref["chi2_joint"] and g["info_gain_joint"] == ref["info_gain_joint"]


def test_identical_duplicate(pgo):
    """the same candidate twice: after the first is accepted the second sees rho' = rho - M S^-1 rho and M' = M - M S^-1 M with
    S = M + Omega^-1; its chi2_cond is rho'' (M' + Omega^-1)^-1 rho'.  Tolerance 64 eps cond relative, as in the chain rule."""
    rng = np.random.default_rng(403)
    M, W = spd(rng, 1e-3, 1e1), spd(rng, 1e-1, 1e2)
    rho = rng.standard_normal(3)
    P = np.block([[M, M], [M, M]])
    g = pgo.gate_joint_evaluate([rho, rho], P, [info6(W), info6(W)], None, [1, -1], np.inf)
    Wi = np.linalg.inv(W)
    S = M + Wi
    rho1, M1 = rho - M @ np.linalg.solve(S, rho), M - M @ np.linalg.solve(S, M)
    S1 = M1 + Wi
    chi2 = rho1 @ np.linalg.solve(S1, rho1)
    tol = 64 * EPS * max(np.linalg.cond(S), np.linalg.cond(S1))
    assert g["accepted"].tolist() == [1, 1]
    assert abs(g["chi2_cond"][1] - chi2) <= tol * chi2
    assert np.abs(g["P_cond"][1] - M1).max() <= tol * np.abs(M).max() and np.abs(g["r_cond"][1] - rho1).max() <= tol * np.abs(rho).max()
    assert g["info_gain_cond"][1] < g["info_gain_cond"][0]   # the second copy adds less than the first


# -------------------------------------------------------------------------------------------------------- 5. errors
def test_errors(pgo):
    r, P, W = problem(3, 501)
    w = info_rows(W)

    def status(*a, **k):
        with pytest.raises(pgo.PgoError) as e:
            pgo.gate_joint_evaluate(*a, **k)
        return e.value

    e = status(np.zeros((257, 3)), np.eye(771))
    assert e.status == -8 and "257" in str(e)
    assert status(r, P, w, None, [-1, 2, 0]).status == -1 and status(r, P, w, None, [-2, 0, 0]).status == -1
    bad = w.copy()
    bad[1] = [1.0, 2.0, 0, 1.0, 0, 1.0]
    assert status(r, P, bad).status == -1
    assert status(r, P, w, [0, 2, 0]).status == -1
    assert status(r, P, w, chi2_gate=np.nan).status == -1
    Q = P.copy()
    Q[3:6, 3:6] = np.diag([1.0, -3e3, 1.0])   # an indefinite block: the pivot of candidate 1 is not positive definite
    e = status(r, Q, None, None, [0, 1, 1])
    assert e.status == -7 and "candidate 1" in str(e)
    g = pgo.gate_joint_evaluate(np.zeros((0, 3)), np.zeros((0, 0)))   # n = 0
    assert g["n_accepted"] == 0 and g["chi2_joint"] == 0.0 and g["info_gain_joint"] == 0.0 and g["accepted"].size == 0
    assert pgo.GATE_JOINT_MAX == 256
    pgo.gate_joint_evaluate(np.zeros((256, 3)), np.eye(768))   # the cap itself is served
