"""numpy restatement of max-mixture edges (Olson & Agarwal, RSS 2012) as csrc/mixture.h states them and as pgo_mixture_solve
runs them, and the planted world the tests share: the reference of tests/test_mixture_host.py, tests/test_mixture_native.py and
tests/test_gpu_mixture.py.  A helper, not a test.

A mixture table is (edge [n], comp_ptr [n + 1], comps [n_comp, 5]) with the rows (x, y, theta, weight pi, info_scale w).  The
inner solves are tests/_loss_restatement.lm on the weighted oracle wrapper of tests/_gnc_restatement.py, with the oracle
graph's measurements rewritten to the selected means before every solve."""
import numpy as np

import _gnc_restatement as GR
import _loss_restatement as LR

TRIVIAL = [("trivial", 0.0)]
MAX_K = 8


def const(pi, w):
    """c_k = -log(pi_k) - 1.5 log(w_k)"""
    return -np.log(np.asarray(pi, np.float64)) - 1.5 * np.log(np.asarray(w, np.float64))


def q_of(comps, s, loss=("trivial", 0.0)):
    """q_k = w_k 1/2 rho(s_k) + c_k; NaN where s_k is not finite (whatever the loss)"""
    comps = np.asarray(comps, np.float64).reshape(-1, 5)
    s = np.asarray(s, np.float64)
    fin = np.isfinite(s)
    with np.errstate(all="ignore"):
        rho0 = LR.rho(loss[0], loss[1], np.where(fin, s, 0.0))[0]
        q = comps[:, 4] * (0.5 * rho0) + const(comps[:, 3], comps[:, 4])
    return np.where(fin, q, np.nan)


def pick(q):
    """(k*, q_best, margin) over the finite q, ties to the lowest index; (-1, nan, nan) without one; margin +inf with one"""
    q = np.asarray(q, np.float64)
    fin = np.isfinite(q)
    if not fin.any():
        return -1, np.nan, np.nan
    v = np.where(fin, q, np.inf)
    k = int(np.argmin(v))   # (the first of equal minima)
    rest = np.delete(v, k)
    second = rest.min() if len(rest) else np.inf
    return k, float(v[k]), float(second - v[k])


def component_s(O, og, poses, table):
    """s[j, k] = the plain |e|^2 of mixture edge j for its component k (NaN beyond its K)"""
    edge, ptr, comps = table
    n = len(edge)
    s = np.full((n, MAX_K), np.nan)
    K = np.diff(ptr)
    work = og.copy()
    for k in range(int(K.max()) if n else 0):
        has = K > k
        work.meas[:] = og.meas
        work.meas[edge[has]] = comps[ptr[:-1][has] + k, :3]
        s[has, k] = GR.plain_s(O, work, poses)[edge[has]]
    return s


def select(O, og, poses, table, losses=TRIVIAL, mix_class=None, prev=None, active=None):
    """the whole select: (chosen, q [n, 2], stats) as pgo_mixture_plan gives them"""
    edge, ptr, comps = table
    n = len(edge)
    s = component_s(O, og, poses, table)
    prev = -np.ones(n, np.int64) if prev is None else np.asarray(prev, np.int64)
    chosen, q = prev.copy(), np.full((n, 2), np.nan)
    st = dict(n_mix=n, n_changed=0, n_nonfinite=0, n_inactive=0, offset=0.0, mix_cost=0.0, count=[0] * MAX_K)
    for j in range(n):
        if active is not None and not active[j]:
            st["n_inactive"] += 1
            continue
        cj = comps[ptr[j]:ptr[j + 1]]
        k, qb, mg = pick(q_of(cj, s[j, :len(cj)], losses[int(mix_class[j]) if mix_class is not None else 0]))
        if k < 0:
            st["n_nonfinite"] += 1
            continue
        chosen[j], q[j] = k, (qb, mg)
        st["n_changed"] += int(k != prev[j])
        st["offset"] += float(const(cj[k, 3], cj[k, 4]))
        st["mix_cost"] += qb
        st["count"][k] += 1
    return chosen, q, st


class MixResult:
    pass


def solve(O, og, table, inner_iters=2, final_iters=50, max_rounds=50, poses=None):
    """the loop of pgo_mixture_solve, METHOD 0, Trivial loss on every edge, from og.poses (or `poses`)"""
    edge, ptr, comps = table
    E = og.n_edges
    cls = np.zeros(E, np.int64)
    x = np.array(og.poses if poses is None else poses, np.float64).reshape(-1, 3)
    work = og.copy()
    w = np.ones(E)
    sel = -np.ones(len(edge), np.int64)
    res = MixResult()
    res.rounds, res.hit_max_rounds, res.failed = [], False, False

    def lm(x0, iters):
        work.poses[:] = x0
        return LR.lm(GR.WeightedOracle(O, w), work, TRIVIAL, cls, method=0, max_iters=iters)

    def apply(chosen):
        rows = comps[ptr[:-1] + chosen]
        work.meas[edge] = rows[:, :3]
        w[edge] = rows[:, 4]

    for k in range(max_rounds):
        chosen, q, st = select(O, og, x, table, prev=sel)
        assert st["n_nonfinite"] == 0
        apply(chosen)
        sel = chosen
        cost = 0.5 * float((w * GR.plain_s(O, work, x)).sum())
        rec = dict(objective=cost + st["offset"], n_changed=st["n_changed"], count=st["count"], lm_iterations=0, lm_termination=0,
                   chosen=chosen.copy(), min_margin=float(np.nanmin(q[:, 1])), margin=q[:, 1].copy(), q_best=q[:, 0].copy())
        res.rounds.append(rec)
        if k > 0 and st["n_changed"] == 0:
            break
        r = lm(x, inner_iters)
        if r.termination == 6:
            res.failed = True
            break
        rec.update(lm_iterations=r.iterations, lm_termination=r.termination)
        x = r.poses
    else:
        res.hit_max_rounds = True
    fin = lm(x, final_iters)
    res.poses, res.final, res.selection, res.weights, res.meas = fin.poses, fin, sel, w.copy(), work.meas.copy()
    res.offset = st["offset"]
    res.objective = fin.final_cost + st["offset"]
    res.n_would_change = select(O, og, fin.poses, table, prev=sel)[2]["n_changed"]
    return res


# ---------------------------------------------------------------------------------------------------------- the planted world
# The null hypothesis: information 1e-4 I (a standard deviation 100 times the inlier's) and a relative weight that puts the
# crossover q_inlier = q_null at |e|^2 = 2 c / (1 - w) ~ 1.02, |e| ~ 1 m (c = -log 6e5 - 1.5 log 1e-4 = 0.511) -- between the
# 0.1 m the true closures of this graph stay below at the solution and the 2 m its bogus loops stay above
# (tests/test_gnc_host.py).  A relative weight above 1 is what the statement allows: the weights need not sum to 1.
PI_NULL, SCALE_NULL = 6e5, 1e-4
WRONG = np.array([3.0, -2.0, 1.2])   # what moves a bimodal closure's wrong mean away from the file's measurement
N_BIMODAL, N_SLIP = 60, 20


def planted(og, seed=11):
    """the mixture table on the 500-pose sub-graph (GR.subgraph(oracle, 500)) and who is who:
    every closure and every bogus loop: [inlier (1, 1), null (PI_NULL, SCALE_NULL)] at the file's measurement;
    N_BIMODAL of the closures: [the measurement moved by WRONG (1, 1), the file's measurement (1, 1), null];
    N_SLIP odometry edges: [the file's measurement (1, 1), no motion (1, 1)].
    Returns (table, roles): roles[j] in {"loop", "bogus", "bimodal", "slip"} per mixture edge."""
    kind = np.asarray(og.kind)
    rng = np.random.default_rng(seed)
    bim = set(rng.choice(np.nonzero(kind == 1)[0], N_BIMODAL, replace=False).tolist())
    slip = set(rng.choice(np.nonzero(kind == 0)[0], N_SLIP, replace=False).tolist())
    edge, ptr, comps, roles = [], [0], [], []
    for e in range(og.n_edges):
        m = og.meas[e]
        if e in slip:
            comps += [[*m, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0, 1.0]]
            roles.append("slip")
        elif e in bim:
            comps += [[*(m + WRONG), 1.0, 1.0], [*m, 1.0, 1.0], [*m, PI_NULL, SCALE_NULL]]
            roles.append("bimodal")
        elif kind[e] != 0:
            comps += [[*m, 1.0, 1.0], [*m, PI_NULL, SCALE_NULL]]
            roles.append("bogus" if kind[e] == 2 else "loop")
        else:
            continue
        edge.append(e)
        ptr.append(len(comps))
    return (np.array(edge, np.int32), np.array(ptr, np.int32), np.array(comps, np.float64)), np.array(roles)


def summation_bound(n_edges, F):
    """F is a sum of n_edges + n_mix <= 2 n_edges terms of one sign pattern: two evaluations of it in different orders differ by
    at most ~ n eps F.  n_edges * 2.2e-16 * F is what the issue states for 'non-increasing up to rounding'."""
    return n_edges * 2.2e-16 * abs(F)


# ---------------------------------------------------------------------------------------------------------- select cases
def cycling_table(og, edges, seed):
    """K cycles 1..8 over `edges`; component means scattered around the file's measurement, pi in (0, 1], w in (0, 1]"""
    rng = np.random.default_rng(seed)
    edge, ptr, comps = np.asarray(edges, np.int32), [0], []
    for i, e in enumerate(edge):
        K = 1 + i % MAX_K
        for _ in range(K):
            m = og.meas[e] + rng.normal(0.0, [0.6, 0.6, 0.3])
            comps.append([*m, 10.0 ** rng.uniform(-2.0, 0.0), 10.0 ** rng.uniform(-1.0, 0.0)])
        ptr.append(len(comps))
    return edge, np.array(ptr, np.int32), np.array(comps, np.float64)


def perturbed(og, seed, sigma=0.3):
    rng = np.random.default_rng(seed)
    return np.asarray(og.poses, np.float64) + rng.normal(0.0, [sigma, sigma, 0.5 * sigma], (og.n_poses, 3))


# ---------------------------------------------------------------------------------------------------------- statement cases
LOSSES = [("trivial", 0.0), ("huber", 0.5), ("softlone", 0.7), ("cauchy", 1.0), ("arctan", 2.0), ("tukey", 1.5)]


def eval_cases(seed=5):
    """(comps [K, 5], s [K], loss) for K = 1..8 under every loss, then the edges of the statement: exact ties (two identical
    components: the lower index), a non-finite s among finite ones (each kind, each position), all components non-finite, and
    pi and w across twelve decades"""
    rng = np.random.default_rng(seed)
    cases = []

    def comps_of(K):
        c = np.zeros((K, 5))
        c[:, :3] = rng.normal(0.0, 1.0, (K, 3))
        c[:, 3] = 10.0 ** rng.uniform(-3.0, 3.0, K)
        c[:, 4] = 10.0 ** rng.uniform(-4.0, 0.0, K)
        return c

    for loss in LOSSES:
        for K in range(1, MAX_K + 1):
            for _ in range(3):
                cases.append((comps_of(K), 10.0 ** rng.uniform(-4.0, 3.0, K), loss))
    for loss in LOSSES:
        for K in range(2, MAX_K + 1):
            c, s = comps_of(K), 10.0 ** rng.uniform(-2.0, 1.0, K)
            i, j = sorted(rng.choice(K, 2, replace=False).tolist())
            c[j], s[j] = c[i], s[i]           # identical twins ...
            c[i, 3:] = c[j, 3:] = (1e6, 1.0)  # ... that win: q = 1/2 rho(1e-3) - 13.8, every other c_k >= -log 1e3 = -6.9
            s[i] = s[j] = 1e-3
            cases.append((c, s, loss))
            for bad in (np.nan, np.inf, -np.inf):
                c, s = comps_of(K), 10.0 ** rng.uniform(-2.0, 1.0, K)
                s[rng.integers(K)] = bad
                cases.append((c, s, loss))
            cases.append((comps_of(K), np.full(K, np.nan), loss))
            cases.append((comps_of(K), np.array([np.nan, np.inf] * 4)[:K], loss))
        cases.append((comps_of(1), np.array([np.inf]), loss))
    for d in range(-12, 13, 2):               # pi from 1e-12 to 1e12, w from 1e-12 to 1
        c = comps_of(3)
        c[:, 3] = [10.0 ** d, 1.0, 10.0 ** -d]
        c[:, 4] = [10.0 ** (-abs(d)), 1.0, 10.0 ** (-abs(d) / 2.0)]
        cases.append((c, np.array([0.3, 7.0, 40.0]), ("trivial", 0.0)))
    return cases


# ---------------------------------------------------------------------------------------------------------- device select cases
SELECT_SIZES = (1, 255, 256, 257, 956)   # less than a chunk, one short of / exactly / one past a chunk, every loop edge (ragged)
SELECT_SEED = 3                          # (chosen on the CPU: tests/test_mixture_host.py checks what it must give)
MARGIN_REL = 1e-9                        # `chosen` is compared where the plan's margin exceeds MARGIN_REL (1 + |q_best|)
S_FLOOR = 0.05 ** 2                      # every component's s in the select cases is above this (see q_tolerance)


def select_case(og, n):
    """the table over the first n non-odometry edges (K cycling 1..8) and the perturbed poses of the device select tests"""
    loops = np.nonzero(np.asarray(og.kind) != 0)[0]
    assert n <= len(loops)
    return cycling_table(og, loops[:n], SELECT_SEED + n), perturbed(og, SELECT_SEED)


def decided(q):
    """the edges whose selection two correct evaluations must agree on"""
    return q[:, 1] > MARGIN_REL * (1.0 + np.abs(q[:, 0]))


# Two correct evaluations of s = |e|^2 differ by the roundings of e: each component of e is a difference of quantities of
# magnitude up to D + |m| ~ 40 m (this graph's extent) formed with a handful of roundings, so |de| <~ 8 eps 40 m = 7e-14 m and
# ds / s <= 2 |de| / |e| <= 2 * 7e-14 / 0.05 = 2.9e-12 at the floor |e| >= 0.05 m, 3e-13 at the typical |e| ~ 0.5 m.  q adds one
# product and one sum of positive terms (pi <= 1 and w <= 1 here: c >= 0).  The issue's 1e-12 is asserted as it stands.
Q_REL = 1e-12
