"""The direct chain + low-rank linear solve (csrc/direct.hip.h, solver_direct.hip) as an OPERATOR: y = (H + D'D)^-1 b for
arbitrary b through pgo_debug_direct_solve -- the launch sequence an LM iteration runs -- with and without its
iterative-refinement step, at the sizes where direct_setup() and the kernels change behaviour, against the numpy
restatement of the same algorithm (_direct_restatement.restate) on the oracle's system (oracle.lm_system).

A handle is advanced with lm_begin / lm_step(1) to the state after its first ACCEPTED step and, where the first 12
iterations have one, after a REJECTED step.  Per state and right-hand side (the system's own b, two Gaussian vectors, unit
vectors at the chain's ends, next to the constant pose, at and around the separators, at the ends of sweep segments and at
the first loop's endpoints), for refine = 0 (the raw Woodbury result), -1 (what LM runs) and, on three cases, 2; infinity
norms, residuals accumulated in numpy.longdouble:
  (a) refined: eta = |b - A y| / (|A| |y| + |b|) <= 1e-10 against the ORACLE's A (BE_ONE of test_gpu_precond.py: the GPU's H
      agrees with the oracle's to ~1e-11, nothing tighter can be asked of a quantity that mixes the two); METHOD 2's A is the
      reduced pose system of the joint LM system over poses and switches (_switch_restatement.joint_system);
  (b) all methods: eta_self, the same quotient with A y from the handle's own product (system_spmv),
      <= RATIO x max(eta_restate, floor): eta_restate the restatement's backward error for the same right-hand side and
      refine count, floor = 4 x (most nonzeros in a row of A) x 2^-53, the rounding of one row of the residual product.
      RATIO = 10: both sides run the same recurrences in fp64 and differ in summation order, a cofactor 3x3 inverse against
      LAPACK's, an explicit inverse factor against triangular solves; a structural mistake leaves the raw eta at 1e-6 .. 1;
  (c) refinement never makes things worse: eta_self(-1) <= max(eta_self(0), 10 floor);
  (d) y is exactly 0.0 on the constant pose, a second call returns bitwise the same y, and a twin handle stepped without
      any of these calls takes bitwise the same trajectory.
Every case asserts through pgo_handle_info (direct_rank, direct_separators, direct_segments, direct_refine_kernel) that it
reached the path its id names.  The case table is also run on the CPU (test_direct_restatement.py): the restatement alone
must solve every case with N <= 5000.

Measured on an MI355X (all 57 cases pass): largest eta_self / max(eta_restate, floor) per refine count --
  refine  0: 3.15 (N300-K96-nb3, rejected state, e74.2: eta_self 2.8e-14 at a floor of 2.0e-14); next 2.32 (N40-fixed-last-m2),
             2.14 (N512-m21-piece128), 1.95 (N257-m300), 1.25 (N40-K66-nb3); every other case below 1;
  refine -1: 0.04 (N2-m1-duplicate-pair; the refined result sits one to two orders below the floor everywhere);
  refine  2: 0.01.
Largest eta against the oracle's matrix: raw 7.6e-12 (N2049-m43-radius1e12), refined 2.4e-14 (N18000-m10-separators15); the four
METHOD 2 cases against the restated reduced system: raw 7.6e-15 (N40-fixed-last-m2), refined 1.6e-15."""
import os
import time

import numpy as np
import pytest

from _direct_restatement import backward_error, norm_inf, restate, rounding_floor, system_matrix
from _switch_restatement import joint_system
from conftest import DATA

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
BE_ONE = 1e-10     # criterion (a)
RATIO = 10.0       # criterion (b)


class ArrayGraph:
    """a graph as plain arrays (what chain_graph builds and _direct_restatement reads)"""
    def __init__(self, poses, ia, ib, meas, kind):
        self.poses, self.meas = np.ascontiguousarray(poses, np.float64), np.ascontiguousarray(meas, np.float64)
        self.ia, self.ib = np.ascontiguousarray(ia, np.int32), np.ascontiguousarray(ib, np.int32)
        self.kind = np.ascontiguousarray(kind, np.uint8)

    n_poses = property(lambda self: len(self.poses))
    n_edges = property(lambda self: len(self.ia))

    def to_pgo(self, pgo):
        return pgo.Graph.from_arrays(self.poses, self.ia, self.ib, self.meas, self.kind)

    def to_oracle(self, O):
        E = self.n_edges
        info = np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]), (E, 1))
        return O.Graph(np.arange(self.n_poses, dtype=np.int32), self.poses.copy(), self.ia.copy(), self.ib.copy(),
                       self.meas.copy(), info, self.kind.copy())


def chain_graph(n, loops, seed, fixed=0):
    """A Manhattan-like walk of unit steps (a quarter turn at every fifth pose or so): odometry edges i -> i+1 with noise
    (0.02, 0.02, 0.01), the loop edges `loops` (pairs a, b: measured a -> b from the true walk, same noise), initial poses =
    the integrated noisy odometry plus pose noise (0.05, 0.05, 0.02) on every pose but the constant one -- without the second
    noise a graph without loops starts at zero residual and LM stops before any state exists to test."""
    rng = np.random.default_rng(seed)
    turn = rng.choice([-1, 0, 0, 0, 1], n)
    turn[0] = 0
    th = np.cumsum(turn) * (np.pi / 2)
    xy = np.zeros((n, 2))
    xy[1:] = np.cumsum(np.column_stack([np.cos(th[:-1]), np.sin(th[:-1])]), axis=0)
    ia = np.concatenate([np.arange(n - 1), np.array([a for a, _ in loops], np.int64)]).astype(np.int32)
    ib = np.concatenate([np.arange(1, n), np.array([b for _, b in loops], np.int64)]).astype(np.int32)
    kind = np.concatenate([np.zeros(n - 1, np.uint8), np.ones(len(loops), np.uint8)])
    d = xy[ib] - xy[ia]
    c, s = np.cos(th[ia]), np.sin(th[ia])
    meas = np.column_stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], th[ib] - th[ia]])
    meas += rng.standard_normal(meas.shape) * np.array([0.02, 0.02, 0.01])
    odo = meas[:n - 1]
    th0 = np.concatenate([[0.0], np.cumsum(odo[:, 2])])
    c, s = np.cos(th0[:-1]), np.sin(th0[:-1])
    xy0 = np.zeros((n, 2))
    xy0[1:] = np.cumsum(np.column_stack([c * odo[:, 0] - s * odo[:, 1], s * odo[:, 0] + c * odo[:, 1]]), axis=0)
    poses = np.column_stack([xy0, th0])
    noise = rng.standard_normal((n, 3)) * np.array([0.05, 0.05, 0.02])
    if fixed >= 0:
        noise[fixed] = 0.0
    return ArrayGraph(poses + noise, ia, ib, meas, kind)


def rand_loops(n, m, seed=3, span=60):
    """m loop pairs of at least 2 and at most `span` poses apart (short: the drift of the integrated odometry stays small and
    the first LM steps are accepted), about a third of them given as (b, a)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(m):
        a = int(rng.integers(0, n - 2))
        b = min(n - 1, a + int(rng.integers(2, max(3, min(span, n - 1) + 1))))
        out.append((b, a) if rng.uniform() < 0.3 else (a, b))
    return out


def layout(n):
    """direct_setup()'s choices for a chain of n poses: separators, sweep segments, refinement kernel"""
    nsep = 0 if n < 256 else min(15, max(3, n // 1200))
    sep = [((j + 1) * n) // (nsep + 1) for j in range(nsep)]
    seglen = max(1, -(-n // 32))
    return sep, -(-n // seglen), seglen, (1 if n <= 4096 else 2)


def _case(n, loops, fixed=0, opts=None, expect=None, states="both", refines=(0, -1), rhs="all", seed=5, dataset=None):
    return dict(n=n, loops=loops, fixed=fixed, opts=dict(opts or {}), expect=dict(expect or {}), states=states, refines=refines,
                rhs=rhs, seed=seed, dataset=dataset)


def _sep_loops(n):
    """endpoints ON a separator pose, on its two neighbours, on pose 0, on pose n-1; a loop that duplicates a chain pair in
    either orientation; the same loop twice"""
    sep = layout(n)[0]
    s0, s1, s2 = sep[0], sep[len(sep) // 2], sep[-1]
    return [(s0, s0 + 40), (s0 - 1, s0 - 30), (s0 + 1, s0 + 35), (s1 - 20, s1), (s1 + 1, s1 - 1), (s2, s2 - 45), (s2 - 1, s2 + 1),
            (0, 40), (n - 41, n - 1), (0, s0), (10, 11), (21, 20), (5, 50), (5, 50)]


SEP1200 = dict(direct_separators=3, direct_segments=32, direct_refine_kernel=1)
CASES = {
    # --- fewer poses than the 32 sweep segments: dl_seglen = ceil(N / 32)
    "N2-m0-segments2": _case(2, [], expect=dict(direct_separators=0, direct_segments=2, direct_refine_kernel=1)),
    "N2-m1-duplicate-pair": _case(2, [(1, 0)], expect=dict(direct_separators=0, direct_segments=2)),
    "N3-m1-segments3": _case(3, [(0, 2)], expect=dict(direct_separators=0, direct_segments=3)),
    "N31-m5-segments31": _case(31, rand_loops(31, 5), expect=dict(direct_separators=0, direct_segments=31)),
    "N32-m5-segments32": _case(32, rand_loops(32, 5), expect=dict(direct_separators=0, direct_segments=32)),
    "N33-m11-seglen2-segments17": _case(33, rand_loops(33, 11), expect=dict(direct_separators=0, direct_segments=17)),
    # --- separators switch on at 256 poses
    "N255-m21-no-separators": _case(255, rand_loops(255, 21), expect=dict(direct_separators=0, direct_segments=32)),
    "N256-m21-separators3": _case(256, rand_loops(256, 21), expect=dict(direct_separators=3, direct_segments=32)),
    "N257-m21-separators3": _case(257, rand_loops(257, 21), expect=dict(direct_separators=3, direct_segments=29), refines=(0, -1, 2)),
    "N257-m21-radius1e12": _case(257, rand_loops(257, 21), opts=dict(radius0=1e12), expect=dict(direct_separators=3)),
    "N257-m300": _case(257, rand_loops(257, 300), expect=dict(direct_separators=3)),
    # --- factor chunk of 128 poses per piece (k_dlr_factor CH): pieces of 128 / 129
    "N512-m21-piece128": _case(512, rand_loops(512, 21), expect=dict(direct_separators=3, direct_segments=32)),
    "N516-m21-piece129": _case(516, rand_loops(516, 21), expect=dict(direct_separators=3, direct_segments=31)),
    # --- sweep chunk of 64 poses (k_dlr_fwd / _mid / _fix CH): seglen 64 / 65
    "N2048-m43-seglen64": _case(2048, rand_loops(2048, 43), expect=dict(direct_separators=3, direct_segments=32, direct_refine_kernel=1)),
    "N2049-m43-seglen65": _case(2049, rand_loops(2049, 43), expect=dict(direct_separators=3, direct_segments=32, direct_refine_kernel=1)),
    "N2049-m43-radius1e12": _case(2049, rand_loops(2049, 43), opts=dict(radius0=1e12), expect=dict(direct_separators=3)),
    # --- ragged fine segments of k_dlr_solve1: dl_seglen2 = ceil(N / 256) leaves fewer than 256 of them
    "N4000-m10-solve1-250-segments": _case(4000, rand_loops(4000, 10), expect=dict(direct_separators=3, direct_refine_kernel=1)),
    # --- refinement column: k_dlr_solve1 up to 4096 poses, the batched kernels above
    "N4096-m10-k_dlr_solve1": _case(4096, rand_loops(4096, 10), expect=dict(direct_separators=3, direct_segments=32, direct_refine_kernel=1)),
    "N4097-m10-batched-refine": _case(4097, rand_loops(4097, 10), expect=dict(direct_separators=3, direct_segments=32, direct_refine_kernel=2),
                                      refines=(0, -1, 2)),
    "N4097-m10-radius1e12": _case(4097, rand_loops(4097, 10), opts=dict(radius0=1e12), expect=dict(direct_refine_kernel=2)),
    # --- a 4th separator, and the cap of 15
    "N4799-m10-separators3": _case(4799, rand_loops(4799, 10), expect=dict(direct_separators=3, direct_refine_kernel=2)),
    "N4800-m10-separators4": _case(4800, _sep_loops(4800)[:10], expect=dict(direct_separators=4, direct_refine_kernel=2)),
    "N4800-m10-fixed-half": _case(4800, _sep_loops(4800)[:10], fixed=2400, expect=dict(direct_separators=4)),
    "N17999-m10-separators14": _case(17999, _sep_loops(17999)[:10], expect=dict(direct_separators=14, direct_segments=32), states="accepted"),
    "N18000-m10-separators15": _case(18000, _sep_loops(18000)[:10], expect=dict(direct_separators=15, direct_segments=32), states="accepted"),
    "N19201-m10-separators-capped15": _case(19201, _sep_loops(19201)[:10], expect=dict(direct_separators=15, direct_segments=32), states="accepted"),
    # --- the largest graph
    "N65536-m10-largest": _case(65536, _sep_loops(65536)[:10], expect=dict(direct_separators=15, direct_segments=32, direct_refine_kernel=2),
                                states="accepted"),
    # --- loop endpoints on and around separators, pose 0, pose N-1, the constant pose; duplicates of chain pairs and of loops
    "N1200-sep-loops-m1": _case(1200, _sep_loops(1200), opts=dict(method=1), expect=dict(SEP1200)),
    "N1200-sep-loops-m0": _case(1200, _sep_loops(1200), opts=dict(method=0), expect=dict(SEP1200)),
    "N1200-sep-loops-m2": _case(1200, _sep_loops(1200), opts=dict(method=2), expect=dict(SEP1200)),
    "N400-hub200": _case(400, [(77, j) if j % 3 else (j, 77) for j in range(100, 300)], expect=dict(direct_separators=3)),
    # --- the constant pose: last, middle (= the middle separator when there are three), a separator, next to one
    "N1200-fixed-last": _case(1200, _sep_loops(1200) + [(1199, 1150)], fixed=1199, expect=dict(SEP1200)),
    "N1200-fixed-separator300": _case(1200, _sep_loops(1200) + [(300, 340)], fixed=300, expect=dict(SEP1200)),
    "N1200-fixed-half-separator600": _case(1200, _sep_loops(1200), fixed=600, expect=dict(SEP1200)),
    "N1200-fixed-301-after-separator": _case(1200, _sep_loops(1200), fixed=301, expect=dict(SEP1200)),
    "N40-fixed-last-m2": _case(40, rand_loops(40, 11), fixed=39, opts=dict(method=2), expect=dict(direct_separators=0)),
    # --- METHOD 0 / 2 on the K sweep's chain
    "N300-m22-method0": _case(300, rand_loops(300, 22), opts=dict(method=0), expect=dict(direct_separators=3)),
    "N300-m22-method2": _case(300, rand_loops(300, 22), opts=dict(method=2), expect=dict(direct_separators=3)),
    # --- the largest rank: K = 6141, nb = 192 (one state, one refine setting, b + 2 random right-hand sides)
    "N300-m2047-largest-rank": _case(300, rand_loops(300, 2047), expect=dict(direct_separators=3), states="accepted", refines=(-1,), rhs="few"),
    # --- anchors to the dataset tests
    "INTEL50-m1": _case(0, None, dataset=("INTEL", 50), opts=dict(method=1), expect=dict(direct_rank=918, direct_separators=3), refines=(0, -1, 2)),
    "INTEL50-m2": _case(0, None, dataset=("INTEL", 50), opts=dict(method=2), expect=dict(direct_rank=918, direct_separators=3)),
    # (FRH forced, K = 4515, is not here: at radius 1e12 the restatement itself does not solve FRH's first system -- eta_restate
    # 1.3e-2 after one refinement step -- so it is no baseline there; test_gpu_parity.py keeps FRH's trajectory test)
}
# --- Cholesky blocks of 32 (CHOL_NB), grid max(1, nb - 1): K = 0, 3, 30, 33, 63, 66, 96, 129 -> nb = 1, 1, 1, 2, 2, 3, 3, 5; on a
# chain without separators and on one with (the chain part is the same across each sweep: a failure names the dense path)
for _n in (40, 300):
    for _m in (0, 1, 10, 11, 21, 22, 32, 43):
        CASES["N%d-K%d-nb%d" % (_n, 3 * _m, max(32, -(-3 * _m // 32) * 32) // 32)] = _case(
            _n, rand_loops(_n, _m, seed=9), expect=dict(direct_separators=3 if _n >= 256 else 0))
REFUSED = {
    "N65537-m0-too-many-poses": (65537, 0),
    "N300-m2048-rank-too-large": (300, 2048),
}


def build_case(case, O):
    """(ArrayGraph, oracle graph) of a case"""
    c = CASES[case]
    if c["dataset"]:
        name, n_out = c["dataset"]
        og = O.read_g2o(os.path.join(DATA, name + ".g2o"))
        if n_out:
            og = O.add_random_C(og, n_out, 1)
        return ArrayGraph(og.poses, og.ia, og.ib, og.meas, og.kind), og
    ag = chain_graph(c["n"], c["loops"], c["seed"], c["fixed"])
    return ag, ag.to_oracle(O)


def unit_poses(n, fixed, loops_first):
    sep, nseg, seglen, _ = layout(n)
    if len(sep) > 3:
        sep = [sep[0], sep[len(sep) // 2], sep[-1]]
    want = [0, 1, n - 2, n - 1, fixed - 1, fixed + 1]
    for s in sep:
        want += [s - 1, s, s + 1]
    for q in (0, 1, nseg - 1):
        want += [q * seglen, min(n, (q + 1) * seglen) - 1]
    want += list(loops_first)
    return sorted({i for i in want if 0 <= i < n and i != fixed})


def right_hand_sides(sysm, n, fixed, loops_first, few, rng):
    cols = [np.array(sysm.b, np.float64), rng.standard_normal(3 * n), rng.standard_normal(3 * n)]
    names = ["b", "gauss0", "gauss1"]
    if not few:
        for i in unit_poses(n, fixed, loops_first):
            for c in (0, 2):
                e = np.zeros(3 * n)
                e[3 * i + c] = 1.0
                cols.append(e)
                names.append("e%d.%d" % (i, c))
    B = np.column_stack(cols)
    if fixed >= 0:
        B[3 * fixed:3 * fixed + 3] = 0.0
    keep = [k for k in range(B.shape[1]) if B[:, k].any()]     # (a zero right-hand side: eta is 0 / 0)
    return B[:, keep], [names[k] for k in keep]


def check_state(O, s, ag, og, c, label, summary):
    rec = s.iter_records()[-1]
    method, fixed, n = c["opts"].get("method", 1), c["fixed"], ag.n_poses
    if method == 2:
        # the reduced pose system of the joint LM system over poses and switches (_switch_restatement.py); after a rejected
        # step the handle keeps the elimination of the previous radius under the LM diagonal of the current one
        recs, g, o = s.iter_records(), s.graph, s.options
        # (pgo.Graph.from_arrays regroups edges by kind and switches() answers in the graph's order: it must be the oracle graph's)
        assert np.array_equal(g.ia, og.ia) and np.array_equal(g.ib, og.ib) and np.array_equal(g.kind, og.kind), label
        sysm = joint_system(O, og, s.poses(), s.switches(), ag.poses, rec["radius"], o.sc_prior_lambda, fixed,
                            jacobi_scaling=o.jacobi_scaling, radius_elim=recs[-2]["radius"] if rec["step_ok"] != 1 else None,
                            min_diag=o.min_lm_diagonal, max_diag=o.max_lm_diagonal, delta=o.huber_delta, threads=THREADS).sysm
    else:
        sysm = O.lm_system(og, s.poses(), ag.poses, rec["radius"], method=method, fixed_pose=fixed, threads=THREADS)
    A = system_matrix(sysm)
    a_norm, floor = norm_inf(A), rounding_floor(A)
    first = (int(ag.ia[n - 1]), int(ag.ib[n - 1])) if ag.n_edges > n - 1 and not c["dataset"] else ()
    B, names = right_hand_sides(sysm, n, fixed, first, c["rhs"] == "few", np.random.default_rng(7))
    steps_of = {rf: (1 if rf < 0 else rf) for rf in c["refines"]}      # (-1: the handle's own setting, dl_refine = 1)
    by_steps = restate(sysm, og, fixed, B, tuple(sorted(set(steps_of.values()))))
    refs = {rf: by_steps[k] for rf, k in steps_of.items()}
    self_err = {}
    for rf in c["refines"]:
        worst = dict(ratio=0.0, eta_self=0.0, eta=0.0, eta_restate=0.0, at="")
        for k, name in enumerate(names):
            b = np.ascontiguousarray(B[:, k])
            y = s.direct_solve(b, rf)
            assert np.isfinite(y).all(), (label, rf, name)
            if fixed >= 0:
                assert not y[3 * fixed:3 * fixed + 3].any(), (label, rf, name, y[3 * fixed:3 * fixed + 3])
            if k < 3:
                np.testing.assert_array_equal(s.direct_solve(b, rf), y)                       # (d) fixed order
            e_self = backward_error(A, y, b, Ay=s.system_spmv(y), a_norm=a_norm)
            e_ref = backward_error(A, refs[rf][:, k], b)
            ratio = e_self / max(e_ref, floor)
            self_err[(rf, k)] = e_self
            e_orc = backward_error(A, y, b)
            if ratio > worst["ratio"]:
                worst.update(ratio=ratio, at=name)
            worst["eta_self"], worst["eta"] = max(worst["eta_self"], e_self), max(worst["eta"], e_orc)
            worst["eta_restate"] = max(worst["eta_restate"], e_ref)
            if rf != 0:
                assert e_orc <= BE_ONE, (label, rf, name, e_orc)                               # (a)
            assert ratio <= RATIO, (label, rf, name, e_self, e_ref, floor)                    # (b)
            if rf == -1 and (0, k) in self_err:
                assert e_self <= max(self_err[(0, k)], 10.0 * floor), (label, name, e_self, self_err[(0, k)])   # (c)
        print("%s LM iteration %d radius %.1e refine %2d: %d right-hand sides, eta_self / max(eta_restate, floor) %.2f (at %s), "
              "eta_self %.1e eta %.1e eta_restate %.1e floor %.1e" % (label, rec["iter"], rec["radius"], rf, len(names), worst["ratio"],
                                                                     worst["at"], worst["eta_self"], worst["eta"], worst["eta_restate"], floor))
        summary[rf] = max(summary.get(rf, 0.0), worst["ratio"])


def strip(recs):
    return [{k: v for k, v in r.items() if k != "seconds"} for r in recs]


@pytest.mark.parametrize("case", list(CASES))
def test_direct_solve_matches_the_restatement(pgo, oracle, case):
    c = CASES[case]
    t0 = time.perf_counter()
    ag, og = build_case(case, oracle)
    g = ag.to_pgo(pgo)
    opts = dict(max_iters=12, linear_solver=2, fixed_pose=c["fixed"], **c["opts"])
    s, ref = pgo.Solver(g, pgo.Options(**opts)), pgo.Solver(g, pgo.Options(**opts))
    info = s.info()
    sep, nseg, _, kernel = layout(ag.n_poses)
    expect = dict(linear_solver=2, direct_separators=len(sep), direct_segments=nseg, direct_refine_kernel=kernel)
    if not c["dataset"]:
        expect["direct_rank"] = 3 * len(c["loops"])
    expect.update(c["expect"])
    for k, v in expect.items():
        assert getattr(info, k) == v, (case, k, getattr(info, k), v)
    s.lm_begin()
    seen, steps, summary = set(), 0, {}
    want = {1} if c["states"] == "accepted" else {1, 0}
    while steps < 12 and not want <= seen:
        done, _ = s.lm_step(1)
        steps += 1
        ok = s.iter_records()[-1]["step_ok"]
        if ok in want and ok not in seen:
            seen.add(ok)
            check_state(oracle, s, ag, og, c, "%s %s" % (case, "accepted" if ok else "rejected"), summary)
        if done:
            break
    assert 1 in seen, (case, [r["step_ok"] for r in s.iter_records()])
    assert s.info().direct_fallbacks == 0, case
    # no side effects: a second handle stepped without the calls takes the same trajectory, bitwise
    ref.lm_begin()
    for _ in range(steps):
        ref.lm_step(1)
    np.testing.assert_array_equal(s.poses(), ref.poses())
    assert strip(s.iter_records()) == strip(ref.iter_records())
    print("%s: steps %d, states %s, largest ratio per refine count %s, %.1f s" % (
        case, steps, sorted(seen), {k: round(v, 2) for k, v in summary.items()}, time.perf_counter() - t0))
    s.close()
    ref.close()


@pytest.mark.parametrize("case", list(REFUSED))
def test_direct_solve_refuses_beyond_its_limits(pgo, case):
    """DIRECT_MAX_POSES = 65536 and DIRECT_MAX_RANK = 6144 (3 m + 1): one more is PGO_ERR_UNSUPPORTED, not a wrong answer"""
    n, m = REFUSED[case]
    g = chain_graph(n, rand_loops(n, m), 5).to_pgo(pgo)
    with pytest.raises(pgo.PgoError) as e:
        pgo.Solver(g, pgo.Options(linear_solver=2))
    assert e.value.status == -8, str(e.value)


def test_direct_solve_entry_point_arguments(pgo):
    ag = chain_graph(40, rand_loops(40, 5), 5)
    g = ag.to_pgo(pgo)
    s = pgo.Solver(g, pgo.Options(linear_solver=2))
    b = np.ones(120)
    b[:3] = 0.0
    with pytest.raises(pgo.PgoError) as e:      # no linearisation yet
        s.direct_solve(b)
    assert e.value.status == -1
    s.lm_begin()
    for bad in (-2, 4):
        with pytest.raises(pgo.PgoError) as e:
            s.direct_solve(b, bad)
        assert e.value.status == -1
    assert pgo.lib().pgo_debug_direct_solve(s._h, None, 0, None) == -1
    y = s.direct_solve(b, 0)                    # the state of iteration 0 (lm_begin) is a state too
    assert np.isfinite(y).all() and np.abs(s.system_spmv(y) - b).max() < 1e-8
    s.close()
    p = pgo.Solver(g, pgo.Options(linear_solver=1))
    p.lm_begin()
    with pytest.raises(pgo.PgoError) as e:
        p.direct_solve(b)
    assert e.value.status == -8
    i = p.info()
    assert (i.direct_separators, i.direct_segments, i.direct_refine_kernel) == (0, 0, 0)
    p.close()
