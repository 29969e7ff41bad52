"""64 candidate loop edges through Solver.gate (one call, three columns per candidate) against the same 64 through 64
Solver.covariance([a, b], cross=True) calls (six columns each, the edge Jacobian and the 3x3 algebra left to the host), on
INTEL + 50 and on M3500; then, per solver of --solver (0 = PCG, 1 = the handle's direct solve, on handles that are on it),
all loop edges of the graph through one Solver.gate call and 24 / all poses through Solver.covariance.  Report only: seconds,
columns, passes, PCG iterations and the largest true residual.  Run on the GPU box.

    python scripts/gate_timing.py [--solver 0 1] [--graphs INTEL+50 M3500]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toy_robust_backend_slam_amd as P   # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
N_CAND = 64


def timed(call, reps=3):
    """best of `reps` wall times of call(), and its last result"""
    best = np.inf
    for _ in range(reps):
        t = time.perf_counter()
        out = call()
        best = min(best, time.perf_counter() - t)
    return best, out


def row(label, solver, dt, rep):
    print(f"{label:34s} solver {solver}: {dt:8.4f} s  columns {rep['columns']:5d}  passes {rep['passes']:3d}  "
          f"pcg iterations (sum over columns) {rep['pcg_iters_total']:7d}  max_rel_residual {rep['max_rel_residual']:.2e}")


def run(name, n_out, iters, solvers):
    g = P.ReadG2O(os.path.join(DATA, name + ".g2o"))
    if n_out:
        g.add_random_C(n_out, 1)
    s = P.Solver(g, P.Options(method=1, max_iters=iters))
    s.solve()
    tag = f"{name}+{n_out}"
    rng = np.random.default_rng(1)
    ia = rng.integers(1, g.n_poses, N_CAND).astype(np.int32)
    ib = ((ia + rng.integers(1, g.n_poses - 1, N_CAND) - 1) % (g.n_poses - 1) + 1).astype(np.int32)
    ib = np.where(ib == ia, ib % (g.n_poses - 1) + 1, ib).astype(np.int32)
    meas = rng.standard_normal((N_CAND, 3))
    s.gate(ia[:1], ib[:1], meas[:1])           # (the first call builds the coarse level where the handle has none)
    for ppp in (8, 16):
        t = time.perf_counter()
        got, rep = s.gate(ia, ib, meas, poses_per_pass=ppp)
        dt = time.perf_counter() - t
        print(f"{tag} gate       {ppp:2d}/pass: {dt:8.4f} s  columns {rep['columns']:4d}  passes {rep['passes']:2d}  "
              f"pcg iterations (sum over columns) {rep['pcg_iters_total']}")
    t = time.perf_counter()
    cols = its = 0
    worst = 0.0
    for k in range(N_CAND):
        M, rep = s.covariance([ia[k], ib[k]], cross=True)
        cols += rep["columns"]
        its += rep["pcg_iters_total"]
        J = got["J"][k]
        worst = max(worst, np.linalg.norm(J @ M @ J.T - got["P"][k]) / np.linalg.norm(got["P"][k]))
    dt = time.perf_counter() - t
    print(f"{tag} covariance x {N_CAND}   : {dt:8.4f} s  columns {cols:4d}  passes {N_CAND:2d}  "
          f"pcg iterations (sum over columns) {its}   (max |dP|/|P| between the routes {worst:.1e})")
    # the solver column: the same calls per solver (solver = 1 on handles on the direct solve only)
    ia_g, ib_g = np.array(g.ia), np.array(g.ib)
    loops = np.nonzero(np.abs(ia_g - ib_g) != 1)[0]
    la, lb, lm = ia_g[loops].astype(np.int32), ib_g[loops].astype(np.int32), np.array(g.meas)[loops]
    p24 = np.unique(np.linspace(1, g.n_poses - 1, 24).astype(np.int64))
    every = np.arange(g.n_poses)
    for solver in solvers:
        if solver == 1 and s.info().linear_solver != 2:
            print(f"{tag}: not on the direct solve, no solver = 1 rows")
            continue
        kw = dict(solver=solver) if solver else dict(poses_per_pass=16)
        row(f"{tag} gate, {N_CAND} candidates", solver, *timed(lambda: s.gate(ia, ib, meas, **kw)[1]))
        row(f"{tag} gate, all {loops.size} loops", solver, *timed(lambda: s.gate(la, lb, lm, **kw)[1], reps=2))
        row(f"{tag} covariance, {p24.size} poses", solver, *timed(lambda: s.covariance(p24, **kw)[1]))
        row(f"{tag} covariance, all {every.size} poses", solver, *timed(lambda: s.covariance(every, **kw)[1], reps=1))
    s.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--solver", type=int, nargs="+", default=[0, 1], help="pgo_covariance_options.solver values to time")
    ap.add_argument("--graphs", nargs="+", default=["INTEL+50", "M3500"])
    a = ap.parse_args()
    for gname in a.graphs:
        name, _, n_out = gname.partition("+")
        run(name, int(n_out or 0), 5 if name != "M3500" else 3, a.solver)
