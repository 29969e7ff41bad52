"""64 candidate loop edges through Solver.gate (one call, three columns per candidate) against the same 64 through 64
Solver.covariance([a, b], cross=True) calls (six columns each, the edge Jacobian and the 3x3 algebra left to the host), on
INTEL + 50 and on M3500.  Report only: seconds and PCG columns of both routes.  Run on the GPU box."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toy_robust_backend_slam_amd as P   # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
N_CAND = 64


def run(name, n_out, iters):
    g = P.ReadG2O(os.path.join(DATA, name + ".g2o"))
    if n_out:
        g.add_random_C(n_out, 1)
    s = P.Solver(g, P.Options(method=1, max_iters=iters))
    s.solve()
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
        print(f"{name}+{n_out} gate       {ppp:2d}/pass: {dt:8.4f} s  columns {rep['columns']:4d}  passes {rep['passes']:2d}  "
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
    print(f"{name}+{n_out} covariance x {N_CAND}   : {dt:8.4f} s  columns {cols:4d}  passes {N_CAND:2d}  "
          f"pcg iterations (sum over columns) {its}   (max |dP|/|P| between the routes {worst:.1e})")
    s.close()


if __name__ == "__main__":
    run("INTEL", 50, 5)
    run("M3500", 0, 3)
