#!/usr/bin/env python3
"""Posterior sampling (pgo_posterior_sample: all-pose marginal covariances by perturb-and-MAP) on the datasets and the synthetic
world.

Cases: INTEL + 50 (METHOD 1, both solvers), M3500 (METHOD 1), synth_manhattan(n, 4.0, 0.10, seed) at the given sizes after
loop_support(apply) + chordal_init(commit) + METHOD 0.  Per case and per rtol in 1e-10 / 1e-6 / 1e-4, for S = 64 and 256 samples:
seconds, passes, PCG iterations per sample, the largest true residual; and where the exact blocks are affordable (a dataset on
the direct solve whole, the others on a pose subset, by pgo_pose_covariance at rtol 1e-10) the realised error of the estimate: the
worst and the mean whitened error || L^-1 C L^-T - I ||_F over the poses compared, in units of sqrt(12 / S) (1 = the expected
root mean square of an exact sampler).  A case that fails or exceeds --budget-s seconds says so and the script goes on.
One JSON line per case as it finishes, flushed.  Needs a GPU; not part of bench.py.

    python scripts/sample_report.py [--sizes 10000,100000,1000000] [--samples 64,256] [--rtols 1e-10,1e-6,1e-4] [--budget-s 120]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toy_robust_backend_slam_amd as P  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")


def whitened(C, Sigma):
    out = []
    for c, s in zip(C, Sigma):
        Li = np.linalg.inv(np.linalg.cholesky(s))
        out.append(np.linalg.norm(Li @ c @ Li.T - np.eye(3)))
    return np.array(out)


def run_case(label, s, solver, idx, args):
    exact = None
    rows = []
    t_case = time.perf_counter()
    if idx is not None:
        t0 = time.perf_counter()
        try:
            exact, rep = s.covariance(idx, solver=1 if s.info().linear_solver == 2 else 0)
            exact_s = time.perf_counter() - t0
        except P.PgoError as e:
            exact, exact_s = None, str(e)
    for rtol in args.rtols:
        for S in args.samples:
            if time.perf_counter() - t_case > args.budget_s:
                rows.append(dict(rtol=rtol, samples=S, skipped="the case's time budget is used up"))
                continue
            t0 = time.perf_counter()
            try:
                _, cov, rep = s.sample(S, seed=args.seed, want_deltas=False, solver=solver, rtol=rtol, samples_per_pass=args.per_pass)
            except P.PgoError as e:
                rows.append(dict(rtol=rtol, samples=S, failed=str(e)))
                continue
            row = dict(rtol=rtol, samples=S, seconds=time.perf_counter() - t0, passes=rep["passes"],
                       pcg_iters_per_sample=rep["pcg_iters_total"] / S, max_rel_residual=rep["max_rel_residual"])
            if exact is not None:
                w = whitened(cov[idx], exact) / np.sqrt(12.0 / S)
                row.update(whitened_worst=float(w.max()), whitened_mean=float(w.mean()), poses_compared=int(len(idx)))
            rows.append(row)
    out = dict(case=label, solver=solver, n_poses=s.n_poses, n_edges=s.n_edges, rows=rows)
    if idx is not None:
        out["exact_blocks_s"] = exact_s
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--samples", default="64,256")
    ap.add_argument("--rtols", default="1e-10,1e-6,1e-4")
    ap.add_argument("--seed", type=int, default=20260410)
    ap.add_argument("--per-pass", type=int, default=24)
    ap.add_argument("--subset", type=int, default=48, help="poses of a synthetic graph whose exact blocks are computed")
    ap.add_argument("--budget-s", type=float, default=120.0)
    ap.add_argument("--datasets", default="INTEL,M3500")
    args = ap.parse_args()
    args.samples = [int(v) for v in args.samples.split(",") if v]
    args.rtols = [float(v) for v in args.rtols.split(",") if v]

    for name in [v for v in args.datasets.split(",") if v]:
        g = P.ReadG2O(os.path.join(DATA, name + ".g2o"))
        if name == "INTEL":
            g.add_random_C(50, 1)
        s = P.Solver(g, P.Options(method=1, max_iters=50))
        s.solve()
        idx = np.arange(1, g.n_poses) if s.info().linear_solver == 2 else np.unique(np.linspace(1, g.n_poses - 1, 8 * args.subset).astype(np.int64))
        run_case(name + ("+50" if name == "INTEL" else ""), s, 0, idx, args)
        if s.info().linear_solver == 2:
            run_case(name + ("+50" if name == "INTEL" else ""), s, 1, idx, args)
        s.close()

    for n in [int(v) for v in args.sizes.split(",") if v]:
        g = P.synth_manhattan(n, 4.0, 0.10, args.seed)
        kw = dict(pcg_rtol=0.01, pcg_max_iters=5000, pcg_check_every=10) if n >= 20000 else {}
        s = P.Solver(g, P.Options(method=0, max_iters=50, **kw))
        try:
            s.loop_support(apply=True)
            s.chordal_init(commit=True)
            s.solve()
        except P.PgoError as e:
            print(json.dumps(dict(case="synth%d" % n, failed=str(e))), flush=True)
            s.close()
            continue
        idx = np.unique(np.linspace(1, n - 1, args.subset).astype(np.int64))
        run_case("synth%d" % n, s, 0, idx, args)
        s.close()


if __name__ == "__main__":
    main()
