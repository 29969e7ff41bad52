#!/usr/bin/env python3
"""Accuracy of METHOD 0 and METHOD 1 against the generator's ground truth, at scale.

synth_manhattan(n, 4.0, 0.10, seed) at n = 10k / 100k / 1M; 50 LM iterations with bench.py's forcing term (pcg_rtol 0.1, at most
500 PCG iterations, no termination tests).  Prints, per size and method: ATE and RPE of the dead-reckoned poses and of the
result (pgo_trajectory_error, unaligned: pose 0 is constant at the truth's origin), the share of bogus and of true loops with
weight < 0.5 (pgo_edge_weights), and the wall time of one score call; then one JSON line with everything.  Needs a GPU.

    python scripts/score_report.py [--sizes 10000,100000,1000000] [--iters 50] [--seed 20260410] [--out FILE.json]
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

KEYS = ("ate_rmse", "ate_max", "rot_rmse", "rpe_trans_rmse", "rpe_rot_rmse")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=20260410)
    ap.add_argument("--pcg-rtol", type=float, default=0.1)
    ap.add_argument("--pcg-max-iters", type=int, default=500)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for n in [int(v) for v in args.sizes.split(",")]:
        g = P.synth_manhattan(n, 4.0, 0.10, args.seed)
        truth = P.synth_manhattan_truth(n, args.seed)
        kind = np.array(g.kind)
        for method in (0, 1):
            opt = P.Options(method=method, max_iters=args.iters, ftol=0.0, gtol=0.0, ptol=0.0, min_radius=0.0, pcg_rtol=args.pcg_rtol,
                            pcg_max_iters=args.pcg_max_iters, pcg_check_every=10)
            s = P.Solver(g, opt)
            init = s.trajectory_error(truth)
            t0 = time.perf_counter()
            summ = s.solve()
            t_solve = time.perf_counter() - t0
            s.trajectory_error(truth)                       # (buffers exist from the first call; this one warms the kernels)
            reps = 5
            t0 = time.perf_counter()
            for _ in range(reps):
                final = s.trajectory_error(truth)
            t_score = (time.perf_counter() - t0) / reps
            t0 = time.perf_counter()
            aligned = s.trajectory_error(truth, align=True)
            t_score_aligned = time.perf_counter() - t0
            s.edge_weights()
            t0 = time.perf_counter()
            w = s.edge_weights()
            t_weights = time.perf_counter() - t0
            down = w["weight"] < 0.5
            row = {"poses": n, "edges": int(g.n_edges), "bogus": int((kind == 2).sum()), "method": method, "lm_iterations": int(summ.iterations),
                   "final_cost": summ.final_cost, "solve_s": t_solve, "score_ms": 1e3 * t_score, "score_aligned_ms": 1e3 * t_score_aligned,
                   "edge_weights_ms": 1e3 * t_weights,
                   "initial": {k: init[k] for k in KEYS}, "final": {k: final[k] for k in KEYS}, "final_aligned_ate_rmse": aligned["ate_rmse"],
                   "bogus_down": float(down[kind == 2].mean()) if (kind == 2).any() else None,
                   "true_loops_down": float(down[kind == 1].mean()) if (kind == 1).any() else None}
            rows.append(row)
            print("n %8d METHOD %d: ATE rmse %.4f -> %.4f m (aligned %.4f), max %.3f -> %.3f; RPE trans %.4f -> %.4f m, rot %.5f -> %.5f rad; "
                  "weight < 0.5: %.1f %% of bogus, %.2f %% of true loops; solve %.2f s, score %.3f ms, edge weights %.3f ms"
                  % (n, method, init["ate_rmse"], final["ate_rmse"], aligned["ate_rmse"], init["ate_max"], final["ate_max"],
                     init["rpe_trans_rmse"], final["rpe_trans_rmse"], init["rpe_rot_rmse"], final["rpe_rot_rmse"],
                     100 * (row["bogus_down"] or 0.0), 100 * (row["true_loops_down"] or 0.0), t_solve, 1e3 * t_score, 1e3 * t_weights), flush=True)
            s.close()
    line = json.dumps({"score_report": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
