#!/usr/bin/env python3
"""What a hierarchical start is worth, at scale.

synth_manhattan(n, 4.0, 0.10, seed) at n = 10k / 100k / 1M, METHOD 0 and 1, strides 16 and 64.  Per case: ATE rmse (unaligned
and aligned) and RPE of the dead-reckoned poses, after coarsen -> coarse solve -> prolong (Solver.initialize_hierarchical's
steps, timed one by one), and after the 50 LM iterations of scripts/score_report.py (bench.py's forcing term: pcg_rtol 0.1,
at most 500 PCG iterations, no termination tests) from that start -- next to section 4f's rows from dead reckoning.  At the
largest size it also times pgo_coarsen against the serial pgo_coarsen_plan on the same arrays.  One JSON line at the end.
Needs a GPU.

    python scripts/init_report.py [--sizes 10000,100000,1000000] [--strides 16,64] [--methods 0,1] [--iters 50]
                                  [--coarse-iters 50] [--seed 20260410] [--out FILE.json]
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


def score(s, truth):
    e = s.trajectory_error(truth)
    out = {k: e[k] for k in KEYS}
    out["ate_rmse_aligned"] = s.trajectory_error(truth, align=True)["ate_rmse"]
    return out


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--strides", default="16,64")
    ap.add_argument("--methods", default="0,1")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--coarse-iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=20260410)
    ap.add_argument("--pcg-rtol", type=float, default=0.1)
    ap.add_argument("--pcg-max-iters", type=int, default=500)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sizes = [int(v) for v in args.sizes.split(",")]
    rows, serial = [], None
    for n in sizes:
        g = P.synth_manhattan(n, 4.0, 0.10, args.seed)
        truth = P.synth_manhattan_truth(n, args.seed)
        p0 = np.array(g.poses)
        for method in [int(v) for v in args.methods.split(",")]:
            for stride in [int(v) for v in args.strides.split(",")]:
                opt = P.Options(method=method, max_iters=args.iters, ftol=0.0, gtol=0.0, ptol=0.0, min_radius=0.0, pcg_rtol=args.pcg_rtol,
                                pcg_max_iters=args.pcg_max_iters, pcg_check_every=10)
                s = P.Solver(g, opt)
                init = score(s, truth)
                s.coarsen(stride)                                   # (tables and buffers exist after the first call)
                (cg, origin), t_coarsen = timed(lambda: s.coarsen(stride))
                coarse, t_create = timed(lambda: P.Solver(cg, P.Options(method=method, pcg_rtol=1e-10, max_iters=args.coarse_iters)))
                csum, t_csolve = timed(coarse.solve)
                X = coarse.poses()
                info = coarse.info()
                coarse.close()
                _, t_prolong = timed(lambda: s.prolong(stride, X))
                prolonged = score(s, truth)
                summ, t_solve = timed(s.solve)
                final = score(s, truth)
                s.close()
                row = {"poses": n, "edges": int(g.n_edges), "method": method, "stride": stride, "key_poses": int(cg.n_poses),
                       "coarse_edges": int(cg.n_edges), "coarse_linear_solver": int(info.linear_solver), "coarse_iterations": int(csum.iterations),
                       "coarse_termination": int(csum.termination), "coarse_pcg_iters": int(csum.total_pcg_iters),
                       "coarsen_s": t_coarsen, "coarse_create_s": t_create, "coarse_solve_s": t_csolve, "prolong_s": t_prolong,
                       "fine_solve_s": t_solve, "fine_iterations": int(summ.iterations), "fine_cost": [summ.initial_cost, summ.final_cost],
                       "initial": init, "prolonged": prolonged, "final": final}
                rows.append(row)
                print("n %8d METHOD %d stride %3d (%6d key poses, %8d edges): ATE rmse %.4f -> %.4f -> %.4f m (aligned %.4f -> %.4f -> %.4f); "
                      "RPE trans %.4f -> %.4f -> %.4f m; coarsen %.4f s, create %.3f s, coarse solve %.3f s (%d iterations, %d PCG, termination %d), "
                      "prolong %.4f s, fine solve %.2f s"
                      % (n, method, stride, cg.n_poses, cg.n_edges, init["ate_rmse"], prolonged["ate_rmse"], final["ate_rmse"],
                         init["ate_rmse_aligned"], prolonged["ate_rmse_aligned"], final["ate_rmse_aligned"], init["rpe_trans_rmse"],
                         prolonged["rpe_trans_rmse"], final["rpe_trans_rmse"], t_coarsen, t_create, t_csolve, csum.iterations, csum.total_pcg_iters,
                         csum.termination, t_prolong, t_solve), flush=True)
        if n == max(sizes):   # the device against the serial statement on the same arrays
            stride = int(args.strides.split(",")[0])
            ia, ib, meas, kind = np.array(g.ia), np.array(g.ib), np.array(g.meas), np.array(g.kind)
            _, t_plan = timed(lambda: P.coarsen_plan(n, ia, ib, meas, kind, stride))
            s = P.Solver(g, P.Options(method=1))
            _, t_first = timed(lambda: s.coarsen(stride))
            t_dev = min(timed(lambda: s.coarsen(stride))[1] for _ in range(5))
            s.close()
            serial = {"poses": n, "stride": stride, "coarsen_plan_s": t_plan, "coarsen_first_call_s": t_first, "coarsen_s": t_dev}
            print("n %8d stride %d: pgo_coarsen_plan %.4f s, pgo_coarsen %.4f s (first call, with the tables: %.4f s)"
                  % (n, stride, t_plan, t_dev, t_first), flush=True)
        del g
    line = json.dumps({"init_report": rows, "coarsen_vs_plan": serial})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
