#!/usr/bin/env python3
"""What sparse absolute fixes buy at scale, and what the two prior kernels cost.

synth_manhattan(n, 4.0, 0.10, seed) at n = 10k / 100k / 1M from dead reckoning; position-only priors diag(1 / sigma^2,
1 / sigma^2, 0) on every K-th pose at pgo_synth_manhattan_truth plus seeded Gaussian noise of sigma metres; METHOD 0 and METHOD 1,
50 LM iterations with bench.py's forcing term (pcg_rtol 0.1, at most 500 PCG iterations, no termination tests).  Prints, per size
and method, the ATE rmse against the truth (unaligned and after a rigid fit) of the start, of the solve without priors and of the
solve with them; then the time of the prior kernels with a prior on EVERY pose of the largest graph: k_prior_add as the difference
of pgo_bench_assemble with and without priors (device events), k_prior_eval as the difference of a cost-only pgo_eval (host
clock, median), against their algorithmic bytes (csrc/prior.hip.h); then one JSON line with everything.  Needs a GPU.

    python scripts/prior_report.py [--sizes 10000,100000,1000000] [--every 100] [--sigma 0.5] [--iters 50] [--out FILE.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=20260410)
    ap.add_argument("--pcg-rtol", type=float, default=0.1)
    ap.add_argument("--pcg-max-iters", type=int, default=500)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows, timing = [], None
    sizes = [int(v) for v in args.sizes.split(",")]
    for n in sizes:
        g = P.synth_manhattan(n, 4.0, 0.10, args.seed)
        truth = P.synth_manhattan_truth(n, args.seed)
        rng = np.random.default_rng(args.seed)
        pose = np.arange(args.every, n, args.every)
        mean = truth[pose].copy()
        mean[:, :2] += args.sigma * rng.standard_normal((len(pose), 2))
        info = np.tile(np.array([1.0 / args.sigma ** 2, 0.0, 0.0, 1.0 / args.sigma ** 2, 0.0, 0.0]), (len(pose), 1))
        for method in (0, 1):
            opt = P.Options(method=method, max_iters=args.iters, ftol=0.0, gtol=0.0, ptol=0.0, min_radius=0.0, pcg_rtol=args.pcg_rtol,
                            pcg_max_iters=args.pcg_max_iters, pcg_check_every=10)
            row = {"poses": n, "edges": int(g.n_edges), "method": method, "priors": int(len(pose)), "sigma": args.sigma}
            for label in ("without", "with"):
                s = P.Solver(g, opt)
                if label == "with":
                    s.set_priors(pose, mean, info)
                row["start"] = s.trajectory_error(truth)["ate_rmse"]
                t0 = time.perf_counter()
                try:
                    summ = s.solve()
                    row[label + "_termination"], row[label + "_iterations"] = int(summ.termination), int(summ.iterations)
                except P.PgoError as e:
                    row[label + "_error"] = str(e)
                row[label + "_s"] = time.perf_counter() - t0
                row[label] = s.trajectory_error(truth)["ate_rmse"]
                row[label + "_aligned"] = s.trajectory_error(truth, align=True)["ate_rmse"]
                if label == "with":
                    d, chi2 = s.prior_residuals()
                    row["prior_rms_m"] = float(np.sqrt((d[:, :2] ** 2).sum(axis=1).mean()))
                s.close()
            rows.append(row)
            print("n %8d METHOD %d, %6d position priors (sigma %.2f m): ATE rmse %.4f m at the start; without priors %.4f (aligned %.4f), "
                  "%.2f s, %s iterations, termination %s; with %.4f (aligned %.4f), %.2f s, %s iterations, termination %s; rms distance "
                  "to the fixes %.3f m"
                  % (n, method, len(pose), args.sigma, row["start"], row["without"], row["without_aligned"], row["without_s"],
                     row.get("without_iterations"), row.get("without_termination", row.get("without_error")), row["with"], row["with_aligned"],
                     row["with_s"], row.get("with_iterations"), row.get("with_termination", row.get("with_error")),
                     row.get("prior_rms_m", float("nan"))), flush=True)
        if n == max(sizes):   # a prior on EVERY pose: the kernels at n priors
            s = P.Solver(g, P.Options(method=1))
            s.lm_begin()   # (pgo_bench_assemble times the assembly of a current linearisation)
            t_asm0 = min(s.bench_assemble(20).ms_avg for _ in range(3))

            def eval_ms():
                ts = []
                for _ in range(21):
                    t0 = time.perf_counter()
                    s.evaluate(want_r=False, want_J=False)
                    ts.append(1e3 * (time.perf_counter() - t0))
                return float(np.median(ts))
            t_eval0 = eval_ms()
            allp = np.arange(n)
            s.set_priors(allp, truth, np.tile(np.array([4.0, 0.0, 0.0, 4.0, 0.0, 0.0]), (n, 1)))
            s.lm_begin()   # (the records of k_prior_eval<true> exist before k_prior_add is timed)
            t_asm1 = min(s.bench_assemble(20).ms_avg for _ in range(3))
            t_eval1 = eval_ms()
            add_bytes, eval_bytes = n * (4 + 72 + 24 + 72 + 72), n * (4 + 24 + 24 + 48)   # (csrc/prior.hip.h; the cost-only eval writes nothing)
            timing = {"priors": n, "k_prior_add_ms": t_asm1 - t_asm0, "k_prior_add_bytes": add_bytes, "assemble_ms": t_asm0,
                      "k_prior_eval_ms": t_eval1 - t_eval0, "k_prior_eval_bytes": eval_bytes, "eval_call_ms": t_eval0}
            print("%d priors: k_prior_add %.4f ms on top of %.4f ms of assembly (%.0f MB algorithmic: %.2f TB/s); the cost-only k_prior_eval %.4f ms "
                  "on top of a %.4f ms pgo_eval call (%.0f MB: %.2f TB/s)"
                  % (n, timing["k_prior_add_ms"], t_asm0, add_bytes / 1e6, add_bytes / max(timing["k_prior_add_ms"], 1e-9) / 1e9,
                     timing["k_prior_eval_ms"], t_eval0, eval_bytes / 1e6, eval_bytes / max(timing["k_prior_eval_ms"], 1e-9) / 1e9), flush=True)
            s.close()
    line = json.dumps({"prior_report": rows, "kernels": timing})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
