#!/usr/bin/env python3
"""Loop support (pgo_loop_support: loop edges judged by odometry cycle consistency) on the synthetic world, from dead reckoning
(DESIGN.md section 4i).

synth_manhattan(n, 4.0, 0.10, seed) at the given sizes.  Per size: what the filter decides, by edge kind (kind 1 = true closure,
kind 2 = bogus), the wall time of a call (the first one, which builds the tables, and a repeated one), and the ATE against
synth_manhattan_truth (unaligned: pose 0 is constant at the truth's origin; aligned in brackets) of
    dead reckoning | filter + METHOD 0 (Trivial loss) | filter + METHOD 1 (DCS, Huber(0.01)) | filter +
    initialize_hierarchical(stride, carry_weights) + METHOD 0 / 1 / 1 through a METHOD 0 coarse solve | METHOD 1 alone | GNC (below --gnc-below poses; section 4h has the larger sizes)
Graphs of --exact-below poses and more run inexact PCG solves (--pcg-rtol / --pcg-max-iters).  One JSON line at the end.  Needs a
GPU; not part of bench.py.

    python scripts/loop_support_report.py [--sizes 2000,10000,100000,1000000] [--seed 20260410] [--stride 16] [--min-support 1]
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


def options(n, args, **kw):
    if n >= args.exact_below:
        kw.update(pcg_rtol=args.pcg_rtol, pcg_max_iters=args.pcg_max_iters, pcg_check_every=10)
    return P.Options(max_iters=args.iters, **kw)


def score(s, truth):
    e = s.trajectory_error(truth)
    return {"ate_rmse": e["ate_rmse"], "ate_max": e["ate_max"], "ate_rmse_aligned": s.trajectory_error(truth, align=True)["ate_rmse"]}


def solve(s, truth):
    t0 = time.perf_counter()
    try:
        summ = s.solve()
    except P.PgoError as e:
        return dict(score(s, truth), failed=str(e))
    return dict(score(s, truth), solve_s=time.perf_counter() - t0, iterations=int(summ.iterations), termination=int(summ.termination))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,10000,100000,1000000")
    ap.add_argument("--seed", type=int, default=20260410)
    ap.add_argument("--stride", type=int, default=16)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--tol-xy", type=float, default=0.1)
    ap.add_argument("--tol-th", type=float, default=0.05)
    ap.add_argument("--min-support", type=int, default=1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--exact-below", type=int, default=20000)
    ap.add_argument("--pcg-rtol", type=float, default=0.01)
    ap.add_argument("--pcg-max-iters", type=int, default=5000)
    ap.add_argument("--gnc-below", type=int, default=20000)
    ap.add_argument("--cbar", type=float, default=0.5)
    ap.add_argument("--plan-below", type=int, default=20000, help="time the serial host statement below this size")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    kw = dict(window=args.window, tol_xy=args.tol_xy, tol_th=args.tol_th, min_support=args.min_support)
    rows = []
    for n in [int(v) for v in args.sizes.split(",")]:
        g = P.synth_manhattan(n, 4.0, 0.10, args.seed)
        truth = P.synth_manhattan_truth(n, args.seed)
        kind = np.array(g.kind)
        row = {"poses": n, "edges": int(g.n_edges), "exact": n < args.exact_below}
        # ---- the filter on a METHOD 0 handle, then the solve from dead reckoning
        s = P.Solver(g, options(n, args, method=0), losses=P.Loss("trivial"))
        row["dead_reckoning"] = score(s, truth)
        t0 = time.perf_counter()
        rec, st = s.loop_support(apply=True, **kw)
        first = time.perf_counter() - t0
        t0 = time.perf_counter()
        for _ in range(args.reps):
            s.loop_support(apply=True, **kw)
        again = (time.perf_counter() - t0) / args.reps
        sup = rec["n_consistent"] >= args.min_support
        row["filter"] = dict(st, first_call_ms=1e3 * first, call_ms=1e3 * again, closures=int((kind == 1).sum()), bogus=int((kind == 2).sum()),
                             closures_supported=int((sup & (kind == 1)).sum()), bogus_supported=int((sup & (kind == 2)).sum()),
                             mean_pairs=float(st["n_pairs_total"]) / max(st["n_selected"], 1))
        if n < args.plan_below:
            t0 = time.perf_counter()
            P.loop_support_plan(n, g.ia, g.ib, g.meas, g.kind, **kw)
            row["filter"]["plan_ms"] = 1e3 * (time.perf_counter() - t0)
        row["filter_m0"] = solve(s, truth)
        s.close()
        make = {0: lambda: P.Solver(g, options(n, args, method=0), losses=P.Loss("trivial")), 1: lambda: P.Solver(g, options(n, args, method=1))}
        s = make[1]()
        s.loop_support(apply=True, **kw)
        row["filter_m1"] = solve(s, truth)
        s.close()
        for m in (0, 1, 2):   # (2: a METHOD 1 handle started through a METHOD 0 coarse solve)
            s = make[min(m, 1)]()
            s.loop_support(apply=True, **kw)
            t0 = time.perf_counter()
            coarse = s.initialize_hierarchical(args.stride, carry_weights=True,
                                               coarse_options=P.Options(method=0, pcg_rtol=1e-10) if m == 2 else None)
            init_s = time.perf_counter() - t0
            after_init = score(s, truth)
            row["filter_hier_m%d" % m] = dict(solve(s, truth), init_s=init_s, after_init=after_init, coarse_iterations=int(coarse.iterations),
                                              coarse_termination=int(coarse.termination))
            s.close()
        # ---- what the library had: METHOD 1, and GNC where it is the tool
        s = P.Solver(g, options(n, args, method=1))
        row["method1"] = solve(s, truth)
        s.close()
        if n < args.gnc_below:
            s = P.Solver(g, options(n, args, method=0), losses=P.Loss("trivial"))
            t0 = time.perf_counter()
            try:
                summ, rounds = s.gnc_solve(args.cbar, final_iters=args.iters)
                w = s.get_edge_weights()
                row["gnc"] = dict(score(s, truth), total_s=time.perf_counter() - t0, rounds=summ["rounds"],
                                  bogus_rejected=int(((w == 0.0) & (kind == 2)).sum()), closures_rejected=int(((w == 0.0) & (kind == 1)).sum()))
            except P.PgoError as e:
                row["gnc"] = dict(score(s, truth), failed=str(e))
            s.close()
        rows.append(row)
        f = lambda d: "ATE rmse %.4f (aligned %.4f) max %.3f m" % (d["ate_rmse"], d["ate_rmse_aligned"], d["ate_max"])
        t = lambda d: ("FAILED: " + d["failed"]) if "failed" in d else "%d iterations (termination %d), %.2f s" % (d["iterations"], d["termination"], d["solve_s"])
        fl = row["filter"]
        print("n %8d, %d edges (%s):" % (n, g.n_edges, "exact solves" if row["exact"] else "inexact PCG"))
        print("  filter           %d selected, %.1f pairs per loop (max %d): supported %d of %d closures, %d of %d bogus; first call %.1f ms, "
              "then %.2f ms%s" % (fl["n_selected"], fl["mean_pairs"], fl["max_pairs"], fl["closures_supported"], fl["closures"], fl["bogus_supported"],
                                  fl["bogus"], fl["first_call_ms"], fl["call_ms"], (", host plan %.0f ms" % fl["plan_ms"]) if "plan_ms" in fl else ""))
        print("  dead reckoning   %s" % f(row["dead_reckoning"]))
        print("  filter + M0      %s; %s" % (f(row["filter_m0"]), t(row["filter_m0"])))
        print("  filter + M1      %s; %s" % (f(row["filter_m1"]), t(row["filter_m1"])))
        for m in (0, 1, 2):
            h = row["filter_hier_m%d" % m]
            print("  filter + hier(%d) + M%s: %s after the start (%.2f s, coarse solve %d iterations, termination %d); then %s; %s"
                  % (args.stride, ("0", "1", "1 (METHOD 0 coarse solve)")[m], f(h["after_init"]), h["init_s"], h["coarse_iterations"], h["coarse_termination"], f(h), t(h)))
        print("  METHOD 1         %s; %s" % (f(row["method1"]), t(row["method1"])))
        if "gnc" in row:
            r = row["gnc"]
            print("  GNC              %s; %s" % (f(r), ("FAILED: " + r["failed"]) if "failed" in r else "%d rounds, %.2f s; rejected %d bogus, %d closures"
                                                 % (r["rounds"], r["total_s"], r["bogus_rejected"], r["closures_rejected"])))
        sys.stdout.flush()
    line = json.dumps({"loop_support_report": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
