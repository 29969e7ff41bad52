#!/usr/bin/env python3
"""Chordal initialisation (pgo_chordal_init: chordal rotations, then positions) on the synthetic world.

synth_manhattan(n, 4.0, 0.10, seed) at the given sizes, after loop_support(apply=True), with --rounds reject rounds (default
0 and 2).  Per size and rounds: the iterations of both stages (every solve), the wall time of the call, min |z|, the edges the
rounds rejected split into bogus (kind 2) and true closures (kind 1), and the ATE against synth_manhattan_truth (unaligned:
pose 0 is constant at the truth's origin; aligned in brackets) of the start and after the same --iters LM iterations with
METHOD 0 (Trivial loss) and METHOD 1 (DCS, Huber(0.01)).  The rows of section 4i (dead reckoning, filter + hierarchical start)
come from scripts/loop_support_report.py.  Graphs of --exact-below poses and more run inexact PCG solves.  One JSON line at the
end.  Needs a GPU; not part of bench.py.

    python scripts/chordal_report.py [--sizes 2000,10000,100000,1000000] [--rounds 0,2] [--seed 20260410]
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
    ap.add_argument("--rounds", default="0,2")
    ap.add_argument("--seed", type=int, default=20260410)
    ap.add_argument("--reject-xy", type=float, default=2.0)
    ap.add_argument("--reject-th", type=float, default=0.35)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--max-iters", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--methods", default="0,1")
    ap.add_argument("--exact-below", type=int, default=20000)
    ap.add_argument("--pcg-rtol", type=float, default=0.01)
    ap.add_argument("--pcg-max-iters", type=int, default=5000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    f = lambda d: "ATE rmse %.4f (aligned %.4f) max %.3f m" % (d["ate_rmse"], d["ate_rmse_aligned"], d["ate_max"])
    t = lambda d: ("FAILED: " + d["failed"]) if "failed" in d else "%d iterations (termination %d), %.2f s" % (d["iterations"], d["termination"], d["solve_s"])
    for n in [int(v) for v in args.sizes.split(",")]:
        g = P.synth_manhattan(n, 4.0, 0.10, args.seed)
        truth = P.synth_manhattan_truth(n, args.seed)
        kind = np.array(g.kind)
        print("n %8d, %d edges (%s):" % (n, g.n_edges, "exact solves" if n < args.exact_below else "inexact PCG"))
        for rounds in [int(v) for v in args.rounds.split(",")]:
            row = {"poses": n, "edges": int(g.n_edges), "rounds": rounds}
            for m in [int(v) for v in args.methods.split(",")]:
                s = P.Solver(g, options(n, args, method=m), **({"losses": P.Loss("trivial")} if m == 0 else {}))
                if "start" not in row:
                    row["dead_reckoning"] = score(s, truth)
                rec, st = s.loop_support(apply=True)
                kept = s.get_edge_weights() > 0.0
                t0 = time.perf_counter()
                try:
                    _, res, summ = s.chordal_init(commit=True, apply_weights=rounds > 0, rounds=rounds, reject_xy=args.reject_xy, reject_th=args.reject_th,
                                                  rtol=args.rtol, max_iters=args.max_iters)
                except P.PgoError as e:
                    row["failed"] = str(e)
                    print("  rounds %d: FAILED: %s" % (rounds, e))
                    s.close()
                    break
                wall = time.perf_counter() - t0
                if "start" not in row:
                    gone = kept & (s.get_edge_weights() == 0.0)
                    row.update(start=score(s, truth), wall_s=wall, summary=summ, bogus_left_by_filter=int((kept & (kind == 2)).sum()),
                               rejected_bogus=int((gone & (kind == 2)).sum()), rejected_closures=int((gone & (kind == 1)).sum()),
                               rejected_odometry=int((gone & (kind == 0)).sum()))
                    sv = summ["solves"]
                    print("  rounds %d: %s solves, iterations R / T %s, converged %s, %.3f s; min |z| %.3e, %d degenerate; bogus loops the filter left %d; "
                          "rejected %d bogus, %d closures, %d odometry-kind" % (rounds, summ["n_solves"], [x["iters"] for x in sv], [x["converged"] for x in sv], wall,
                                                                               summ["min_mag"], summ["n_degenerate"], row["bogus_left_by_filter"],
                                                                               row["rejected_bogus"], row["rejected_closures"], row["rejected_odometry"]))
                    print("    dead reckoning %s" % f(row["dead_reckoning"]))
                    print("    the start      %s" % f(row["start"]))
                row["m%d" % m] = solve(s, truth)
                print("    + METHOD %d     %s; %s" % (m, f(row["m%d" % m]), t(row["m%d" % m])))
                sys.stdout.flush()
                s.close()
            rows.append(row)
    line = json.dumps({"chordal_report": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
