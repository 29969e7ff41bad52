#!/usr/bin/env python3
"""Graduated non-convexity (GNC-TLS, pgo_gnc_solve) against METHOD 1 on the synthetic world, from dead reckoning (DESIGN.md
section 4h).

synth_manhattan(n, 4.0, 0.10, seed) at the given sizes.  From the same dead-reckoned start, per size:
    dead reckoning | METHOD 1 (DCS, Huber(0.01)) | GNC (METHOD 0, Trivial loss) | GNC after initialize_hierarchical(stride)
and for each the ATE against synth_manhattan_truth (unaligned: pose 0 is constant at the truth's origin; with --align also after
a rigid fit), the wall time, and for the GNC runs the rounds, the wall time per round and the confusion counts of "weight 0"
against kind == 2.  Graphs of --exact-below poses and more run inexact PCG solves: --pcg-rtol / --pcg-max-iters, by default bench.py's forcing term
(0.1, at most 500 PCG iterations).
--kernels adds the kernel timings of section 4h: K1's general instantiation with and without a weight plane (pgo_bench_eval), and
pgo_gnc_update against pgo_edge_weights.  One JSON line at the end.  Needs a GPU; not part of bench.py.

    python scripts/gnc_report.py [--sizes 2000,10000,100000] [--seed 20260410] [--cbar 0.5] [--stride 16] [--align] [--kernels | --kernels-only]
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


def score(s, truth, align):
    e = s.trajectory_error(truth)
    out = {"ate_rmse": e["ate_rmse"], "ate_max": e["ate_max"]}
    if align:
        out["ate_rmse_aligned"] = s.trajectory_error(truth, align=True)["ate_rmse"]
    return out


def confusion(w, kind):
    rej = w == 0.0
    return {"bogus": int((kind == 2).sum()), "bogus_rejected": int((rej & (kind == 2)).sum()), "closures": int((kind == 1).sum()),
            "closures_rejected": int((rej & (kind == 1)).sum()), "nonbinary": int(((w > 0.0) & (w < 1.0)).sum())}


def run_gnc(g, truth, kind, n, args, stride):
    s = P.Solver(g, options(n, args, method=0), losses=P.Loss("trivial"))
    row = {"init_stride": stride}
    t0 = time.perf_counter()
    if stride:
        s.initialize_hierarchical(stride)
        row["init_s"] = time.perf_counter() - t0
        row["after_init"] = score(s, truth, args.align)
    t1 = time.perf_counter()
    try:
        summ, rounds = s.gnc_solve(args.cbar, inner_iters=args.inner, final_iters=args.iters, max_rounds=args.max_rounds)
    except P.PgoError as e:   # (a failed inner solve: reported, with the poses of the last good round)
        row.update(score(s, truth, args.align), failed=str(e))
        s.close()
        return row
    row["gnc_s"] = time.perf_counter() - t1
    row["total_s"] = time.perf_counter() - t0
    row.update(score(s, truth, args.align))
    row.update(rounds=summ["rounds"], hit_max_rounds=summ["hit_max_rounds"], mu0=summ["mu0"], rmax2=summ["rmax2"],
               round_ms=[1e3 * r["seconds"] for r in rounds], lm_iterations=[r["lm_iterations"] for r in rounds],
               final_iterations=summ["final_solve"]["iterations"], final_termination=summ["final_solve"]["termination"])
    row.update(confusion(s.get_edge_weights(), kind))
    s.close()
    return row


def kernels(g, n, args):
    """K1's general instantiation with and without the plane; pgo_gnc_update against pgo_edge_weights"""
    s = P.Solver(g, options(n, args, method=0), losses=[P.Loss("huber", 0.01), P.Loss("cauchy", 0.5)])   # two classes: general
    out = {}
    for jac in (True, False):
        s.set_edge_weights(None)
        s.bench_eval(5, jac)
        a = s.bench_eval(args.reps, jac).ms_avg
        s.set_edge_weights(np.random.default_rng(1).random(g.n_edges))
        s.bench_eval(5, jac)
        b = s.bench_eval(args.reps, jac).ms_avg
        out["k1_general_jac%d_ms" % jac] = [a, b]
    s.set_edge_weights(None)
    for name, call in (("edge_weights", lambda: s.edge_weights()), ("gnc_update_measure", lambda: s.gnc_update(args.cbar, 0.0)),
                       ("gnc_update", lambda: s.gnc_update(args.cbar, 0.05))):
        call()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            call()
        out[name + "_call_ms"] = 1e3 * (time.perf_counter() - t0) / args.reps
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,10000,100000")
    ap.add_argument("--seed", type=int, default=20260410)
    ap.add_argument("--cbar", type=float, default=0.5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--max-rounds", type=int, default=100)
    ap.add_argument("--stride", type=int, default=16)
    ap.add_argument("--exact-below", type=int, default=20000)
    ap.add_argument("--pcg-rtol", type=float, default=0.1)
    ap.add_argument("--pcg-max-iters", type=int, default=500)
    ap.add_argument("--align", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="the kernel timings without the solves")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for n in [int(v) for v in args.sizes.split(",")]:
        g = P.synth_manhattan(n, 4.0, 0.10, args.seed)
        truth = P.synth_manhattan_truth(n, args.seed)
        kind = np.array(g.kind)
        row = {"poses": n, "edges": int(g.n_edges), "exact": n < args.exact_below}
        if args.kernels_only:
            row["kernels"] = kernels(g, n, args)
            rows.append(row)
            print("n %8d, %d edges: kernels: %s" % (n, g.n_edges, json.dumps(row["kernels"])), flush=True)
            continue
        s = P.Solver(g, options(n, args, method=1))
        row["dead_reckoning"] = score(s, truth, args.align)
        t0 = time.perf_counter()
        summ = s.solve()
        row["method1"] = dict(score(s, truth, args.align), solve_s=time.perf_counter() - t0, iterations=int(summ.iterations),
                              termination=int(summ.termination))
        s.close()
        row["gnc"] = run_gnc(g, truth, kind, n, args, 0)
        row["hier_gnc"] = run_gnc(g, truth, kind, n, args, args.stride)
        if args.kernels:
            row["kernels"] = kernels(g, n, args)
        rows.append(row)
        f = lambda d: "ATE rmse %.4f max %.3f m%s" % (d["ate_rmse"], d["ate_max"], (" (aligned %.4f)" % d["ate_rmse_aligned"]) if args.align else "")
        print("n %8d, %d edges (%s):" % (n, g.n_edges, "exact solves" if row["exact"] else "inexact PCG"))
        print("  dead reckoning   %s" % f(row["dead_reckoning"]))
        print("  METHOD 1         %s; %d iterations, %.2f s" % (f(row["method1"]), row["method1"]["iterations"], row["method1"]["solve_s"]))
        for key, label in (("gnc", "GNC             "), ("hier_gnc", "hier(%d) + GNC  " % args.stride)):
            r = row[key]
            if "failed" in r:
                print("  %s %s; FAILED: %s" % (label, f(r), r["failed"]))
                continue
            print("  %s %s; %d rounds%s, %.2f s (%.1f ms per round), final solve %d iterations; rejected %d of %d bogus, %d of %d closures, %d non-binary"
                  % (label, f(r), r["rounds"], " (max_rounds)" if r["hit_max_rounds"] else "", r["total_s"],
                     float(np.mean(r["round_ms"])) if r["round_ms"] else 0.0, r["final_iterations"], r["bogus_rejected"], r["bogus"],
                     r["closures_rejected"], r["closures"], r["nonbinary"]))
        if args.kernels:
            print("  kernels: %s" % json.dumps(row["kernels"]))
        sys.stdout.flush()
    line = json.dumps({"gnc_report": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
