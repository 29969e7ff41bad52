#!/usr/bin/env python3
"""Max-mixture edges with a null hypothesis (pgo_set_mixture_null, pgo_mixture_solve) against METHOD 1 and GNC on the synthetic
world.

synth_manhattan(n, 4.0, 0.10, seed) at the given sizes.  Every run starts as section 4j's: loop_support(apply=True), then
chordal_init(commit=True) with --chordal-rounds reject rounds (default 0; the blocks they drop stay dropped).  Per size:
    METHOD 1 (DCS, Huber(0.01)) | GNC (METHOD 0, Trivial loss, the loops the filter kept) | the null-hypothesis mixture (METHOD 0,
    Trivial loss, (pi, scale) beside every loop the filter kept)
and for each the ATE against synth_manhattan_truth (unaligned: pose 0 is constant at the truth's origin; aligned in brackets)
and the wall time; for the mixture also the rounds and the share of the kept bogus loops and of the kept true closures that end
on the null component.  Graphs of --exact-below poses and more run inexact PCG solves.  --kernel adds the time of a
pgo_mixture_select call (the select kernel, the fold, one 64-byte copy and the synchronisation) with and without apply.  One JSON
line at the end.  Needs a GPU; not part of bench.py.

    python scripts/mixture_report.py [--sizes 2000,10000,100000,1000000] [--pi 6e5] [--scale 1e-4] [--inner 2] [--chordal-rounds 0] [--kernel]
"""
import argparse
import ctypes as C
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


def start(g, n, args, method):
    """a handle at section 4j's start; returns (handle, the loops the filter kept, seconds)"""
    s = P.Solver(g, options(n, args, method=method), **({"losses": P.Loss("trivial")} if method == 0 else {}))
    t0 = time.perf_counter()
    s.loop_support(apply=True)
    r = args.chordal_rounds   # (reject rounds drop further blocks: METHOD 0 and 1 keep them dropped, section 4j)
    s.chordal_init(commit=True, apply_weights=r > 0, rounds=r, reject_xy=args.reject_xy, reject_th=args.reject_th, rtol=1e-8, max_iters=20000)
    kept = s.get_edge_weights() > 0.0
    return s, kept, time.perf_counter() - t0


def select_ms(s, apply, reps):
    st = P.MixStats()
    call = lambda: P._check(P.lib().pgo_mixture_select(s._h, apply, C.byref(st), None, None))
    for _ in range(3):
        call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return {"min": min(t), "median": float(np.median(t)), "n_mix": st.n_mix}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,10000,100000,1000000")
    ap.add_argument("--seed", type=int, default=20260410)
    ap.add_argument("--pi", type=float, default=6e5)
    ap.add_argument("--scale", type=float, default=1e-4)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--max-rounds", type=int, default=50)
    ap.add_argument("--cbar", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--exact-below", type=int, default=20000)
    ap.add_argument("--pcg-rtol", type=float, default=0.01)
    ap.add_argument("--pcg-max-iters", type=int, default=5000)
    ap.add_argument("--chordal-rounds", type=int, default=0, help="reject rounds of chordal_init (section 4j ran 0 and 2)")
    ap.add_argument("--reject-xy", type=float, default=2.0)
    ap.add_argument("--reject-th", type=float, default=0.35)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    f = lambda d: "ATE rmse %.4f (aligned %.4f) max %.3f m" % (d["ate_rmse"], d["ate_rmse_aligned"], d["ate_max"])
    for n in [int(v) for v in args.sizes.split(",")]:
        g = P.synth_manhattan(n, 4.0, 0.10, args.seed)
        truth = P.synth_manhattan_truth(n, args.seed)
        kind = np.array(g.kind)
        row = {"poses": n, "edges": int(g.n_edges), "exact": n < args.exact_below, "pi": args.pi, "scale": args.scale, "chordal_rounds": args.chordal_rounds}
        print("n %8d, %d edges (%s):" % (n, g.n_edges, "exact solves" if row["exact"] else "inexact PCG"), flush=True)
        # METHOD 1
        s, kept, t_start = start(g, n, args, 1)
        row["start"] = dict(score(s, truth), seconds=t_start, bogus_kept=int((kept & (kind == 2)).sum()), closures_kept=int((kept & (kind == 1)).sum()))
        print("  the start        %s; the filter kept %d bogus loops and %d closures" % (f(row["start"]), row["start"]["bogus_kept"], row["start"]["closures_kept"]))
        t0 = time.perf_counter()
        try:
            summ = s.solve()
            row["method1"] = dict(score(s, truth), seconds=time.perf_counter() - t0, iterations=int(summ.iterations))
            print("  METHOD 1         %s; %d iterations, %.2f s" % (f(row["method1"]), summ.iterations, row["method1"]["seconds"]), flush=True)
        except P.PgoError as e:
            row["method1"] = dict(score(s, truth), failed=str(e))
            print("  METHOD 1         FAILED: %s" % e)
        s.close()
        # GNC over the loops the filter kept
        s, kept, _ = start(g, n, args, 0)
        loops = kept & (kind != 0)
        t0 = time.perf_counter()
        try:
            summ, rounds = s.gnc_solve(args.cbar, select=loops, final_iters=args.iters)
            w = s.get_edge_weights()
            row["gnc"] = dict(score(s, truth), seconds=time.perf_counter() - t0, rounds=summ["rounds"],
                              bogus_rejected=int((loops & (kind == 2) & (w == 0.0)).sum()), closures_rejected=int((loops & (kind == 1) & (w == 0.0)).sum()))
            print("  GNC              %s; %d rounds, %.2f s; rejected %d bogus, %d closures" % (
                f(row["gnc"]), summ["rounds"], row["gnc"]["seconds"], row["gnc"]["bogus_rejected"], row["gnc"]["closures_rejected"]), flush=True)
        except P.PgoError as e:
            row["gnc"] = dict(score(s, truth), failed=str(e))
            print("  GNC              FAILED: %s" % e)
        s.close()
        # the null-hypothesis mixture over the same loops
        s, kept, _ = start(g, n, args, 0)
        loops = kept & (kind != 0)
        mk = kind[np.nonzero(loops)[0]]              # (the mixture edges are the selected edges in ascending order)
        s.set_mixture_null(args.pi, args.scale, select=loops)
        if args.kernel:
            row["select_call_ms"] = select_ms(s, 0, args.reps)
        t0 = time.perf_counter()
        try:
            summ, rounds = s.mixture_solve(inner_iters=args.inner, final_iters=args.iters, max_rounds=args.max_rounds)
            sel = s.mixture_selection()
            nb, nc = max(int((mk == 2).sum()), 1), max(int((mk == 1).sum()), 1)
            row["mixture"] = dict(score(s, truth), seconds=time.perf_counter() - t0, rounds=summ["rounds"], hit_max_rounds=summ["hit_max_rounds"],
                                  would_change=summ["n_would_change"], objective=[r["objective"] for r in rounds],
                                  changed=[r["n_changed"] for r in rounds], round_ms=[1e3 * r["seconds"] for r in rounds],
                                  bogus_on_null=int(((mk == 2) & (sel == 1)).sum()), closures_on_null=int(((mk == 1) & (sel == 1)).sum()),
                                  bogus_share=float(((mk == 2) & (sel == 1)).sum() / nb), closures_share=float(((mk == 1) & (sel == 1)).sum() / nc),
                                  final_iterations=summ["final_solve"]["iterations"])
            m = row["mixture"]
            print("  null mixture     %s; %d rounds%s, %.2f s; on the null component: %d of %d bogus (%.1f %%), %d of %d closures (%.3f %%); changed per round %s"
                  % (f(m), m["rounds"], " (max_rounds)" if m["hit_max_rounds"] else "", m["seconds"], m["bogus_on_null"], int((mk == 2).sum()),
                     100.0 * m["bogus_share"], m["closures_on_null"], int((mk == 1).sum()), 100.0 * m["closures_share"], m["changed"]), flush=True)
        except P.PgoError as e:
            row["mixture"] = dict(score(s, truth), failed=str(e))
            print("  null mixture     FAILED: %s" % e)
        if args.kernel:
            row["select_apply_call_ms"] = select_ms(s, 1, args.reps)
            print("  pgo_mixture_select call: measure %s ms, apply %s ms" % (json.dumps(row["select_call_ms"]), json.dumps(row["select_apply_call_ms"])), flush=True)
        s.close()
        rows.append(row)
    line = json.dumps({"mixture_report": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
