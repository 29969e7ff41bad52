#!/usr/bin/env python3
"""What carrying the information matrices through the coarse graph is worth, at scale.

synth_manhattan(n, 4.0, 0.10, seed) at n = 10k / 100k / 1M, strides 16 and 64, two fine informations -- unit, and the generator's
true noise diag(1 / 0.02^2, 1 / 0.02^2, 1 / 0.01^2) --, three coarse solves: METHOD 0 after loop_support(apply=True), and METHOD 1
with phi 0.5 and phi 5.  Per case the ATE rmse (unaligned and aligned) of the prolonged start with unit coarse information
(pgo_coarsen) and with the propagated one (pgo_coarsen_info, info_weighting = 1), the coarse solve's iterations and time, and
the times of pgo_coarsen_info against pgo_coarsen (each handle's first call, then the median of 9) and against the serial
pgo_coarsen_info_plan (median of 3).  One JSON line at the end.
Needs a GPU.

    python scripts/init_info_report.py [--sizes 10000,100000,1000000] [--strides 16,64] [--coarse-iters 50] [--seed 20260410]
                                       [--cases m0,m1phi0.5,m1phi5] [--out FILE.json]
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

CASES = {"m0": (0, None), "m1phi0.5": (1, 0.5), "m1phi5": (1, 5.0)}


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def median_of(f, reps=9):
    """median wall time of `reps` calls"""
    return float(np.median([timed(f)[1] for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--strides", default="16,64")
    ap.add_argument("--cases", default="m0,m1phi0.5,m1phi5")
    ap.add_argument("--coarse-iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=20260410)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows, times = [], []
    for n in [int(v) for v in args.sizes.split(",")]:
        g0 = P.synth_manhattan(n, 4.0, 0.10, args.seed)
        truth = P.synth_manhattan_truth(n, args.seed)
        poses, ia, ib, meas, kind = np.array(g0.poses), np.array(g0.ia), np.array(g0.ib), np.array(g0.meas), np.array(g0.kind)
        E = len(ia)
        fine = {"unit": np.tile([1.0, 0, 0, 1, 0, 1], (E, 1)), "noise": np.tile([2500.0, 0, 0, 2500.0, 0, 10000.0], (E, 1))}
        for fname, info in fine.items():
            g = P.Graph.from_arrays(poses, ia, ib, meas, kind, info=info)
            for stride in [int(v) for v in args.strides.split(",")]:
                if fname == "unit":   # the transfer operator alone: the first call of each (tables; information check), then medians of 9
                    s = P.Solver(g, P.Options(method=0))
                    _, t_first = timed(lambda: s.coarsen(stride))
                    _, t_first_info = timed(lambda: s.coarsen(stride, information=True))
                    t_plain = median_of(lambda: s.coarsen(stride))
                    t_info = median_of(lambda: s.coarsen(stride, information=True))
                    s.close()
                    t_plan = median_of(lambda: P.coarsen_info_plan(n, ia, ib, meas, kind, stride, info), 3)
                    times.append({"n": n, "stride": stride, "coarsen_first_s": t_first, "coarsen_info_first_s": t_first_info,
                                  "coarsen_s": t_plain, "coarsen_info_s": t_info, "plan_s": t_plan})
                    print(json.dumps(times[-1]), flush=True)
                for case in args.cases.split(","):
                    method, phi = CASES[case]
                    for information in (False, True):
                        if fname == "noise" and not information:
                            continue   # (pgo_coarsen reads no information: the unit row)
                        s = P.Solver(g, P.Options(method=method))
                        if method == 0:
                            s.loop_support(apply=True)
                        f = int(s.options.fixed_pose)
                        o = P.Options(method=method, pcg_rtol=1e-10, max_iters=args.coarse_iters, info_weighting=int(information),
                                      fixed_pose=(f if f < 0 else (f // stride if f % stride == 0 else 0)))
                        if phi is not None:
                            o.phi = phi
                        summ, t = timed(lambda: s.initialize_hierarchical(stride, coarse_options=o, carry_weights=(method == 0),
                                                                          information=information))
                        row = {"n": n, "fine_info": fname, "stride": stride, "case": case, "propagated": information,
                               "ate": s.trajectory_error(truth)["ate_rmse"], "ate_aligned": s.trajectory_error(truth, align=True)["ate_rmse"],
                               "coarse_iterations": summ.iterations, "termination": P.TERMINATION.get(summ.termination, "?"), "seconds": t}
                        s.close()
                        rows.append(row)
                        print(json.dumps(row), flush=True)
    out = json.dumps({"rows": rows, "times": times})
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
