"""64 local windows (window_plan([e], 10) around the first 64 loop edges of INTEL + 50, 2 LM iterations each) three ways:
  window   ONE Solver.window_solve call on a live handle
  batch    Batch(the 64 extracted graphs) + solve + close, as before pgo_window_solve
  active   64 x (set_active + solve) on one live handle, as before pgo_window_solve (the pose reset between two windows is
           outside the timed span)
Report only: the median of 10 rounds per way (python window_timing.py MODE, one process per way; run on the GPU box).
DESIGN.md section 4e holds the measured numbers."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toy_robust_backend_slam_amd as P   # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
N_WIN, RADIUS, ITERS, ROUNDS = 64, 10, 2, 10


def main(mode):
    g = P.ReadG2O(os.path.join(DATA, "INTEL.g2o"))
    g.add_random_C(50, 1)
    a = {k: np.array(getattr(g, k)) for k in ("poses", "ia", "ib", "meas", "kind", "info")}
    n, E = len(a["poses"]), len(a["ia"])
    loops = np.nonzero(a["kind"] != 0)[0][:N_WIN]
    wins = [P.window_plan(n, a["ia"], a["ib"], a["kind"], [e], RADIUS) for e in loops]
    times = []
    if mode == "window":
        s = P.Solver(g, P.Options(method=1))
        s.window_solve(wins[:1], max_iters=ITERS)                  # (the first call allocates the staging buffers)
        for _ in range(ROUNDS + 1):
            t = time.perf_counter()
            poses, res = s.window_solve(wins, max_iters=ITERS)
            times.append(time.perf_counter() - t)
        note = f"iterations {sum(r.iterations for r in res)}"
        s.close()
    elif mode == "batch":
        graphs, anchors = [], []
        for p, e, an in wins:
            new = -np.ones(n, np.int64)
            new[p] = np.arange(len(p))
            graphs.append(P.Graph.from_arrays(a["poses"][p], new[a["ia"][e]], new[a["ib"][e]], a["meas"][e], a["kind"][e], a["info"][e]))
            anchors.append(int(new[an]))
        assert len(set(anchors)) == 1                              # (one fixed_pose for the whole batch: the anchor is the first pose)
        for _ in range(ROUNDS + 1):
            t = time.perf_counter()
            b = P.Batch(graphs, P.Options(method=1, max_iters=ITERS, fixed_pose=anchors[0]))
            summ = b.solve()
            b.close()
            times.append(time.perf_counter() - t)
        note = f"iterations {sum(x.iterations for x in summ)}"
    elif mode == "active":
        s = P.Solver(g, P.Options(method=1, max_iters=ITERS))
        masks = []
        for p, e, an in wins:
            m, pc = np.zeros(E, bool), np.zeros(n, bool)
            m[e] = True
            pc[an] = True
            masks.append((m, pc))
        its = 0
        for _ in range(ROUNDS + 1):
            dt, its = 0.0, 0
            for m, pc in masks:
                s.set_poses(a["poses"])                            # (every window starts from the same poses: not timed)
                t = time.perf_counter()
                s.set_active(m, pc)
                its += s.solve().iterations
                dt += time.perf_counter() - t
            times.append(dt)
        note = f"iterations {its}"
        s.close()
    else:
        raise SystemExit("usage: window_timing.py window|batch|active")
    times = times[1:]                                              # (the first round warms the kernels up)
    print(f"{mode:7s}: {N_WIN} windows, {ITERS} LM iterations each: median of {ROUNDS} rounds {1e3 * float(np.median(times)):9.3f} ms "
          f"(min {1e3 * min(times):.3f}, max {1e3 * max(times):.3f}); {note}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "")
