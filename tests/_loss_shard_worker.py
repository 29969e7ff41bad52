"""Worker of tests/test_gpu_loss.py: one rank of a sharded solve with per-edge loss classes (run as a subprocess)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import toy_robust_backend_slam_amd as P  # noqa: E402


def main():
    cfg = json.loads(sys.argv[1])
    rank, world = cfg["rank"], cfg["world"]
    g = P.ReadG2O(os.path.join(ROOT, "tests", "golden", "data", cfg["graph"] + ".g2o"))
    if cfg.get("outliers"):
        g.add_random_C(cfg["outliers"], 1)
    comm = P.Comm.shm(cfg["name"], rank, world, 0) if world > 1 else None
    losses = [P.Loss(n, a) for n, a in cfg["losses"]]
    edge_class = np.arange(g.n_edges) % len(losses)    # every rank passes the same classes in the caller's edge order
    s = P.Solver(g, P.Options(**cfg["options"]), comm, device=0, losses=losses, edge_class=edge_class)
    c0, _, _ = s.evaluate(want_r=False, want_J=False)
    summ = s.solve()
    out = dict(cost0=c0, summary=summ.as_dict(), records=s.iter_records())
    np.save(os.path.join(cfg["out"], "poses_%d.npy" % rank), s.poses())
    json.dump(out, open(os.path.join(cfg["out"], "out_%d.json" % rank), "w"))
    s.close()
    if comm:
        comm.close()


if __name__ == "__main__":
    main()
