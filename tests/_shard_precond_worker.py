"""Worker of tests/test_gpu_sharded_coarse.py: one rank applies the two-level preconditioner (pgo_debug_precond) after one
LM iteration (run as a subprocess; the same configuration as tests/_shard_worker.py, plus `precond_seed`)."""
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
    comm = P.Comm.shm(cfg["name"], rank, world, 0) if world > 1 else None
    s = P.Solver(g, P.Options(**cfg["options"]), comm, device=0)
    s.lm_begin()
    s.lm_step(1)
    r = np.random.default_rng(cfg["precond_seed"]).standard_normal(3 * g.n_poses)
    z = s.precond(r)   # several ranks: z on this rank's own rows, 0 elsewhere
    np.save(os.path.join(cfg["out"], "z_%d.npy" % rank), z)
    np.save(os.path.join(cfg["out"], "poses_%d.npy" % rank), s.poses())
    json.dump(dict(records=s.iter_records(), info=s.info().as_dict()), open(os.path.join(cfg["out"], "out_%d.json" % rank), "w"))
    s.close()
    if comm:
        comm.close()


if __name__ == "__main__":
    main()
