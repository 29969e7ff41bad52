"""The second preconditioner level (csrc/coarse.hip.h) on sharded solves (GPU box).

1. PCG iterations, one level against two, at world 1 / 2 / 4 through the shared-memory test communicator (ranks are processes
   on one GPU): synthetic 100k poses, pcg_rtol 1e-6, 5 LM iterations, pose_ordering = 1, 64-pose aggregates.  The shared-
   memory collectives are host-staged: their timings say nothing about xGMI, so only the counts are reported.
2. GN it/s with and without the level at world 1 through RCCL with PGO_FORCE_COLLECTIVES=1 (the collective path: the larger
   all-reduce and the replicated coarse solve after it, captured into the PCG hipGraph), next to the plain world-1 solve.
Multi-GPU speed is not measured here (one GPU).
usage: exp_shard_coarse.py [n_poses]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_shard_worker.py")
_RUNS = [0]


def run(world, cfg, env=None):
    out = tempfile.mkdtemp(prefix="exp_shard_coarse_")
    _RUNS[0] += 1
    name = "pgo_exp_%d_%d" % (os.getpid(), _RUNS[0])   # (a fresh shared-memory segment per run)
    procs = [subprocess.Popen([sys.executable, WORKER, json.dumps(dict(cfg, rank=r, world=world, name=name, out=out))],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, **(env or {})))
             for r in range(world)]
    logs = [p.communicate(timeout=600)[0] for p in procs]
    if any(p.returncode != 0 for p in procs):
        raise SystemExit("\n".join("rank %d exit %s:\n%s" % (r, p.returncode, logs[r][-2000:]) for r, p in enumerate(procs)))
    return json.load(open(os.path.join(out, "out_0.json")))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    opts = dict(method=1, max_iters=5, pcg_rtol=1e-6, pcg_max_iters=60000, pose_ordering=1)
    base = dict(graph="synth", n_poses=n, seed=20260410)
    print("synthetic %d poses, pcg_rtol 1e-6, 5 LM iterations: total PCG iterations (shared-memory communicator)" % n)
    print("| world | one level | two levels (A = 64) | ratio |")
    print("|---|---|---|---|")
    for world in (1, 2, 4):
        its = []
        for a in (0, 64):
            o = run(world, dict(base, options=dict(opts, pcg_coarse_poses=a)))
            assert o["info"]["pcg_coarse_poses"] == a, o["info"]
            its.append(o["summary"]["total_pcg_iters"])
        print("| %d | %d | %d | %.1f x |" % (world, its[0], its[1], its[0] / max(1, its[1])), flush=True)
    print("\nworld 1, GN it/s (iterations / seconds_total of the solve, handle creation excluded)")
    print("| communicator | one level | two levels (A = 64) | PCG iterations one / two |")
    print("|---|---|---|---|")
    for tag, extra, env in (("none (plain one-rank path)", {}, None),
                            ("RCCL, PGO_FORCE_COLLECTIVES=1", dict(comm="rccl"), {"PGO_FORCE_COLLECTIVES": "1"})):
        row = []
        for a in (0, 64):
            o = run(1, dict(base, options=dict(opts, pcg_coarse_poses=a), **extra), env)
            s = o["summary"]
            row.append((s["iterations"] / s["seconds_total"], s["total_pcg_iters"], o["info"]["pcg_graph_replay"]))
        print("| %s | %.1f | %.1f | %d / %d (graph replay %d / %d) |"
              % (tag, row[0][0], row[1][0], row[0][1], row[1][1], row[0][2], row[1][2]), flush=True)


if __name__ == "__main__":
    main()
