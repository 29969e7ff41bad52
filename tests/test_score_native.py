"""csrc/traj_error.h as a program of its own, tests/native/traj_error_main.cpp, built by g++ under ASan + UBSan: the run is
clean and its output is bitwise what the library's host entry point, pgo_trajectory_error_eval, returns (the same statement,
the same serial order)."""
import os

import numpy as np
import pytest

import _native_san as NS

FIELDS_I = ("n_poses", "n_pairs", "ate_max_pose", "rpe_max_pose")
FIELDS_D = ("align_x", "align_y", "align_phi", "ate_rmse", "ate_mean", "ate_max", "rot_rmse", "rot_max", "rpe_trans_rmse",
            "rpe_trans_max", "rpe_rot_rmse", "rpe_rot_max")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("traj_native"), "traj_error_main")


def run_program(exe, tmp, est, ref, mask, align, delta):
    n = len(est)
    src, dst = os.path.join(str(tmp), "in.txt"), os.path.join(str(tmp), "out.txt")
    with open(src, "w") as f:
        f.write("%d %d %d %d\n" % (n, align, delta, mask is not None))
        for i in range(n):
            f.write(" ".join("%.17g" % v for v in (*est[i], *ref[i])) + " %d\n" % (1 if mask is None else int(mask[i])))
    out = NS.run([exe, src, dst])
    assert "traj error ok: %d poses" % n in out
    lines = open(dst).read().split("\n")
    got = {k: int(lines[j]) for j, k in enumerate(FIELDS_I)}
    got.update({k: float(lines[4 + j]) for j, k in enumerate(FIELDS_D)})
    per = np.array([[float(v) for v in line.split()] for line in lines[16:16 + n]])
    return got, per


def test_sanitized_program_is_bitwise_the_library(pgo, exe, tmp_path):
    n, seed = 300, 3
    dead, truth = np.array(pgo.synth_manhattan(n, 4.0, 0.1, seed).poses), pgo.synth_manhattan_truth(n, seed)
    mask = np.random.default_rng(5).random(n) < 0.7
    for m, align, delta in ((None, 0, 1), (None, 1, 10), (mask, 1, 1), (mask, 0, n), (np.zeros(n, bool), 1, 1)):
        got, per = run_program(exe, tmp_path, dead, truth, m, align, delta)
        ref, rper = pgo.trajectory_error(dead, truth, mask=m, align=bool(align), rpe_delta=delta, per_pose=True)
        for k in FIELDS_I:
            assert got[k] == ref[k], (k, got[k], ref[k])
        for k in FIELDS_D:
            assert np.float64(got[k]).tobytes() == np.float64(ref[k]).tobytes(), (k, got[k], ref[k])
        assert per.tobytes() == rper.tobytes()
    assert ref["n_poses"] == 0 and ref["ate_max_pose"] == -1
