"""GPU: the two-level PCG preconditioner (csrc/coarse.hip.h) on sharded solves against the single-rank two-level solve.

Several ranks replicate the coarse problem and distribute only the restriction and the prolongation; the shards are aligned to
the aggregates, so the aggregation is the one-rank aggregation.  Ranks run as processes on one GPU through the shared-memory
communicator (tests/test_gpu_sharded.py), or as one rank through RCCL with the collectives forced on.  Every world-1 vs
world-N comparison sets pose_ordering = 1 on both sides: the aggregates are runs of the internal pose numbering."""
import json
import os

import numpy as np
import pytest

import test_gpu_sharded
from conftest import GOLDEN, ROOT
from test_gpu_sharded import run

pytestmark = pytest.mark.gpu


def _same_history(a_recs, b_recs, rel, pcg_slack=None):
    assert len(a_recs) == len(b_recs)
    for a, b in zip(a_recs, b_recs):
        assert a["step_ok"] == b["step_ok"] and a["cost"] == pytest.approx(b["cost"], rel=rel)
        if pcg_slack is not None:
            assert abs(a["pcg_iters"] - b["pcg_iters"]) <= pcg_slack


def _check_ranks(res, poses, coarse, coarse_rank=None):
    for r in range(len(res)):
        i = res[r]["info"]
        assert i["pcg_coarse_poses"] == coarse and i["pcg_single_reduction"] == 0
        assert i["pcg_coarse_rank"] == (coarse_rank if coarse_rank is not None else res[0]["info"]["pcg_coarse_rank"])
        assert i["pcg_coarse_off_iters"] == res[0]["info"]["pcg_coarse_off_iters"]
        np.testing.assert_array_equal(poses[r], poses[0])
        assert [a["pcg_iters"] for a in res[r]["records"]] == [a["pcg_iters"] for a in res[0]["records"]]


@pytest.mark.parametrize("world", [2, 3])
def test_exact_solve_matches_one_rank_and_fixture(tmp_path, world):
    """M3500 METHOD 1, exact mode (pcg_rtol 1e-10), a full LM run: the bars of test_two_level_preconditioner"""
    cfg = dict(graph="M3500", options=dict(method=1, linear_solver=1, pcg_coarse_poses=16, pcg_max_iters=400000, pose_ordering=1))
    ref, ref_poses = run(1, cfg, tmp_path, tag="ref")
    res, poses = run(world, cfg, tmp_path)
    assert ref[0]["info"]["pcg_coarse_poses"] == 16
    _check_ranks(res, poses, 16, ref[0]["info"]["pcg_coarse_rank"])
    fx = json.load(open(os.path.join(GOLDEN, "lm_M3500_out0_m1.json")))
    fx_poses = np.load(os.path.join(GOLDEN, "lm_M3500_out0_m1_poses.npy"))
    assert [a["step_ok"] for a in res[0]["records"]] == [a["step_ok"] for a in fx["records"]] == [a["step_ok"] for a in ref[0]["records"]]
    assert res[0]["summary"]["final_cost"] == pytest.approx(fx["final_cost"], rel=1e-7)
    assert np.abs(poses[0][:, :2] - fx_poses[:, :2]).max() < 5e-6
    assert all(a["iter"] == 0 or a["pcg_rel_residual"] <= 1e-10 for a in res[0]["records"])
    n_ref, n = ref[0]["summary"]["total_pcg_iters"], res[0]["summary"]["total_pcg_iters"]
    print("M3500 world %d: PCG iterations %d (one rank %d)" % (world, n, n_ref))
    assert abs(n - n_ref) <= 0.03 * n_ref


SYNTH = dict(graph="synth", n_poses=30001, seed=11,
             options=dict(method=1, max_iters=5, pcg_rtol=1e-6, pcg_max_iters=20000, pcg_chain_len=64, pcg_coarse_poses=64,
                          pose_ordering=1, halo_exchange=0))


@pytest.mark.parametrize("world", [2, 4])
def test_fewer_iterations_than_one_level(tmp_path, world):
    ref, ref_poses = run(1, SYNTH, tmp_path, tag="ref")
    two, two_poses = run(world, SYNTH, tmp_path, tag="two")
    one, _ = run(world, dict(SYNTH, options=dict(SYNTH["options"], pcg_coarse_poses=0)), tmp_path, tag="one")
    _check_ranks(two, two_poses, 64, ref[0]["info"]["pcg_coarse_rank"])
    n_one, n_two = one[0]["summary"]["total_pcg_iters"], two[0]["summary"]["total_pcg_iters"]
    print("synthetic 30k world %d: PCG iterations one level %d, two levels %d (one rank %d)"
          % (world, n_one, n_two, ref[0]["summary"]["total_pcg_iters"]))
    assert 3 * n_two <= n_one
    _same_history(two[0]["records"], ref[0]["records"], 1e-8, pcg_slack=2)
    assert np.abs(two_poses[0] - ref_poses[0]).max() < 1e-6


def test_exchange_modes(tmp_path):
    """all-gather of the search direction, point-to-point halo exchange, and the exchange overlapped with the product"""
    out = {}
    for halo, ov in ((0, 0), (1, 0), (1, 1)):
        cfg = dict(SYNTH, options=dict(SYNTH["options"], halo_exchange=halo, halo_overlap=ov))
        res, poses = run(2, cfg, tmp_path, tag="h%do%d" % (halo, ov))
        _check_ranks(res, poses, 64)
        assert res[0]["info"]["halo_exchange"] == halo and res[0]["info"]["halo_overlap"] == ov
        out[(halo, ov)] = (res, poses)
    base = out[(0, 0)]
    for k in ((1, 0), (1, 1)):
        _same_history(out[k][0][0]["records"], base[0][0]["records"], 1e-8, pcg_slack=2)
        assert np.abs(out[k][1][0] - base[1][0]).max() < 1e-6


def test_ranks_that_own_no_rows(tmp_path):
    """65 poses in 24-row shards on 4 ranks (aligned to lcm(8, 8) = 8): rank 3 owns nothing, has no aggregate and no coarse
    block, and still takes part in every collective"""
    cfg = dict(graph="recipe", recipe=[65, 1299, 1.0, 65, False, 1], knobs=dict(shm_timeout_s=20),
               options=dict(method=1, fixed_pose=0, max_iters=3, pcg_rtol=1e-12, pcg_max_iters=100000, linear_solver=1,
                            pcg_chain_len=8, pcg_coarse_poses=8, pose_ordering=1))
    ref, ref_poses = run(1, cfg, tmp_path)
    res, poses = run(4, cfg, tmp_path)
    assert res[3]["info"]["row_lo"] == res[3]["info"]["row_hi"]
    _check_ranks(res, poses, 8, ref[0]["info"]["pcg_coarse_rank"])
    assert [a["step_ok"] for a in res[0]["records"]] == [b["step_ok"] for b in ref[0]["records"]]
    assert res[0]["summary"]["final_cost"] == pytest.approx(ref[0]["summary"]["final_cost"], rel=1e-8, abs=1e-12)
    assert np.abs(poses[0] - ref_poses[0]).max() < 1e-6 * max(1.0, np.abs(ref_poses[0]).max())


@pytest.mark.parametrize("graph,outliers,extra", [("INTEL", 50, dict(method=0)), ("INTEL", 50, dict(method=2)),
                                                  ("M3500", 0, dict(method=1, info_weighting=1, phi=1.0))])
def test_methods_and_information_weighting(tmp_path, graph, outliers, extra):
    cfg = dict(graph=graph, outliers=outliers,
               options=dict(max_iters=5, linear_solver=1, pcg_coarse_poses=16, pcg_max_iters=400000, pose_ordering=1, **extra))
    ref, ref_poses = run(1, cfg, tmp_path, tag="ref")
    res, poses = run(2, cfg, tmp_path)
    assert ref[0]["info"]["pcg_coarse_poses"] == 16
    _check_ranks(res, poses, 16, ref[0]["info"]["pcg_coarse_rank"])
    _same_history(res[0]["records"], ref[0]["records"], 1e-8)


def test_rccl_single_rank_in_a_captured_graph(tmp_path):
    """world 1 through RCCL with the collectives forced on: the new all-reduce (r_c with the r.z / r.r sums) is recorded into
    the PCG hipGraph and replayed; the eager loop (PGO_GRAPH_COLLECTIVES=0) gives the same poses"""
    base = dict(graph="synth", n_poses=60001, seed=4,
                options=dict(method=1, max_iters=3, pcg_rtol=1e-6, pcg_max_iters=20000, pcg_coarse_poses=64, pose_ordering=1))
    ref, ref_poses = run(1, base, tmp_path, tag="ref")
    res, poses = run(1, dict(base, comm="rccl"), tmp_path, env={"PGO_FORCE_COLLECTIVES": "1"}, tag="rccl")
    eager, eager_poses = run(1, dict(base, comm="rccl"), tmp_path, env={"PGO_FORCE_COLLECTIVES": "1", "PGO_GRAPH_COLLECTIVES": "0"},
                             tag="eager")
    i = res[0]["info"]
    assert i["pcg_coarse_poses"] == 64 and i["pcg_graph_replay"] == 1 and i["pcg_single_reduction"] == 0
    assert eager[0]["info"]["pcg_coarse_poses"] == 64 and eager[0]["info"]["pcg_graph_replay"] == 0
    _same_history(res[0]["records"], ref[0]["records"], 1e-8, pcg_slack=2)
    assert np.abs(poses[0] - ref_poses[0]).max() < 1e-6
    assert np.abs(eager_poses[0] - poses[0]).max() <= 1e-12 * max(1.0, np.abs(poses[0]).max())


def test_preconditioner_apply_matches_one_rank(tmp_path, monkeypatch):
    """pgo_debug_precond on two ranks: every rank returns M^-1 r on its own rows; together they are the one-rank M^-1 r"""
    monkeypatch.setattr(test_gpu_sharded, "WORKER", os.path.join(ROOT, "tests", "_shard_precond_worker.py"))
    cfg = dict(graph="M3500", precond_seed=7,
               options=dict(method=1, linear_solver=1, pcg_coarse_poses=16, pcg_max_iters=400000, pose_ordering=1))
    run(1, cfg, tmp_path, tag="ref")
    run(2, cfg, tmp_path)
    z1 = np.load(os.path.join(str(tmp_path), "w1ref", "z_0.npy"))
    zs = [np.load(os.path.join(str(tmp_path), "w2", "z_%d.npy" % r)) for r in range(2)]
    assert all(np.count_nonzero(z) > 0 for z in zs)
    assert np.count_nonzero(zs[0] * zs[1]) == 0   # disjoint rows
    z2 = zs[0] + zs[1]
    rel = np.linalg.norm(z2 - z1) / np.linalg.norm(z1)
    print("M^-1 r, two ranks against one: relative difference %.2e" % rel)
    assert rel <= 1e-12


def test_auto_stays_one_level_on_several_ranks(tmp_path):
    """the default (auto) does not enable the second level at world > 1"""
    cfg = dict(graph="M3500", options=dict(method=1, max_iters=1, pcg_rtol=1e-10, pcg_max_iters=400000))
    res, _ = run(2, cfg, tmp_path)
    for r in range(2):
        assert res[r]["info"]["pcg_coarse_poses"] == 0 and res[r]["info"]["pcg_coarse_rank"] == 0
