"""The restatement of the LM loop with pose priors (tests/_prior_restatement.py), checked on the CPU: without priors it is
bitwise _loss_restatement.lm, and with priors it agrees with an independent route that knows no priors at all -- the same
information stated as edges from one extra, constant pose at the origin (anchor edges).

Measured when this was written (INTEL, identity edge information, info_weighting, Huber(0.01) on the edges and on the priors,
from the prior-free 50-iteration solution, 12 priors with noise (0.05 m, 0.05 m, 0.02 rad) and random SPD information; METHOD 0
clean / METHOD 1 + 50 loops): identical accept / reject history over 50 iterations, cost within 5.7e-15 / 7.8e-15 relative,
poses within 1.8e-14 / 2.3e-13, the priors moving the poses by 0.096 m / 0.88 m, the largest heading residual 0.016 / 0.005 rad.
The bounds asserted, 1e-12 on the cost and 1e-9 on the poses, are that spread with room for another BLAS summation order.
Started from the file's poses the two routes differ in the first cost already (the headings of the anchor edges fold with
asin): that is the edge model, not a defect."""
import os

import numpy as np
import pytest

import _loss_restatement as LR
import _prior_restatement as PR
from conftest import DATA

HUBER = ("huber", 0.01)   # the library's default loss, on every edge class and on the priors


def _graph(O, n_out):
    og = O.read_g2o(os.path.join(DATA, "INTEL.g2o"))
    if n_out:
        og = O.add_random_C(og, n_out, 1)
    return og


def test_without_priors_the_restatement_is_the_loss_restatement(oracle):
    og = _graph(oracle, 50)
    cls = LR.classes(og.kind, 1)
    for method in (0, 1):
        a = LR.lm(oracle, og, [HUBER], cls, method=method, max_iters=6)
        b = PR.lm(oracle, og, [HUBER], cls, method=method, max_iters=6)
        assert a.poses.tobytes() == b.poses.tobytes()
        assert (a.termination, a.iterations, a.final_cost, a.initial_cost) == (b.termination, b.iterations, b.final_cost, b.initial_cost)
        assert a.records == b.records


@pytest.mark.parametrize("method,n_out", [(0, 0), (1, 50)])
def test_priors_equal_anchor_edges(oracle, method, n_out):
    og = _graph(oracle, n_out)
    N = og.n_poses
    ident = np.tile(PR.info6(np.eye(3)[None]), (og.n_edges, 1))
    og_i = oracle.Graph(np.array(og.pose_id), np.array(og.poses), np.array(og.ia), np.array(og.ib), np.array(og.meas), ident, np.array(og.kind))
    cls = LR.classes(og_i.kind, 1)
    start = LR.lm(oracle, og_i, [HUBER], cls, method=method, info_weighting=True).poses
    og_a, og_b, pri = PR.anchor_case(oracle, og_i, start)
    # the equivalence needs every heading residual of the anchor edges below pi / 2, at the start and (below) at the end
    assert np.abs(PR.residuals(pri, start)[0][:, 2]).max() < 0.5 * np.pi
    A = LR.lm(oracle, og_a, [HUBER], LR.classes(og_a.kind, 1), method=method, fixed_pose=N, info_weighting=True)
    B = PR.lm(oracle, og_b, [HUBER], cls, priors=pri, prior_loss=HUBER, method=method, fixed_pose=-1, info_weighting=True)
    moved = np.abs(B.poses[:, :2] - start[:, :2]).max()
    worst_cost = max(abs(a["cost"] - b["cost"]) / abs(a["cost"]) for a, b in zip(A.records, B.records))
    worst_pose = np.abs(A.poses[:N] - B.poses).max()
    heading = np.abs(PR.residuals(pri, B.poses)[0][:, 2]).max()
    print(f"METHOD {method} + {n_out}: {B.iterations} iterations, cost diff {worst_cost:.1e}, pose diff {worst_pose:.1e}, "
          f"moved {moved:.2e} m, max heading residual {heading:.2e}")
    assert heading < 0.5 * np.pi
    assert (A.termination, A.iterations) == (B.termination, B.iterations)
    assert [r["step_ok"] for r in A.records] == [r["step_ok"] for r in B.records]
    assert worst_cost <= 1e-12
    assert worst_pose <= 1e-9
    assert np.all(A.poses[N] == 0.0)   # the anchor never moved
    assert moved > 1e-3                # ... and the priors did something


def test_rows_match_the_normal_equation_terms():
    """the two statements of the priors in the restatement -- extra rows for lm(), block terms for the operator test -- agree"""
    rng = np.random.default_rng(3)
    n, N = 7, 20
    B = rng.normal(size=(n, 3, 3))
    info = np.einsum("nij,nkj->nik", B, B)
    info[0] = np.diag([2.0, 2.0, 0.0])
    pri = PR.make(rng.choice(N, n, replace=False), rng.normal(size=(n, 3)), info)
    x, scale = rng.normal(size=(N, 3)), rng.uniform(0.1, 1.0, size=(N, 3))
    for loss in (("trivial", 0.0), ("huber", 0.5), ("cauchy", 0.3), ("tukey", 1.0)):
        c, r, J = PR.rows(pri, loss, x)
        dH, dg, c2 = PR.normal_eq_terms(pri, loss, x, scale)
        assert c == c2
        S = scale[pri["pose"]]
        Js = J * S[:, None, :]
        np.testing.assert_allclose(np.einsum("nki,nkj->nij", Js, Js), dH, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(np.einsum("nki,nk->ni", Js, r.reshape(n, 3)), dg, rtol=1e-12, atol=1e-14)
