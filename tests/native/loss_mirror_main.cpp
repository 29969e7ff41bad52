// Robust losses through the C++ mirror of the reference interface: the reference's METHOD 1 problem (main.cpp:95-153)
// with ceres::CauchyLoss(a) on the closure and bogus blocks and a NULL loss on the odometry blocks, i.e. two loss classes.
// Writes the optimised poses (node order, 17 digits) to OUT.  Built and run by tests/test_gpu_loss.py (needs a GPU).
//     loss_mirror_main G2O OUT A
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "ceres_error.h"
#include "g2o_util.h"
#include "pgo_problem.h"

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  ReadG2O g2o(argv[1]);
  g2o.add_random_C(50, 1);
  std::unique_ptr<pgo::LossFunction> cauchy(new pgo::CauchyLoss(atof(argv[3])));
  pgo::Problem problem;
  for (Edge* ed : g2o.nEdgesOdometry)
    problem.AddResidualBlock(OdometryResidue::Create(ed->x, ed->y, ed->theta), nullptr, ed->a->p, ed->b->p);
  for (auto* list : {&g2o.nEdgesClosure, &g2o.nEdgesBogus})
    for (Edge* ed : *list) problem.AddResidualBlock(DCSClosureResidue::Create(ed->x, ed->y, ed->theta), cauchy.get(), ed->a->p, ed->b->p);
  problem.SetParameterBlockConstant(g2o.nNodes[0]->p);
  pgo::Solver::Options options;
  options.linear_solver_type = pgo::SPARSE_NORMAL_CHOLESKY;
  pgo::Solver::Summary summary;
  pgo::Solve(options, &problem, &summary);
  double rho[3];
  cauchy->Evaluate(4.0, rho);   // LossFunction::Evaluate on the host
  FILE* f = fopen(argv[2], "w");
  if (!f) return 1;
  for (Node* nd : g2o.nNodes) fprintf(f, "%.17g %.17g %.17g\n", nd->p[0], nd->p[1], nd->p[2]);
  fclose(f);
  printf("loss mirror ok: %d iterations, final cost %.17g, rho(4) = %.17g %.17g %.17g\n", summary.s.iterations,
         summary.s.final_cost, rho[0], rho[1], rho[2]);
  return 0;
}
