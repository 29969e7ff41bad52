// Pose priors through the C++ mirror of the reference interface: the reference's METHOD 1 problem (main.cpp:95-153) under
// HuberLoss(0.01), plus one PosePriorResidue per line of PRIORS ("EDGE_PRIOR_SE2 id x y th I11 I12 I13 I22 I23 I33", id = the
// vertex id) under ceres::CauchyLoss(A).  MODE solve: pgo::Solve; gnc: pgo::SolveGnc (METHOD 0 blocks); batch: pgo::SolveBatch
// of the problem twice -- problems with priors go to the thread pool.  Writes the optimised poses (node order, 17 digits) to OUT.
// Built and run by tests/test_gpu_priors_mirror.py (needs a GPU).
//     prior_mirror_main G2O PRIORS OUT A MODE
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "ceres_error.h"
#include "g2o_util.h"
#include "pgo_problem.h"

static void build(ReadG2O& g2o, pgo::Problem& problem, pgo::LossFunction* huber, pgo::LossFunction* cauchy, const char* priors, bool dcs) {
  for (Edge* ed : g2o.nEdgesOdometry)
    problem.AddResidualBlock(OdometryResidue::Create(ed->x, ed->y, ed->theta), huber, ed->a->p, ed->b->p);
  for (auto* list : {&g2o.nEdgesClosure, &g2o.nEdgesBogus})
    for (Edge* ed : *list)
      problem.AddResidualBlock(dcs ? DCSClosureResidue::Create(ed->x, ed->y, ed->theta) : OdometryResidue::Create(ed->x, ed->y, ed->theta), huber,
                               ed->a->p, ed->b->p);
  problem.SetParameterBlockConstant(g2o.nNodes[0]->p);
  std::ifstream in(priors);
  std::unordered_map<int, Node*> by_id;   // vertex id -> node
  for (Node* nd : g2o.nNodes) by_id[nd->index] = nd;
  std::string tag;
  int id;
  double z[3], w[6];
  while (in >> tag >> id >> z[0] >> z[1] >> z[2] >> w[0] >> w[1] >> w[2] >> w[3] >> w[4] >> w[5]) {
    const auto found = by_id.find(id);
    Node* at = found == by_id.end() ? nullptr : found->second;
    if (!at || tag != "EDGE_PRIOR_SE2") exit(4);
    problem.AddResidualBlock(PosePriorResidue::Create(z[0], z[1], z[2], w), cauchy, at->p);
  }
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  const std::string mode = argv[5];
  std::unique_ptr<pgo::LossFunction> huber(new pgo::HuberLoss(0.01)), cauchy(new pgo::CauchyLoss(atof(argv[4])));
  pgo::Solver::Options options;
  options.linear_solver_type = pgo::SPARSE_NORMAL_CHOLESKY;
  ReadG2O g2o(argv[1]);
  g2o.add_random_C(50, 1);
  pgo::Problem problem;
  build(g2o, problem, huber.get(), cauchy.get(), argv[2], mode == "solve" || mode == "batch");
  int iterations = 0;
  if (mode == "solve") {
    pgo::Solver::Summary summary;
    pgo::Solve(options, &problem, &summary);
    iterations = summary.s.iterations;
  } else if (mode == "gnc") {
    pgo::GncOptions gnc;
    gnc.cbar = 0.5;
    gnc.max_rounds = 4;
    gnc.final_iterations = 5;
    gnc.select.assign((size_t)problem.NumResidualBlocks(), 1);
    for (size_t e = 0; e < g2o.nEdgesOdometry.size(); ++e) gnc.select[e] = 0;
    pgo::GncSummary gs;
    pgo::SolveGnc(options, gnc, &problem, &gs);
    iterations = gs.final_solve.s.iterations;
  } else if (mode == "batch") {
    ReadG2O twin(argv[1]);
    twin.add_random_C(50, 1);
    pgo::Problem second;
    build(twin, second, huber.get(), cauchy.get(), argv[2], true);
    std::vector<pgo::Solver::Summary> sums;
    pgo::SolveBatch(options, {&problem, &second}, &sums);
    for (size_t k = 0; k < g2o.nNodes.size(); ++k)
      if (memcmp(g2o.nNodes[k]->p, twin.nNodes[k]->p, 3 * sizeof(double)) != 0) return 5;   // the same problem twice: the same bits
    iterations = sums[1].s.iterations;
  } else {
    return 2;
  }
  double d[3];
  PosePriorResidue(0.0, 0.0, 3.1)(g2o.nNodes[0]->p, d);   // the functor stays host-callable
  FILE* f = fopen(argv[3], "w");
  if (!f) return 1;
  for (Node* nd : g2o.nNodes) fprintf(f, "%.17g %.17g %.17g\n", nd->p[0], nd->p[1], nd->p[2]);
  fclose(f);
  printf("prior mirror ok: %s, %d pose priors, %d iterations\n", mode.c_str(), problem.NumPosePriors(), iterations);
  return 0;
}
