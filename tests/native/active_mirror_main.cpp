// pgo::Problem with several constant parameter blocks and a block that no residual block uses, through the C++ mirror of the
// reference interface: every SetParameterBlockConstant call counts (main.cpp:153 makes one; the layer managers' windows more),
// and an unused block is constant as it would be outside Ceres' reduced program.  Checked against the C-ABI used directly:
// pgo_create + pgo_set_active on the same arrays must give the same poses bit for bit.
// Built and run by tests/test_gpu_active.py::test_host_active_mirror (needs a GPU).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ceres_error.h"
#include "g2o_util.h"
#include "pgo_problem.h"

static int fail(const char* what) {
  fprintf(stderr, "active mirror: %s (%s)\n", what, pgo_last_error());
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  ReadG2O g2o(argv[1]);
  const int N = (int)g2o.nNodes.size();
  const int extra = N;                       // one more pose block that no residual block uses
  const int also_constant = 600;
  std::vector<double*> poses;
  for (auto* nd : g2o.nNodes) poses.push_back(new double[3]{nd->p[0], nd->p[1], nd->p[2]});
  poses.push_back(new double[3]{7.0, -3.0, 0.25});
  std::vector<double> start;
  for (double* p : poses) start.insert(start.end(), p, p + 3);

  pgo::Problem problem;
  pgo::LossFunction* loss = new pgo::HuberLoss(0.01);
  for (double* p : poses) problem.AddParameterBlock(p, 3);   // block k = pose k
  std::vector<int32_t> ia, ib;
  std::vector<double> meas;
  for (auto* list : {&g2o.nEdgesOdometry, &g2o.nEdgesClosure})
    for (auto* ed : *list) {
      problem.AddResidualBlock(OdometryResidue::Create(ed->x, ed->y, ed->theta), loss, poses[ed->a->index], poses[ed->b->index]);
      ia.push_back(ed->a->index);
      ib.push_back(ed->b->index);
      meas.insert(meas.end(), {ed->x, ed->y, ed->theta});
    }
  problem.SetParameterBlockConstant(poses[0]);
  problem.SetParameterBlockConstant(poses[also_constant]);
  problem.SetParameterBlockConstant(poses[0]);               // (again: no effect)
  if (problem.NumParameterBlocks() != N + 1) return fail("parameter block count");

  pgo::Solver::Options options;
  options.max_num_iterations = 3;
  pgo::Solver::Summary summary;
  pgo::Solve(options, &problem, &summary);
  if (!(summary.s.final_cost < summary.s.initial_cost) || summary.s.iterations != 3) return fail("the solve made no progress");
  for (int k : {0, also_constant, extra})
    if (memcmp(poses[k], &start[3 * (size_t)k], 3 * sizeof(double)) != 0) return fail("a constant block moved");
  if (memcmp(poses[1], &start[3], 3 * sizeof(double)) == 0) return fail("a free block did not move");

  // the same problem through the C-ABI
  pgo_options o;
  pgo_options_default(&o);
  o.method = 0;
  o.fixed_pose = 0;
  o.max_iters = options.max_num_iterations;
  o.pcg_rtol = options.pcg_rtol;
  o.pcg_max_iters = options.pcg_max_iters;
  std::vector<uint8_t> kind(ia.size(), PGO_EDGE_ODOMETRY), cls(ia.size(), 0), constant((size_t)N + 1, 0);
  constant[0] = constant[also_constant] = 1;
  pgo_t* h = nullptr;
  if (pgo_create(&h, N + 1, start.data(), (int32_t)ia.size(), ia.data(), ib.data(), meas.data(), kind.data(), &o, nullptr, 0) != PGO_OK)
    return fail("pgo_create");
  const pgo_loss huber = pgo::HuberLoss(0.01).loss();
  if (pgo_set_losses(h, 1, &huber, cls.data()) != PGO_OK) return fail("pgo_set_losses");
  if (pgo_set_active(h, nullptr, constant.data()) != PGO_OK) return fail("pgo_set_active");
  pgo_handle_info info;
  if (pgo_get_info(h, &info) != PGO_OK || info.n_active_edges != (int32_t)ia.size() || info.n_constant_poses != 3)
    return fail("pgo_get_info: resolved sets");
  pgo_summary s;
  if (pgo_solve(h, &s) != PGO_OK) return fail("pgo_solve");
  std::vector<double> x(start.size());
  if (pgo_get_poses(h, x.data()) != PGO_OK) return fail("pgo_get_poses");
  pgo_destroy(h);
  if (s.final_cost != summary.s.final_cost || s.iterations != summary.s.iterations) return fail("summaries differ");
  for (int k = 0; k <= N; ++k)
    if (memcmp(poses[k], &x[3 * (size_t)k], 3 * sizeof(double)) != 0) return fail("poses differ from pgo_set_active's");

  printf("constant blocks 0, %d and the unused block %d stayed; cost %.6f -> %.6f in %d iterations\n", also_constant, extra,
         summary.s.initial_cost, summary.s.final_cost, summary.s.iterations);
  printf("active mirror ok\n");
  return 0;
}
