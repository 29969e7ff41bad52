// pgo::InitializeHierarchical(..., information = true) on a pgo::Problem with residual block weights, through the C++ mirror:
// 0 / 1 weights go to the coarse handle as pgo_set_active -- the prolonged start must be the one of the same problem with the
// weight-0 blocks left out: two exact-mode solves of one problem that differ in the order of their sums, so within the
// pose-parity bound of the golden LM tests, 5e-6, times 1 + L (L = the longest segment path, which a coarse heading error
// turns) --, and a weight that is neither throws std::invalid_argument and moves no block.
// Built and run by tests/test_gpu_coarsen_info.py::test_host_mirror_with_weights (needs a GPU).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "ceres_error.h"
#include "g2o_util.h"
#include "pgo_problem.h"

static int fail(const char* what) {
  fprintf(stderr, "init info mirror: %s (%s)\n", what, pgo_last_error());
  return 1;
}

// the problem of the g2o file with every loop whose index is in `drop` (a) weighted 0, or (b) left out
static void build(ReadG2O& g2o, std::vector<double*>& poses, pgo::LossFunction* loss, bool leave_out, int stride_of_drops, double weight,
                  pgo::Problem* problem) {
  for (double* p : poses) problem->AddParameterBlock(p, 3);
  std::vector<double> w;
  for (auto* ed : g2o.nEdgesOdometry) {
    problem->AddResidualBlock(OdometryResidue::Create(ed->x, ed->y, ed->theta), loss, poses[ed->a->index], poses[ed->b->index]);
    w.push_back(1.0);
  }
  int k = 0;
  for (auto* ed : g2o.nEdgesClosure) {
    const bool dropped = (k++ % stride_of_drops) == 0;
    if (dropped && leave_out) continue;
    problem->AddResidualBlock(OdometryResidue::Create(ed->x, ed->y, ed->theta), loss, poses[ed->a->index], poses[ed->b->index]);
    w.push_back(dropped ? weight : 1.0);
  }
  problem->SetParameterBlockConstant(poses[0]);
  if (!leave_out) problem->SetResidualBlockWeights(w);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  ReadG2O g2o(argv[1]);
  std::vector<double> start;
  for (auto* nd : g2o.nNodes) start.insert(start.end(), nd->p, nd->p + 3);
  const size_t N = g2o.nNodes.size();
  pgo::LossFunction* loss = new pgo::HuberLoss(0.01);
  auto fresh = [&](std::vector<double*>* poses) {
    poses->clear();
    for (size_t i = 0; i < N; ++i) poses->push_back(new double[3]{start[3 * i], start[3 * i + 1], start[3 * i + 2]});
  };
  std::vector<double*> pa, pb, pc;
  fresh(&pa), fresh(&pb), fresh(&pc);
  pgo::Solver::Options options;
  pgo::Solver::Summary sa, sb;
  {
    pgo::Problem weighted, without;
    build(g2o, pa, loss, false, 3, 0.0, &weighted);
    build(g2o, pb, loss, true, 3, 0.0, &without);
    pgo::InitializeHierarchical(&weighted, 16, options, &sa, true);
    pgo::InitializeHierarchical(&without, 16, options, &sb, true);
  }
  if (sa.num_residual_blocks <= sb.num_residual_blocks) return fail("the weighted coarse graph should list the dropped blocks");
  // (both coarse solves stop on the function tolerance, 1e-6 relative)
  if (std::fabs(sa.s.final_cost - sb.s.final_cost) > 1e-6 * sb.s.final_cost) return fail("coarse solves differ");
  std::vector<double> seg((N + 15) / 16, 0.0);
  for (auto* ed : g2o.nEdgesOdometry) seg[(size_t)std::min(ed->a->index, ed->b->index) / 16] += std::hypot(ed->x, ed->y);
  double L = 0.0, worst = 0.0;
  for (double v : seg) L = std::max(L, v);
  bool moved = false;
  for (size_t i = 0; i < N; ++i) {
    for (int k = 0; k < 3; ++k) worst = std::max(worst, std::fabs(pa[i][k] - pb[i][k]));
    moved = moved || memcmp(pa[i], &start[3 * i], 3 * sizeof(double)) != 0;
  }
  printf("prolonged starts: max difference %.3e (bound %.3e)\n", worst, 5e-6 * (1.0 + L));
  if (!(worst <= 5e-6 * (1.0 + L))) return fail("prolonged starts differ");
  if (!moved) return fail("no block moved");
  bool thrown = false;
  {
    pgo::Problem half;
    build(g2o, pc, loss, false, 3, 0.5, &half);
    try {
      pgo::InitializeHierarchical(&half, 16, options, nullptr, true);
    } catch (const std::invalid_argument&) {
      thrown = true;
    }
  }
  if (!thrown) return fail("a weight of 0.5 was accepted");
  for (size_t i = 0; i < N; ++i)
    if (memcmp(pc[i], &start[3 * i], 3 * sizeof(double)) != 0) return fail("a refused call moved a block");
  printf("coarse graph %d blocks (%d without the dropped ones), cost %.6f -> %.6f in %d iterations\n", sa.num_residual_blocks,
         sb.num_residual_blocks, sa.s.initial_cost, sa.s.final_cost, sa.s.iterations);
  printf("init info mirror ok\n");
  return 0;
}
