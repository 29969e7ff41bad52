// Command-line front end with the reference's run contract (DCS-ceres/main.cpp:22-40, do_build.sh:10):
//     ./main DATASET NUM_OUTLIER_LOOPS METHOD [--seed S] [--data DIR] [--save DIR] [--device D] [--precision P]
//            [--loss NAME[:A]] [--loop-loss NAME[:A]] [--score FILE [--align]] [--init-stride S [--init-info]] [--gnc CBAR [--gnc-inner K]]
//            [--loop-support MIN[:WINDOW[:TOL_XY[:TOL_TH]]]]
//            [--chordal-init [ROUNDS[:REJECT_XY[:REJECT_TH]]]] [--mixture-null PI:SCALE[:INNER]]
//            [--priors FILE [--prior-loss NAME[:A]]] [--sample-cov S[:SEED]]
// METHOD 0 = baseline, 1 = DCS, 2 = switchable constraints run on the MI355X backend; 3/4 are outside it (exit code 3).
// Reads DIR/DATASET.g2o (default ../data, as the reference), writes init_/opt_ nodes+edges text files that
// drawer/plot_results.py consumes (default ../save; unlike the reference the directory is created).
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <unordered_map>
#include <vector>

#include "ceres_error.h"
#include "g2o_util.h"
#include "graph.h"
#include "pgo_problem.h"

// --loss / --loop-loss NAME[:A]: trivial, huber, softlone, cauchy, arctan, tukey; A defaults to main.cpp:68's 0.01
static std::unique_ptr<pgo::LossFunction> make_loss(const std::string& spec) {
  const size_t colon = spec.find(':');
  const std::string name = spec.substr(0, colon);
  const double a = colon == std::string::npos ? 0.01 : std::stod(spec.substr(colon + 1));
  std::unique_ptr<pgo::LossFunction> l;
  if (name == "trivial") l.reset(new pgo::TrivialLoss());
  else if (name == "huber") l.reset(new pgo::HuberLoss(a));
  else if (name == "softlone") l.reset(new pgo::SoftLOneLoss(a));
  else if (name == "cauchy") l.reset(new pgo::CauchyLoss(a));
  else if (name == "arctan") l.reset(new pgo::ArctanLoss(a));
  else if (name == "tukey") l.reset(new pgo::TukeyLoss(a));
  else throw std::invalid_argument("unknown loss " + name + " (trivial, huber, softlone, cauchy, arctan, tukey)");
  double rho[3];
  l->Evaluate(0.0, rho);   // checks the scale
  return l;
}

int main(int argc, char* argv[]) {
  if (argc < 4) {
    std::cout << "Usage: " << argv[0] << " DATASET NUM_OUTLIER_LOOPS METHOD [--seed S] [--data DIR] [--save DIR] [--device D]\n"
              << "       [--precision P] [--loss NAME[:A]] [--loop-loss NAME[:A]]  (losses: trivial huber softlone cauchy arctan tukey;\n"
              << "       --loss sets every block's, default huber:0.01; --loop-loss overrides it on closure and bogus blocks)\n"
              << "       [--score FILE [--align]]  (FILE: reference poses as writePoseGraph_nodes writes them, <index> <x> <y> <theta>; prints\n"
              << "       the trajectory error of the result against it, --align after a rigid fit; a wrong pose count: exit code 2)\n"
              << "       [--init-stride S]  (2..256: start the solve from the prolonged solution of the graph coarsened at stride S)\n"
              << "       [--init-info]  (with --init-stride: the coarse graph carries information matrices propagated along the odometry chain --\n"
              << "       unit fine information -- and is solved with info_weighting = 1; without --init-stride: exit code 2)\n"
              << "       [--gnc CBAR [--gnc-inner K]]  (METHOD 0 only: graduated non-convexity with the TLS surrogate over the closure and bogus\n"
              << "       blocks, CBAR = the residual norm above which a block is an outlier, K LM iterations per round, default 5; prints the\n"
              << "       rounds and writes weights.txt, one weight per edge in the order of the edges files)\n"
              << "       [--chordal-init [ROUNDS[:REJECT_XY[:REJECT_TH]]]]  (after --loop-support, before --init-stride: start from the linear\n"
              << "       relaxation -- chordal rotations, then positions --; ROUNDS > 0 drops the blocks whose residual exceeds REJECT_XY metres\n"
              << "       or REJECT_TH radians and solves again (METHOD 0 and 1: they stay dropped))\n"
              << "       [--loop-support MIN[:WINDOW[:TOL_XY[:TOL_TH]]]]  (METHOD 0 and 1: before anything else, judge the closure and bogus blocks\n"
              << "       by odometry cycle consistency and drop -- weight 0 -- those with fewer than MIN consistent neighbours within WINDOW\n"
              << "       poses, default 32; tolerances per sqrt(step), default 0.1 m and 0.05 rad: fit them to the dataset's odometry;\n"
              << "       --init-stride and --gnc then run without the dropped blocks; writes weights.txt)\n"
              << "       [--mixture-null PI:SCALE[:INNER]]  (METHOD 0 only: max-mixtures -- every closure and bogus block gets a null hypothesis\n"
              << "       beside its measurement, relative weight PI and information scale SCALE in (0, 1]; rounds of selection and INNER LM\n"
              << "       iterations, default 2, until the selection stands.  The loop blocks run under the Trivial loss unless --loop-loss is\n"
              << "       given: the null component wins where 1/2 rho(s) exceeds its constant -log PI - 1.5 log SCALE, and under the default\n"
              << "       huber:0.01 rho grows like 0.02 |e|, so that it would win only kilometres out.  Writes weights.txt)\n"
              << "       [--priors FILE [--prior-loss NAME[:A]]]  (METHOD 0 and 1: absolute pose priors, one g2o-format line each,\n"
              << "       EDGE_PRIOR_SE2 id x y th I11 I12 I13 I22 I23 I33 -- id a vertex id of the dataset, the information positive SEMI-definite\n"
              << "       (a 0 0 a 0 0 is a position-only fix); --prior-loss: one loss for all of them, default trivial)\n"
              << "METHOD: 0=baseline, 1=DCS, 2=Switchable (3=Layer, 4=Simple Layer MCTS: not in this backend)\n"
              << "       [--sample-cov S[:SEED]]  (METHOD 0 and 1: after the solve, S posterior samples (seed SEED, default 0) estimate every\n"
              << "       pose's marginal covariance; writes cov_nodes.txt, one line <index> sxx sxy sxt syy syt stt per pose)\n"
              << "Example: " << argv[0] << " INTEL 50 1\n";
    return -1;
  }
  std::string base = "../data", save = "../save", loss_spec = "huber:0.01", loop_spec, score_file, priors_file, prior_loss_spec = "trivial";
  long long seed = -1;
  int device = 0, precision = 0, score_align = 0, init_stride = 0, gnc_inner = 5, sample_n = 0;
  unsigned long long sample_seed = 0;
  double gnc_cbar = 0.0;
  bool gnc_on = false, support_on = false, init_info = false;
  pgo::LoopSupportOptions support;
  bool chordal_on = false;
  pgo::ChordalOptions chordal;
  bool mixture_on = false;
  pgo::MixtureOptions mixture;
  for (int i = 4; i < argc; i += 2) {
    if (!strcmp(argv[i], "--chordal-init")) {   // [ROUNDS[:REJECT_XY[:REJECT_TH]]]: the value is optional
      chordal_on = true;
      if (i + 1 >= argc || !strncmp(argv[i + 1], "--", 2)) {
        --i;
        continue;
      }
      std::vector<std::string> f;
      std::string spec = argv[i + 1];
      for (size_t at = 0; at <= spec.size();) {
        const size_t colon = std::min(spec.find(':', at), spec.size());
        f.push_back(spec.substr(at, colon - at));
        at = colon + 1;
      }
      if (f.size() > 3 || f[0].empty()) { std::cerr << "--chordal-init [ROUNDS[:REJECT_XY[:REJECT_TH]]]\n"; return -1; }
      chordal.rounds = atoi(f[0].c_str());
      if (f.size() > 1) chordal.reject_xy = atof(f[1].c_str());
      if (f.size() > 2) chordal.reject_th = atof(f[2].c_str());
      continue;
    }
    if (!strcmp(argv[i], "--align")) {   // (the one option without a value)
      score_align = 1;
      --i;
      continue;
    }
    if (!strcmp(argv[i], "--init-info")) {
      init_info = true;
      --i;
      continue;
    }
    if (i + 1 >= argc) { std::cerr << "option " << argv[i] << " needs a value\n"; return -1; }
    if (!strcmp(argv[i], "--score")) score_file = argv[i + 1];
    else if (!strcmp(argv[i], "--seed")) seed = atoll(argv[i + 1]);
    else if (!strcmp(argv[i], "--data")) base = argv[i + 1];
    else if (!strcmp(argv[i], "--save")) save = argv[i + 1];
    else if (!strcmp(argv[i], "--device")) device = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--precision")) precision = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--loss")) loss_spec = argv[i + 1];
    else if (!strcmp(argv[i], "--loop-loss")) loop_spec = argv[i + 1];
    else if (!strcmp(argv[i], "--priors")) priors_file = argv[i + 1];
    else if (!strcmp(argv[i], "--prior-loss")) prior_loss_spec = argv[i + 1];
    else if (!strcmp(argv[i], "--init-stride")) init_stride = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--sample-cov")) {   // S[:SEED]
      unsigned long long sd = 0;
      if (sscanf(argv[i + 1], "%d:%llu", &sample_n, &sd) < 1 || sample_n < 1) { std::cerr << "--sample-cov S[:SEED]\n"; return -1; }
      sample_seed = sd;
    }
    else if (!strcmp(argv[i], "--gnc")) { gnc_on = true; gnc_cbar = atof(argv[i + 1]); }
    else if (!strcmp(argv[i], "--gnc-inner")) gnc_inner = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--mixture-null")) {   // PI:SCALE[:INNER]
      mixture_on = true;
      const int got = sscanf(argv[i + 1], "%lf:%lf:%d", &mixture.pi_null, &mixture.scale_null, &mixture.inner_iterations);
      if (got < 2) { std::cerr << "--mixture-null PI:SCALE[:INNER]\n"; return -1; }
    }
    else if (!strcmp(argv[i], "--loop-support")) {   // MIN[:WINDOW[:TOL_XY[:TOL_TH]]]
      support_on = true;
      std::vector<std::string> f;
      std::string spec = argv[i + 1];
      for (size_t at = 0; at <= spec.size();) {
        const size_t colon = std::min(spec.find(':', at), spec.size());
        f.push_back(spec.substr(at, colon - at));
        at = colon + 1;
      }
      if (f.size() > 4 || f[0].empty()) { std::cerr << "--loop-support MIN[:WINDOW[:TOL_XY[:TOL_TH]]]\n"; return -1; }
      support.min_support = atoi(f[0].c_str());
      if (f.size() > 1) support.window = atoi(f[1].c_str());
      if (f.size() > 2) support.tol_xy = atof(f[2].c_str());
      if (f.size() > 3) support.tol_th = atof(f[3].c_str());
    }
    else { std::cerr << "unknown option " << argv[i] << "\n"; return -1; }
  }
  std::unique_ptr<pgo::LossFunction> loss_function, loop_loss, prior_loss;
  try {
    prior_loss = make_loss(prior_loss_spec);
    loss_function = make_loss(loss_spec);
    if (!loop_spec.empty()) loop_loss = make_loss(loop_spec);
    else if (mixture_on) loop_loss = make_loss("trivial");   // (see --help: under huber:0.01 the null component would never win)
  } catch (const std::exception& e) {
    std::cerr << "error: " << e.what() << std::endl;
    return -1;
  }
  pgo::LossFunction* closure_loss = loop_loss ? loop_loss.get() : loss_function.get();
  const int method = atoi(argv[3]);
  if (method < 0 || method > 2) {
    std::cerr << "METHOD " << method << " is not part of the MI355X backend (METHOD 0, 1 and 2 only)\n";
    return 3;
  }
  if (init_info && init_stride == 0) {
    std::cerr << "--init-info goes with --init-stride\n";
    return 2;
  }
  if (gnc_on && method != 0) {
    std::cerr << "--gnc runs on METHOD 0 only (the weights take the place of DCS / the switches)\n";
    return -1;
  }
  if (mixture_on && (method != 0 || gnc_on)) {
    std::cerr << "--mixture-null runs on METHOD 0 only (the selection takes the place of DCS / the switches), and not with --gnc\n";
    return -1;
  }
  if (!priors_file.empty() && method == 2) {
    std::cerr << "--priors: METHOD 0 and 1 only\n";
    return -1;
  }
  if (sample_n > 0 && method == 2) {
    std::cerr << "--sample-cov: METHOD 0 and 1 only (the switch rows would need noise of their own)\n";
    return -1;
  }
  if (support_on && method == 2) {
    std::cerr << "--loop-support writes edge weights: METHOD 0 and 1 only\n";
    return -1;
  }
  try {
    std::cout << "Start Reading PoseGraph\n";
    ReadG2O g2o_manager(base + "/" + argv[1] + ".g2o");
    g2o_manager.add_random_C(atoi(argv[2]), seed);
    mkdir(save.c_str(), 0755);
    g2o_manager.writePoseGraph_nodes(save + "/init_nodes.txt", precision);
    g2o_manager.writePoseGraph_edges(save + "/init_edges.txt");
    std::cout << "total nodes : " << g2o_manager.nNodes.size() << std::endl;
    std::cout << "total nEdgesOdometry : " << g2o_manager.nEdgesOdometry.size() << std::endl;
    std::cout << "total nEdgesClosure : " << g2o_manager.nEdgesClosure.size() << std::endl;
    std::cout << "total nEdgesBogus : " << g2o_manager.nEdgesBogus.size() << std::endl;

    pgo::Problem problem;   // (the loss: main.cpp:68's HuberLoss(0.01) unless --loss / --loop-loss say otherwise)
    const bool DCS_ON = (method == 1), SC_ON = (method == 2);
    std::vector<double> switch_priors;      // for SC (reference main.cpp:105-107)
    std::vector<double*> switch_variables;
    const double sc_prior_lambda = 1.0;
    for (Edge* ed : g2o_manager.nEdgesOdometry)
      problem.AddResidualBlock(OdometryResidue::Create(ed->x, ed->y, ed->theta), loss_function.get(), ed->a->p, ed->b->p);
    for (auto* list : {&g2o_manager.nEdgesClosure, &g2o_manager.nEdgesBogus})
      for (Edge* ed : *list) {
        if (SC_ON) {
          double* s = new double(1.0);
          switch_variables.push_back(s);
          switch_priors.push_back(1.0);
          problem.AddResidualBlock(SwitchableClosureResidue::Create(ed->x, ed->y, ed->theta), closure_loss, ed->a->p, ed->b->p, s);
          problem.AddResidualBlock(SwitchPriorResidue::Create(sc_prior_lambda), nullptr, s);
        } else {
          problem.AddResidualBlock(DCS_ON ? DCSClosureResidue::Create(ed->x, ed->y, ed->theta)
                                          : OdometryResidue::Create(ed->x, ed->y, ed->theta),
                                   closure_loss, ed->a->p, ed->b->p);
        }
      }
    problem.SetParameterBlockConstant(g2o_manager.nNodes[0]->p);
    if (!priors_file.empty()) {   // EDGE_PRIOR_SE2 id x y th I11 I12 I13 I22 I23 I33 (the g2o parser itself does not know the tag)
      std::ifstream in(priors_file);
      if (!in) throw std::runtime_error("cannot open " + priors_file);
      std::string tag;
      int id;
      double z[3], w[6];
      int n_priors = 0;
      std::unordered_map<int, Node*> by_id;   // vertex id -> node, built once
      for (Node* nd : g2o_manager.nNodes) by_id[nd->index] = nd;
      while (in >> tag) {
        if (tag != "EDGE_PRIOR_SE2" || !(in >> id >> z[0] >> z[1] >> z[2] >> w[0] >> w[1] >> w[2] >> w[3] >> w[4] >> w[5]))
          throw std::runtime_error(priors_file + ": expected EDGE_PRIOR_SE2 id x y th I11 I12 I13 I22 I23 I33");
        const auto found = by_id.find(id);
        Node* at = found == by_id.end() ? nullptr : found->second;
        if (!at) throw std::runtime_error(priors_file + ": vertex " + std::to_string(id) + " is not in the dataset");
        problem.AddResidualBlock(PosePriorResidue::Create(z[0], z[1], z[2], w), prior_loss.get(), at->p);
        ++n_priors;
      }
      std::cout << "total pose priors : " << n_priors << std::endl;
    }

    pgo::Solver::Options options;
    options.minimizer_progress_to_stdout = true;
    options.linear_solver_type = pgo::SPARSE_NORMAL_CHOLESKY;
    options.device = device;
    pgo::Solver::Summary summary;
    const size_t n_odo = g2o_manager.nEdgesOdometry.size(), n_all = (size_t)problem.NumResidualBlocks();
    if (support_on) {   // the closure and bogus blocks (added after the odometry blocks, above) judged by odometry cycle consistency
      support.apply = true;
      support.select.assign(n_all, 1);
      std::fill(support.select.begin(), support.select.begin() + (long)n_odo, (uint8_t)0);
      pgo::LoopSupportSummary ss;
      pgo::LoopSupport(options, support, &problem, &ss);
      const size_t n_clo = g2o_manager.nEdgesClosure.size();
      size_t drop_clo = 0, drop_bogus = 0;
      for (size_t e = n_odo; e < n_all; ++e)
        if (ss.blocks[e].selected && ss.blocks[e].n_consistent < support.min_support) ++(e < n_odo + n_clo ? drop_clo : drop_bogus);
      std::cout << "loop-support: min " << support.min_support << " window " << support.window << " tol_xy " << support.tol_xy << " tol_th "
                << support.tol_th << ": " << ss.stats.n_selected << " selected blocks, " << ss.stats.n_supported << " supported, dropped "
                << drop_clo << " closure and " << drop_bogus << " bogus; " << ss.stats.n_pairs_total << " pairs, at most " << ss.stats.max_pairs
                << " per block" << std::endl;
    }
    if (chordal_on) {   // the linear start: chordal rotations, then positions; the blocks its reject rounds drop stay dropped
      chordal.apply_weights = chordal.rounds > 0 && method != 2;
      pgo::ChordalSummary cs;
      pgo::ChordalInit(options, chordal, &problem, &cs);
      const pgo_chordal_solve& last = cs.s.solve[cs.s.n_solves - 1];
      std::cout << "chordal-init: rounds " << chordal.rounds << " reject_xy " << chordal.reject_xy << " reject_th " << chordal.reject_th << ": "
                << cs.s.n_solves << " solves, " << cs.s.n_rejected << " blocks rejected, " << last.iters[0] << " + " << last.iters[1]
                << " iterations, min |z| " << cs.s.min_mag << ", " << cs.s.n_degenerate << " degenerate" << std::endl;
    }
    if (init_stride != 0) {   // hierarchical initialisation: the parameter blocks start at the coarse graph's prolonged solution
      pgo::Solver::Options coarse_options;
      coarse_options.device = device;
      pgo::Solver::Summary coarse;
      pgo::InitializeHierarchical(&problem, init_stride, coarse_options, &coarse, init_info);
      std::cout << "init-stride " << init_stride << (init_info ? " (propagated information)" : "") << ": coarse graph of " << coarse.num_parameter_blocks << " poses and " << coarse.num_residual_blocks
                << " edges, cost " << coarse.s.initial_cost << " -> " << coarse.s.final_cost << " in " << coarse.s.iterations << " iterations"
                << std::endl;
    }
    if (gnc_on) {   // graduated non-convexity over the closure and bogus blocks (added after the odometry blocks, above)
      pgo::GncOptions gnc;
      gnc.cbar = gnc_cbar;
      gnc.inner_iterations = gnc_inner;
      gnc.select.assign(n_all, 1);
      std::fill(gnc.select.begin(), gnc.select.begin() + (long)n_odo, (uint8_t)0);
      for (size_t e = 0; e < problem.ResidualBlockWeights().size(); ++e)   // (--loop-support: a dropped block stays dropped)
        if (problem.ResidualBlockWeights()[e] == 0.0) gnc.select[e] = 0;
      pgo::GncSummary gs;
      options.minimizer_progress_to_stdout = false;
      pgo::SolveGnc(options, gnc, &problem, &gs);
      std::cout << "gnc: cbar " << gnc_cbar << ", " << gs.g.n_selected << " selected blocks, rmax2 " << gs.g.rmax2 << ", mu0 " << gs.g.mu0 << "\n";
      for (size_t k = 0; k < gs.rounds.size(); ++k)
        std::cout << "gnc round " << k + 1 << ": mu " << gs.rounds[k].mu << " weighted_cost " << gs.rounds[k].weighted_cost << " nonbinary "
                  << gs.rounds[k].n_nonbinary << " zero " << gs.rounds[k].n_zero << " lm_iterations " << gs.rounds[k].lm_iterations
                  << " lm_termination " << gs.rounds[k].lm_termination << "\n";
      std::cout << "gnc: " << gs.g.rounds << " rounds" << (gs.g.hit_max_rounds ? " (max_rounds reached)" : "") << ", " << gs.g.n_zero
                << " blocks at weight 0" << std::endl;
      summary = gs.final_solve;
      std::ofstream wf(save + "/weights.txt");
      wf.precision(17);
      for (double w : gs.weights) wf << w << "\n";
      if (!wf) throw std::runtime_error("cannot write " + save + "/weights.txt");
    } else if (mixture_on) {   // a null hypothesis beside the closure and bogus blocks (added after the odometry blocks, above)
      mixture.select.assign(n_all, 1);
      std::fill(mixture.select.begin(), mixture.select.begin() + (long)n_odo, (uint8_t)0);
      pgo::MixtureSummary ms;
      options.minimizer_progress_to_stdout = false;
      pgo::SolveMixture(options, mixture, &problem, &ms);
      std::cout.precision(12);
      for (size_t k = 0; k < ms.rounds.size(); ++k)
        std::cout << "mixture round " << k + 1 << ": objective " << ms.rounds[k].objective << " changed " << ms.rounds[k].n_changed << " inlier "
                  << ms.rounds[k].count[0] << " null " << ms.rounds[k].count[1] << " lm_iterations " << ms.rounds[k].lm_iterations
                  << " lm_termination " << ms.rounds[k].lm_termination << "\n";
      size_t n_null = 0;
      for (int32_t k : ms.selection) n_null += k == 1;
      std::cout << "mixture: " << ms.m.rounds << " rounds" << (ms.m.hit_max_rounds ? " (max_rounds reached)" : "") << ", " << ms.m.n_mix
                << " mixture blocks, " << n_null << " on the null hypothesis, " << ms.m.n_would_change << " would change" << std::endl;
      std::cout.precision(6);
      summary = ms.final_solve;
      std::ofstream wf(save + "/weights.txt");
      wf.precision(17);
      for (double w : ms.weights) wf << w << "\n";
      if (!wf) throw std::runtime_error("cannot write " + save + "/weights.txt");
    } else {
      pgo::Solve(options, &problem, &summary);
      if (support_on) {
        std::ofstream wf(save + "/weights.txt");
        wf.precision(17);
        for (double w : problem.ResidualBlockWeights()) wf << w << "\n";
        if (!wf) throw std::runtime_error("cannot write " + save + "/weights.txt");
      }
    }
    std::cout << summary.FullReport() << std::endl;

    if (sample_n > 0) {   // every pose's marginal covariance at the result, from sample_n posterior samples
      pgo::SampleOptions so;
      so.num_samples = sample_n;
      so.seed = sample_seed;
      pgo::SampleSummary ss;
      pgo::SamplePosterior(options, so, &problem, &ss);
      std::ofstream cf(save + "/cov_nodes.txt");
      cf.precision(17);
      for (size_t i = 0; i < g2o_manager.nNodes.size(); ++i) {
        const double* c = &ss.covariance[9 * i];
        cf << g2o_manager.nNodes[i]->index << " " << c[0] << " " << c[1] << " " << c[2] << " " << c[4] << " " << c[5] << " " << c[8] << "\n";
      }
      if (!cf) throw std::runtime_error("cannot write " + save + "/cov_nodes.txt");
      std::cout << "sample-cov: " << sample_n << " samples in " << ss.report.passes << " passes, " << ss.report.pcg_iters_total
                << " PCG iterations, max relative residual " << ss.report.max_rel_residual << ", " << ss.report.seconds << " s" << std::endl;
    }
    g2o_manager.writePoseGraph_nodes(save + "/opt_nodes.txt", precision);
    g2o_manager.writePoseGraph_edges(save + "/opt_edges.txt");
    if (SC_ON) g2o_manager.writePoseGraph_switches(save + "/switches.txt", switch_priors, switch_variables);
    for (double* s : switch_variables) delete s;
    if (!score_file.empty()) {   // the result (Node::p, optimised in place) against the reference poses of FILE
      std::ifstream in(score_file);
      if (!in) throw std::runtime_error("cannot open " + score_file);
      std::vector<double> ref, est;
      double idx, x, y, th;
      while (in >> idx >> x >> y >> th) ref.insert(ref.end(), {x, y, th});
      const size_t n = g2o_manager.nNodes.size();
      if (!in.eof() || ref.size() != 3 * n)
        throw std::runtime_error(score_file + ": " + std::to_string(ref.size() / 3) + " poses read, the graph has " + std::to_string(n));
      for (Node* nd : g2o_manager.nNodes) est.insert(est.end(), nd->p, nd->p + 3);
      pgo_traj_options topt;
      pgo_traj_options_default(&topt);
      topt.align = score_align;
      pgo_traj_error te;
      if (pgo_trajectory_error_eval((int32_t)n, est.data(), ref.data(), nullptr, &topt, &te, nullptr) != PGO_OK)
        throw std::runtime_error(pgo_last_error());
      std::cout << "score: ate_rmse " << te.ate_rmse << " ate_max " << te.ate_max << " rot_rmse " << te.rot_rmse << " rpe_trans_rmse "
                << te.rpe_trans_rmse << " rpe_rot_rmse " << te.rpe_rot_rmse << (score_align ? " (aligned)" : "") << std::endl;
    }
  } catch (const std::exception& e) {
    std::cerr << "error: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
