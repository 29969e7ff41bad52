// The slice of the ceres API that DCS-ceres/main.cpp:66-164 uses, re-hosted on libpgo.so:
//   Problem::AddResidualBlock(cost, loss, p1, p2)   main.cpp:99,114,128,137,148
//   Problem::SetParameterBlockConstant(p)           main.cpp:153
//   Solver::Options / Solver::Summary / Solve()     main.cpp:154-164
// Parameter blocks are identified by their double* (Node::p), as in Ceres, and are updated in place.
#ifndef PGO_HOST_PROBLEM_H_
#define PGO_HOST_PROBLEM_H_

#include <cstdio>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "ceres_error.h"
#include "pgo.h"

namespace pgo {

// ceres::LossFunction and the family the device evaluates (include/pgo.h, "robust losses").  A residual block added with
// a NULL loss has the Trivial one, as in Ceres.
struct LossFunction {
  explicit LossFunction(int32_t type, double a = 0.0) {
    l_.type = type;
    l_._pad = 0;
    l_.a = type == PGO_LOSS_TRIVIAL ? 0.0 : a;
  }
  virtual ~LossFunction() {}
  // rho[0..2] = rho(s), rho'(s), rho''(s)
  void Evaluate(double s, double rho[3]) const {
    const int st = pgo_loss_evaluate(&l_, s, rho);
    if (st != PGO_OK) throw std::invalid_argument(std::string("loss: ") + pgo_last_error());
  }
  const pgo_loss& loss() const { return l_; }

 private:
  pgo_loss l_;
};
struct TrivialLoss : LossFunction { TrivialLoss() : LossFunction(PGO_LOSS_TRIVIAL) {} };
struct HuberLoss : LossFunction { explicit HuberLoss(double a) : LossFunction(PGO_LOSS_HUBER, a) {} };  // main.cpp:68
struct SoftLOneLoss : LossFunction { explicit SoftLOneLoss(double a) : LossFunction(PGO_LOSS_SOFTLONE, a) {} };
struct CauchyLoss : LossFunction { explicit CauchyLoss(double a) : LossFunction(PGO_LOSS_CAUCHY, a) {} };
struct ArctanLoss : LossFunction { explicit ArctanLoss(double a) : LossFunction(PGO_LOSS_ARCTAN, a) {} };
struct TukeyLoss : LossFunction { explicit TukeyLoss(double a) : LossFunction(PGO_LOSS_TUKEY, a) {} };

enum LinearSolverType { SPARSE_NORMAL_CHOLESKY, BLOCK_JACOBI_PCG };

class Problem {
 public:
  void AddResidualBlock(CostFunction* cost, LossFunction* loss, double* p1, double* p2) {
    std::unique_ptr<CostFunction> own(cost);  // TAKE_OWNERSHIP, as Ceres does by default
    if (p1 == p2) throw std::invalid_argument("duplicate parameter block in a residual block");
    const uint8_t cls = loss_class(loss);
    ia_.push_back(block(p1));
    ib_.push_back(block(p2));
    meas_.insert(meas_.end(), {cost->dx, cost->dy, cost->dtheta});
    if (cost->kind == CostFunction::SWITCHABLE || cost->kind == CostFunction::SWITCH_PRIOR)
      throw std::invalid_argument("switchable blocks take the (P1, P2, S) / (S) overloads");
    const bool dcs = cost->kind == CostFunction::DCS;
    kind_.push_back(dcs ? PGO_EDGE_CLOSURE : PGO_EDGE_ODOMETRY);
    switch_.push_back(nullptr);
    any_dcs_ = any_dcs_ || dcs;
    class_.push_back(cls);
  }
  // SwitchableClosureResidue: (P1, P2, S)  (reference main.cpp:122,143)
  void AddResidualBlock(CostFunction* cost, LossFunction* loss, double* p1, double* p2, double* s) {
    std::unique_ptr<CostFunction> own(cost);
    if (cost->kind != CostFunction::SWITCHABLE) throw std::invalid_argument("three parameter blocks: SwitchableClosureResidue only");
    if (p1 == p2) throw std::invalid_argument("duplicate parameter block in a residual block");
    const uint8_t cls = loss_class(loss);
    ia_.push_back(block(p1));
    ib_.push_back(block(p2));
    meas_.insert(meas_.end(), {cost->dx, cost->dy, cost->dtheta});
    kind_.push_back(PGO_EDGE_CLOSURE);
    switch_.push_back(s);
    any_sc_ = true;
    class_.push_back(cls);
  }
  // One parameter block.  SwitchPriorResidue: (S), no loss  (reference main.cpp:124-125,144-145).  PosePriorResidue: (P), an
  // absolute prior on the pose block P (include/pgo.h, "pose priors") -- at most one per block, and ONE loss (NULL = Trivial) for
  // all pose priors of a problem; they are no residual blocks of NumResidualBlocks() and carry no residual block weight.
  void AddResidualBlock(CostFunction* cost, LossFunction* loss, double* p) {
    std::unique_ptr<CostFunction> own(cost);
    if (cost->kind == CostFunction::POSE_PRIOR) {
      const pgo_loss l = loss ? loss->loss() : TrivialLoss().loss();
      if (!prior_pose_.empty() && (l.type != prior_loss_.type || l.a != prior_loss_.a))
        throw std::invalid_argument("this backend takes one loss function for all pose priors of a problem");
      const int32_t k = block(p);
      for (int32_t q : prior_pose_)
        if (q == k) throw std::invalid_argument("this backend takes at most one pose prior per parameter block");
      prior_loss_ = l;
      prior_pose_.push_back(k);
      prior_mean_.insert(prior_mean_.end(), {cost->dx, cost->dy, cost->dtheta});
      prior_info_.insert(prior_info_.end(), cost->info, cost->info + 6);
      return;
    }
    if (cost->kind != CostFunction::SWITCH_PRIOR || loss) throw std::invalid_argument("one parameter block: SwitchPriorResidue without loss, or PosePriorResidue");
    prior_lambda_[p] = cost->dx;
  }
  int NumPosePriors() const { return (int)prior_pose_.size(); }
  // Any number of blocks may be made constant.  The first one is the handle's fixed pose (one block, called once: exactly
  // the path of a problem with a single anchor); the others, and the blocks that appear in no residual block, are applied
  // through pgo_set_active when the problem is solved.
  void SetParameterBlockConstant(double* p) {
    const int32_t k = block(p);
    for (int32_t c : constant_)
      if (c == k) return;
    constant_.push_back(k);
    fixed_ = constant_[0];
  }
  // Problem::AddParameterBlock: a pose block of its own; one that no residual block uses is constant, as it would not be
  // part of Ceres' reduced program
  void AddParameterBlock(double* p, int size = 3) {
    if (size != 3) throw std::invalid_argument("pose blocks have 3 parameters");
    block(p);
  }
  int NumResidualBlocks() const { return (int)ia_.size(); }
  int NumParameterBlocks() const { return (int)ptr_.size(); }
  // The weight in [0, 1] of every residual block, in the order the blocks were added (include/pgo.h, "edge weight plane"):
  // what LoopSupport with apply left, or the caller's own.  Empty: none -- every block counts fully.  Blocks added afterwards
  // have weight 1.  A problem with weights is a METHOD 0 or DCS one.
  const std::vector<double>& ResidualBlockWeights() const { return weights_; }
  void SetResidualBlockWeights(const std::vector<double>& w) {
    if (w.size() > ia_.size()) throw std::invalid_argument("more weights than residual blocks");
    weights_ = w;
  }

 private:
  friend struct SolverAccess;
  // the block's loss class: every distinct loss value (type, a) is one class, NULL = Trivial; the device has 4 classes
  uint8_t loss_class(const LossFunction* loss) {
    const pgo_loss l = loss ? loss->loss() : TrivialLoss().loss();
    for (size_t k = 0; k < losses_.size(); ++k)
      if (losses_[k].type == l.type && losses_[k].a == l.a) return (uint8_t)k;
    if (losses_.size() == 4) throw std::invalid_argument("this backend takes at most 4 distinct loss functions per problem");
    losses_.push_back(l);
    return (uint8_t)(losses_.size() - 1);
  }
  int32_t block(double* p) {
    auto it = id_.find(p);
    if (it != id_.end()) return it->second;
    int32_t k = (int32_t)ptr_.size();
    id_[p] = k;
    ptr_.push_back(p);
    return k;
  }
  std::unordered_map<double*, int32_t> id_;
  std::vector<double*> ptr_;
  std::vector<int32_t> ia_, ib_;
  std::vector<double> meas_;
  std::vector<uint8_t> kind_;
  int32_t fixed_ = -1;
  std::vector<int32_t> constant_;                  // every constant block, in the order they were set (fixed_ = the first)
  std::vector<pgo_loss> losses_;                   // the distinct losses (pgo_set_losses' classes)
  std::vector<uint8_t> class_;                     // per residual block: its loss class
  std::vector<double*> switch_;                    // per residual block: its switch variable or nullptr
  std::unordered_map<double*, double> prior_lambda_;  // switch -> lambda of its prior
  bool any_dcs_ = false, any_sc_ = false;
  std::vector<double> weights_;                    // per residual block, or empty (SetResidualBlockWeights)
  std::vector<int32_t> prior_pose_;                // pose priors (PosePriorResidue): the block, the mean (x 3), the information (x 6)
  std::vector<double> prior_mean_, prior_info_;
  pgo_loss prior_loss_ = {PGO_LOSS_TRIVIAL, 0, 0.0};
};

namespace Solver {
struct Options {
  bool minimizer_progress_to_stdout = false;
  LinearSolverType linear_solver_type = SPARSE_NORMAL_CHOLESKY;  // = the library's exact solve: the direct chain + low-rank solve where it applies
                                                                 // (INTEL, MIT, CSAIL, FR079 ...), else PCG to pcg_rtol; BLOCK_JACOBI_PCG: always PCG
  int max_num_iterations = 50;
  double function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  double initial_trust_region_radius = 1e4;
  double pcg_rtol = 1e-10;
  int pcg_max_iters = 200000;
  int device = 0;
};
struct Summary {
  pgo_summary s{};
  std::vector<pgo_iter_record> iterations;
  int num_parameter_blocks = 0, num_residual_blocks = 0;
  std::string FullReport() const {
    static const char* term[] = {"?", "CONVERGENCE (function tolerance)", "CONVERGENCE (gradient tolerance)",
                                 "CONVERGENCE (parameter tolerance)", "NO_CONVERGENCE (max iterations)",
                                 "NO_CONVERGENCE (min trust region radius)", "FAILURE"};
    std::ostringstream o;
    char b[256];
    o << "\nSolver Summary (pgo-amd, MI355X HIP backend)\n\n";
    o << "Parameter blocks   " << num_parameter_blocks << "\nResidual blocks    " << num_residual_blocks << "\n";
    o << "Linear solver      block-Jacobi PCG (total " << s.total_pcg_iters << " iterations)\n\n";
    snprintf(b, sizeof b, "Cost:\nInitial  %.6e\nFinal    %.6e\nChange   %.6e\n\n", s.initial_cost, s.final_cost, s.initial_cost - s.final_cost);
    o << b;
    o << "Minimizer iterations  " << s.iterations << "\nSuccessful steps      " << s.successful_steps << "\n\n";
    snprintf(b, sizeof b, "Time (in seconds):\n  Residual+Jacobian  %.6f\n  Assembly           %.6f\n  Linear solver      %.6f\n  Candidate cost     %.6f\nTotal                %.6f\n\n",
             s.seconds_eval, s.seconds_assemble, s.seconds_linear, s.seconds_candidate, s.seconds_total);
    o << b << "Termination: " << term[(s.termination >= 0 && s.termination <= 6) ? s.termination : 0] << "\n";
    return o.str();
  }
};
}  // namespace Solver

// Graduated non-convexity with the TLS surrogate (include/pgo.h, "graduated non-convexity"; pgo_gnc_solve) around the
// problem's solves.  The problem must be a METHOD 0 one (no DCS, no switchable blocks).
struct GncOptions {
  double cbar = 0.0;                 // no default: the residual norm above which a block is an outlier
  double mu_factor = 1.4;
  int inner_iterations = 5, final_iterations = 50, max_rounds = 100;
  // one byte per residual block, in the order the blocks were added: non-zero = the block takes part.  Empty: the blocks the
  // problem classifies as other than kind 0 (odometry) -- in a METHOD 0 problem every block is kind 0, so name the loops here
  std::vector<uint8_t> select;
};
struct GncSummary {
  pgo_gnc_summary g{};
  std::vector<pgo_gnc_round> rounds;
  std::vector<double> weights;       // per residual block, after the call
  Solver::Summary final_solve;       // the last solve's summary and iteration records
};

// Max-mixture residual blocks (include/pgo.h, "max-mixture edges"; pgo_mixture_solve) around the problem's solves.  The problem
// must be a METHOD 0 one (no DCS, no switchable blocks).  Either a table -- block[] strictly ascending in the order the blocks
// were added, comp_ptr[] its CSR offsets into comps[] -- or, with block empty, the null hypothesis (pi_null, scale_null) beside
// every block named by select (empty: the blocks the problem classifies as other than kind 0, as GncOptions::select).
struct MixtureOptions {
  int inner_iterations = 2, final_iterations = 50, max_rounds = 50;
  std::vector<int32_t> block, comp_ptr;
  std::vector<pgo_mix_component> comps;
  double pi_null = 0.0, scale_null = 0.0;
  std::vector<uint8_t> select;
};
struct MixtureSummary {
  pgo_mixture_summary m{};
  std::vector<pgo_mixture_round> rounds;
  std::vector<int32_t> selection;    // per mixture block, in the table's order: the component in force after the call
  std::vector<double> weights;       // per residual block, after the call
  Solver::Summary final_solve;       // the last solve's summary and iteration records
};

// Loop edges judged by odometry cycle consistency (include/pgo.h, "loop support"; pgo_loop_support): no solve, no estimate.
// The default tolerances fit pgo_synth_manhattan's odometry noise; a real dataset needs its own.
struct LoopSupportOptions {
  int window = 32, min_support = 1;
  double tol_xy = 0.1, tol_th = 0.05;
  bool apply = false;                // true: the verdict becomes the problem's residual block weights (1 supported, 0 not)
  // one byte per residual block, in the order the blocks were added: non-zero = the block is a loop to judge.  Empty: the blocks
  // the problem classifies as other than kind 0 (odometry) -- in a METHOD 0 problem every block is kind 0, so name the loops here
  std::vector<uint8_t> select;
};
struct LoopSupportSummary {
  pgo_loop_support_stats stats{};
  std::vector<pgo_loop_support_record> blocks;   // per residual block
};

// An estimate-free linear start (include/pgo.h, "chordal initialisation"; pgo_chordal_init): chordal rotations, then positions
// given the rotations, from the measurements and the constant blocks alone.  The defaults are pgo_chordal_options_default's.
struct ChordalOptions {
  double rtol = 1e-8, mag_min = 1e-3;
  int max_iters = 20000, check_every = 50;
  int rounds = 0;                          // reject rounds: after a solve, drop the blocks off the chain whose residual exceeds ...
  double reject_xy = 2.0, reject_th = 0.35;   // ... these (metres, radians), and solve again
  bool apply_weights = false;              // true: the dropped blocks get the residual block weight 0
};
struct ChordalSummary {
  pgo_chordal_summary s{};
  std::vector<double> residuals;           // per residual block: |position residual|, |heading residual|
};

// Posterior sampling (include/pgo.h, "posterior sampling"): draws delta ~ N(0, (J'J)^-1) around the problem's CURRENT parameter
// blocks (call Solve first) and their second moment per parameter block.  The defaults are pgo_sample_options_default's.
struct SampleOptions {
  int num_samples = 256;
  uint64_t seed = 0;
  int first_sample = 0;
  double rtol = 1e-10;
  int max_iters = 20000, samples_per_pass = 24;
  bool direct = false;          // true: the handle's direct solve (problems the direct solve covers only; never a fallback)
  bool keep_samples = false;    // true: SampleSummary::samples holds the draws
};
struct SampleSummary {
  pgo_covariance_report report{};
  std::vector<double> covariance;   // per parameter block: row-major 3x3 in (x, y, theta); zero on constant blocks
  std::vector<double> samples;      // keep_samples: num_samples x blocks x 3 increments
};

struct SolverAccess {
  static void check(int st) {
    if (st != PGO_OK) throw std::runtime_error(std::string("pgo: ") + pgo_strerror(st) + ": " + pgo_last_error());
  }
  // Problem -> device handle (the arrays the residual blocks were recorded into)
  // the problem's loss classes on a handle or a batch (one Huber or NULL loss for all blocks: the library's default path)
  static std::vector<pgo_loss> LossTable(const Problem* pr) {
    return pr->losses_.empty() ? std::vector<pgo_loss>{TrivialLoss().loss()} : pr->losses_;
  }
  static bool SameLosses(const Problem* a, const Problem* b) {
    const std::vector<pgo_loss> x = LossTable(a), y = LossTable(b);
    if (x.size() != y.size()) return false;
    for (size_t k = 0; k < x.size(); ++k)
      if (x[k].type != y[k].type || x[k].a != y[k].a) return false;
    return true;
  }
  // pose_constant of pgo_set_active for a problem that needs it -- more than one constant block, or a block without a
  // residual block -- else empty: the handle then runs exactly as it does for a problem with one anchor
  static std::vector<uint8_t> ConstantMask(const Problem* pr) {
    const size_t N = pr->ptr_.size();
    std::vector<uint8_t> used(N, 0), mask;
    for (size_t e = 0; e < pr->ia_.size(); ++e) used[pr->ia_[e]] = used[pr->ib_[e]] = 1;
    bool need = pr->constant_.size() > 1;
    for (size_t i = 0; i < N && !need; ++i) need = !used[i];
    if (!need) return mask;
    mask.assign(N, 0);
    for (int32_t c : pr->constant_) mask[c] = 1;
    return mask;
  }
  static pgo_t* Prepare(const Solver::Options& opt, Problem* pr) {
    const int32_t N = (int32_t)pr->ptr_.size(), E = (int32_t)pr->ia_.size();
    std::vector<double> poses((size_t)3 * N);
    for (int32_t i = 0; i < N; ++i)
      for (int k = 0; k < 3; ++k) poses[3 * (size_t)i + k] = pr->ptr_[i][k];
    pgo_options o;
    pgo_options_default(&o);
    if (pr->any_sc_ && pr->any_dcs_) throw std::invalid_argument("DCS and switchable blocks cannot be mixed (the reference's METHOD is one of them)");
    o.method = pr->any_sc_ ? 2 : (pr->any_dcs_ ? 1 : 0);
    if (pr->any_sc_) {  // every switch needs exactly its prior, all with one lambda (as main.cpp:107)
      double lam = -1.0;
      for (double* sp : pr->switch_) {
        if (!sp) continue;
        auto it = pr->prior_lambda_.find(sp);
        if (it == pr->prior_lambda_.end()) throw std::invalid_argument("a switch variable has no SwitchPriorResidue");
        if (lam >= 0.0 && it->second != lam) throw std::invalid_argument("this backend needs one lambda for all switch priors");
        lam = it->second;
        if (*sp != 1.0) throw std::invalid_argument("switch variables must start at 1.0 (main.cpp:117,139)");
      }
      o.sc_prior_lambda = lam;
    }
    o.fixed_pose = pr->fixed_;
    o.max_iters = opt.max_num_iterations;
    o.ftol = opt.function_tolerance;
    o.gtol = opt.gradient_tolerance;
    o.ptol = opt.parameter_tolerance;
    o.radius0 = opt.initial_trust_region_radius;
    o.pcg_rtol = opt.pcg_rtol;
    o.linear_solver = opt.linear_solver_type == BLOCK_JACOBI_PCG ? 1 : 0;
    o.pcg_max_iters = opt.pcg_max_iters;
    o.verbose = opt.minimizer_progress_to_stdout ? 1 : 0;
    pgo_t* h = nullptr;
    check(pgo_create(&h, N, poses.data(), E, pr->ia_.data(), pr->ib_.data(), pr->meas_.data(), pr->kind_.data(), &o, nullptr, opt.device));
    const std::vector<pgo_loss> L = LossTable(pr);
    int st = pgo_set_losses(h, (int32_t)L.size(), L.data(), E ? pr->class_.data() : nullptr);
    const std::vector<uint8_t> mask = ConstantMask(pr);
    if (st == PGO_OK && !mask.empty()) st = pgo_set_active(h, nullptr, mask.data());
    if (st == PGO_OK && !pr->weights_.empty()) {
      std::vector<double> w = pr->weights_;
      w.resize((size_t)E, 1.0);
      st = pgo_set_edge_weights(h, w.data());
    }
    if (st == PGO_OK && !pr->prior_pose_.empty())   // (every solve goes through here: Solve, SolveGnc, SolveMixture carry the priors)
      st = pgo_set_priors(h, (int32_t)pr->prior_pose_.size(), pr->prior_pose_.data(), pr->prior_mean_.data(), pr->prior_info_.data(), &pr->prior_loss_);
    if (st != PGO_OK) {
      const std::string msg = pgo_last_error();
      pgo_destroy(h);
      throw std::runtime_error(std::string("pgo: ") + pgo_strerror(st) + ": " + msg);
    }
    return h;
  }
  // results back into the caller's parameter blocks (in place, like Ceres); destroys the handle
  static void Finish(Problem* pr, pgo_t* h, int st, Solver::Summary* sum) {
    const int32_t N = (int32_t)pr->ptr_.size(), E = (int32_t)pr->ia_.size();
    std::vector<double> poses((size_t)3 * N);
    if (st == PGO_OK) st = pgo_get_poses(h, poses.data());
    std::vector<double> sw((size_t)E, 1.0);
    if (st == PGO_OK && pr->any_sc_) st = pgo_get_switches(h, sw.data(), nullptr);
    if (st == PGO_OK) {
      sum->iterations.resize((size_t)pgo_num_iter_records(h));
      st = pgo_get_iter_records(h, sum->iterations.data(), (int32_t)sum->iterations.size());
    }
    pgo_destroy(h);
    check(st);
    for (int32_t i = 0; i < N; ++i)
      for (int k = 0; k < 3; ++k) pr->ptr_[i][k] = poses[3 * (size_t)i + k];
    for (int32_t e = 0; e < E; ++e)
      if (pr->switch_[e]) *pr->switch_[e] = sw[(size_t)e];
    sum->num_parameter_blocks = N;
    sum->num_residual_blocks = E;
  }
  static void Solve(const Solver::Options& opt, Problem* pr, Solver::Summary* sum) {
    pgo_t* h = Prepare(opt, pr);
    const int st = pgo_solve(h, &sum->s);
    Finish(pr, h, st, sum);
  }
  static void SolveGnc(const Solver::Options& opt, const GncOptions& gnc, Problem* pr, GncSummary* sum) {
    const size_t E = pr->ia_.size();
    if (!gnc.select.empty() && gnc.select.size() != E) throw std::invalid_argument("GncOptions::select: one byte per residual block");
    pgo_t* h = Prepare(opt, pr);
    pgo_gnc_options o;
    pgo_gnc_options_default(&o);
    o.cbar = gnc.cbar;
    o.mu_factor = gnc.mu_factor;
    o.inner_iters = gnc.inner_iterations;
    o.final_iters = gnc.final_iterations;
    o.max_rounds = gnc.max_rounds;
    o.select = gnc.select.empty() ? nullptr : gnc.select.data();
    sum->rounds.assign((size_t)(gnc.max_rounds > 0 ? gnc.max_rounds : 0), pgo_gnc_round());
    int st = pgo_gnc_solve(h, &o, &sum->g, sum->rounds.data(), (int32_t)sum->rounds.size());
    sum->rounds.resize((size_t)(st == PGO_OK ? sum->g.rounds : 0));
    sum->weights.assign(E, 1.0);
    if (st == PGO_OK && E > 0) st = pgo_get_edge_weights(h, sum->weights.data());
    sum->final_solve.s = sum->g.final_solve;
    Finish(pr, h, st, &sum->final_solve);
  }
  static void SolveMixture(const Solver::Options& opt, const MixtureOptions& mix, Problem* pr, MixtureSummary* sum) {
    const size_t E = pr->ia_.size();
    if (!mix.select.empty() && mix.select.size() != E) throw std::invalid_argument("MixtureOptions::select: one byte per residual block");
    if (!mix.block.empty() && mix.comp_ptr.size() != mix.block.size() + 1)
      throw std::invalid_argument("MixtureOptions::comp_ptr: one entry per mixture block and one more");
    if (!mix.block.empty() && (size_t)std::max(mix.comp_ptr.back(), 0) > mix.comps.size())
      throw std::invalid_argument("MixtureOptions::comps: fewer components than comp_ptr names");
    pgo_t* h = Prepare(opt, pr);
    int st = mix.block.empty() ? pgo_set_mixture_null(h, mix.select.empty() ? nullptr : mix.select.data(), mix.pi_null, mix.scale_null)
                               : pgo_set_mixtures(h, (int32_t)mix.block.size(), mix.block.data(), mix.comp_ptr.data(), mix.comps.data());
    pgo_mixture_options o;
    pgo_mixture_options_default(&o);
    o.inner_iters = mix.inner_iterations;
    o.final_iters = mix.final_iterations;
    o.max_rounds = mix.max_rounds;
    sum->rounds.assign((size_t)(mix.max_rounds > 0 ? mix.max_rounds : 0), pgo_mixture_round());
    if (st == PGO_OK) st = pgo_mixture_solve(h, &o, &sum->m, sum->rounds.data(), (int32_t)sum->rounds.size());
    sum->rounds.resize((size_t)(st == PGO_OK ? sum->m.rounds : 0));
    sum->selection.assign(E, -1);
    if (st == PGO_OK) st = pgo_get_mixture_selection(h, sum->selection.data());
    sum->selection.resize((size_t)(st == PGO_OK ? sum->m.n_mix : 0));
    sum->weights.assign(E, 1.0);
    if (st == PGO_OK && E > 0) st = pgo_get_edge_weights(h, sum->weights.data());
    sum->final_solve.s = sum->m.final_solve;
    Finish(pr, h, st, &sum->final_solve);
  }
  static void LoopSupport(const Solver::Options& opt, const LoopSupportOptions& ls, Problem* pr, LoopSupportSummary* sum) {
    const size_t E = pr->ia_.size();
    if (!ls.select.empty() && ls.select.size() != E) throw std::invalid_argument("LoopSupportOptions::select: one byte per residual block");
    pgo_t* h = Prepare(opt, pr);
    pgo_loop_support_options o;
    pgo_loop_support_options_default(&o);
    o.window = ls.window;
    o.min_support = ls.min_support;
    o.tol_xy = ls.tol_xy;
    o.tol_th = ls.tol_th;
    o.apply = ls.apply ? 1 : 0;
    sum->blocks.assign(E, pgo_loop_support_record());
    int st = pgo_loop_support(h, &o, ls.select.empty() ? nullptr : ls.select.data(), sum->blocks.data(), &sum->stats);
    std::vector<double> w(E, 1.0);
    if (st == PGO_OK && ls.apply && E > 0) st = pgo_get_edge_weights(h, w.data());
    const std::string msg = st != PGO_OK ? std::string(pgo_last_error()) : std::string();
    pgo_destroy(h);
    if (st != PGO_OK) throw std::runtime_error(std::string("pgo: ") + pgo_strerror(st) + ": " + msg);
    if (ls.apply) pr->weights_.swap(w);
  }
  static void SamplePosterior(const Solver::Options& opt, const SampleOptions& so, Problem* pr, SampleSummary* sum) {
    const size_t N = pr->ptr_.size();
    pgo_t* h = Prepare(opt, pr);
    pgo_sample_options o;
    pgo_sample_options_default(&o);
    o.rtol = so.rtol;
    o.max_iters = so.max_iters;
    o.samples_per_pass = so.samples_per_pass;
    o.solver = so.direct ? 1 : 0;
    o.first_sample = so.first_sample;
    o.seed = so.seed;
    sum->covariance.assign(9 * N, 0.0);
    sum->samples.assign(so.keep_samples ? (size_t)std::max(so.num_samples, 0) * 3 * N : 0, 0.0);
    const int st = pgo_posterior_sample(h, so.num_samples, &o, so.keep_samples ? sum->samples.data() : nullptr, sum->covariance.data(), &sum->report);
    const std::string msg = st != PGO_OK ? std::string(pgo_last_error()) : std::string();
    pgo_destroy(h);
    if (st != PGO_OK) throw std::runtime_error(std::string("pgo: ") + pgo_strerror(st) + ": " + msg);
  }
  // the parameter blocks moved, in place, to the chordal start; constant blocks are not moved
  static void ChordalInit(const Solver::Options& opt, const ChordalOptions& co, Problem* pr, ChordalSummary* sum) {
    const int32_t N = (int32_t)pr->ptr_.size();
    const size_t E = pr->ia_.size();
    pgo_t* h = Prepare(opt, pr);
    pgo_chordal_options o;
    pgo_chordal_options_default(&o);
    o.rtol = co.rtol;
    o.mag_min = co.mag_min;
    o.max_iters = co.max_iters;
    o.check_every = co.check_every;
    o.rounds = co.rounds;
    o.reject_xy = co.reject_xy;
    o.reject_th = co.reject_th;
    o.apply_weights = co.apply_weights ? 1 : 0;
    o.commit = 1;
    ChordalSummary local;
    ChordalSummary* cs = sum ? sum : &local;
    cs->residuals.assign(2 * E, 0.0);
    std::vector<double> poses((size_t)3 * N), w(E, 1.0);
    int st = pgo_chordal_init(h, &o, poses.data(), E ? cs->residuals.data() : nullptr, &cs->s);
    if (st == PGO_OK && co.apply_weights && E > 0) st = pgo_get_edge_weights(h, w.data());
    const std::string msg = st != PGO_OK ? std::string(pgo_last_error()) : std::string();
    pgo_destroy(h);
    if (st != PGO_OK) throw std::runtime_error(std::string("pgo: ") + pgo_strerror(st) + ": " + msg);
    for (int32_t i = 0; i < N; ++i)
      for (int k = 0; k < 3; ++k) pr->ptr_[i][k] = poses[3 * (size_t)i + k];
    if (co.apply_weights) pr->weights_.swap(w);
  }
  // Hierarchical initialisation (include/pgo.h): the problem's graph coarsened at `stride`, the coarse graph solved exactly (the
  // problem's METHOD, pcg_rtol 1e-10, everything else left to the library; a constant block that is a key pose stays the
  // constant one), the result prolonged and written into the caller's parameter blocks in place -- the start of the Solve
  // that follows.  Constant blocks are not moved.  information: pgo_coarsen_info -- the coarse graph carries the information
  // matrices propagated through the composition (unit fine information: a Problem holds none) and the coarse solve runs with
  // info_weighting = 1; residual block weights must then be 0 or 1 and are passed as pgo_set_active.
  static void InitializeHierarchical(const Solver::Options& opt, Problem* pr, int stride, Solver::Summary* coarse_sum, bool information) {
    pgo_t* h = Prepare(opt, pr);
    pgo_graph* cg = nullptr;
    pgo_t* ch = nullptr;
    // (a problem with residual block weights: every coarse edge takes the weight of the block it came from)
    const int32_t E = (int32_t)pr->ia_.size();
    std::vector<int32_t> origin(pr->weights_.empty() ? 0 : (size_t)E);
    int32_t n_coarse = 0;
    int st = information ? pgo_coarsen_info(h, stride, &cg, origin.empty() ? nullptr : origin.data(), nullptr, (int32_t)origin.size(), &n_coarse)
                         : pgo_coarsen(h, stride, &cg, origin.empty() ? nullptr : origin.data(), (int32_t)origin.size(), &n_coarse);
    Solver::Summary local;
    Solver::Summary* cs = coarse_sum ? coarse_sum : &local;
    if (st == PGO_OK) {
      pgo_options o;
      pgo_options_default(&o);
      o.method = pr->any_sc_ ? 2 : (pr->any_dcs_ ? 1 : 0);
      o.pcg_rtol = 1e-10;
      o.fixed_pose = pr->fixed_ < 0 ? pr->fixed_ : (pr->fixed_ % stride == 0 ? pr->fixed_ / stride : 0);
      o.info_weighting = information ? 1 : 0;
      st = pgo_create_from_graph(&ch, cg, &o, nullptr, opt.device);
    }
    bool binary = true;
    if (st == PGO_OK && !origin.empty()) {
      std::vector<double> cw((size_t)n_coarse, 1.0);
      for (int32_t e = 0; e < n_coarse; ++e)
        if (origin[e] >= 0 && (size_t)origin[e] < pr->weights_.size()) cw[e] = pr->weights_[origin[e]];
      if (information) {   // (the weight plane refuses info_weighting = 1)
        std::vector<uint8_t> on((size_t)n_coarse);
        for (int32_t e = 0; e < n_coarse; ++e) {
          binary = binary && (cw[e] == 0.0 || cw[e] == 1.0);
          on[e] = cw[e] != 0.0;
        }
        if (binary) st = pgo_set_active(ch, on.data(), nullptr);
      } else {
        st = pgo_set_edge_weights(ch, cw.data());
      }
    }
    if (!binary) {
      pgo_destroy(ch);
      pgo_graph_free(cg);
      pgo_destroy(h);
      throw std::invalid_argument("InitializeHierarchical: information = true carries residual block weights 0 and 1 only");
    }
    if (st == PGO_OK) st = pgo_solve(ch, &cs->s);
    std::vector<double> X;
    if (st == PGO_OK) {
      X.resize((size_t)3 * pgo_graph_num_poses(cg));
      st = pgo_get_poses(ch, X.data());
    }
    if (st == PGO_OK) {
      cs->iterations.resize((size_t)pgo_num_iter_records(ch));
      st = pgo_get_iter_records(ch, cs->iterations.data(), (int32_t)cs->iterations.size());
      cs->num_parameter_blocks = pgo_graph_num_poses(cg);
      cs->num_residual_blocks = pgo_graph_num_edges(cg);
    }
    if (st == PGO_OK) st = pgo_prolong(h, stride, X.data());
    const std::string msg = st != PGO_OK ? std::string(pgo_last_error()) : std::string();
    if (ch) pgo_destroy(ch);
    pgo_graph_free(cg);
    const int32_t N = (int32_t)pr->ptr_.size();
    std::vector<double> poses((size_t)3 * N);
    if (st == PGO_OK) st = pgo_get_poses(h, poses.data());
    pgo_destroy(h);
    if (st != PGO_OK) throw std::runtime_error(std::string("pgo: ") + pgo_strerror(st) + ": " + (msg.empty() ? pgo_last_error() : msg));
    for (int32_t i = 0; i < N; ++i)
      for (int k = 0; k < 3; ++k) pr->ptr_[i][k] = poses[3 * (size_t)i + k];
  }
  // The layer managers' pattern (src/simple_layer_manager.cpp:457-622: one ceres::Solve per candidate layer / window).
  // ONE batched handle (pgo_batch_*: a workgroup per problem, per-problem LM state on one launch sequence) when every
  // problem uses the same plain / DCS functor, loss and anchor index; else a pool of host threads over ordinary handles.
  static bool BatchEligible(const std::vector<Problem*>& prs) {
    if (prs.empty()) return false;
    for (Problem* pr : prs)
      if (pr->any_sc_ || pr->any_dcs_ != prs[0]->any_dcs_ || !SameLosses(pr, prs[0]) || pr->fixed_ != prs[0]->fixed_ ||
          pr->ptr_.empty() || !ConstantMask(pr).empty() ||   // (several constant blocks: ordinary handles, pgo_set_active)
          !pr->prior_pose_.empty())                          // (pose priors: there is no batch entry point for them)
        return false;
    return true;
  }
  static void SolveBatch(const Solver::Options& opt, const std::vector<Problem*>& prs, std::vector<Solver::Summary>* sums,
                         int max_concurrency) {
    if (BatchEligible(prs)) {
      std::vector<pgo_graph*> gs(prs.size(), nullptr);
      pgo_batch_t* b = nullptr;
      auto cleanup = [&] {
        for (pgo_graph* g : gs) pgo_graph_free(g);
        if (b) pgo_batch_destroy(b);
      };
      try {
        for (size_t i = 0; i < prs.size(); ++i) {
          Problem* pr = prs[i];
          const int32_t N = (int32_t)pr->ptr_.size(), E = (int32_t)pr->ia_.size();
          std::vector<double> poses((size_t)3 * N);
          for (int32_t k = 0; k < N; ++k)
            for (int c = 0; c < 3; ++c) poses[3 * (size_t)k + c] = pr->ptr_[k][c];
          check(pgo_graph_from_arrays(N, poses.data(), E, pr->ia_.data(), pr->ib_.data(), pr->meas_.data(), nullptr, pr->kind_.data(), &gs[i]));
        }
        pgo_options o;
        pgo_options_default(&o);
        o.method = prs[0]->any_dcs_ ? 1 : 0;
        o.fixed_pose = prs[0]->fixed_;
        o.max_iters = opt.max_num_iterations;
        o.ftol = opt.function_tolerance;
        o.gtol = opt.gradient_tolerance;
        o.ptol = opt.parameter_tolerance;
        o.radius0 = opt.initial_trust_region_radius;
        o.pcg_rtol = opt.pcg_rtol;
        o.linear_solver = opt.linear_solver_type == BLOCK_JACOBI_PCG ? 1 : 0;
        o.pcg_max_iters = opt.pcg_max_iters;
        int st = pgo_batch_create(&b, (int32_t)prs.size(), gs.data(), &o, opt.device);
        if (st != PGO_ERR_UNSUPPORTED) {
          check(st);
          std::vector<uint8_t> cls;   // the problems' blocks concatenated
          for (Problem* pr : prs) cls.insert(cls.end(), pr->class_.begin(), pr->class_.end());
          const std::vector<pgo_loss> L = LossTable(prs[0]);
          check(pgo_batch_set_losses(b, (int32_t)L.size(), L.data(), cls.empty() ? nullptr : cls.data()));
          std::vector<pgo_summary> raw(prs.size());
          check(pgo_batch_solve(b, raw.data()));
          sums->assign(prs.size(), Solver::Summary());
          for (size_t i = 0; i < prs.size(); ++i) {
            Problem* pr = prs[i];
            const int32_t N = (int32_t)pr->ptr_.size();
            std::vector<double> poses((size_t)3 * N);
            check(pgo_batch_get_poses(b, (int32_t)i, poses.data()));
            for (int32_t k = 0; k < N; ++k)
              for (int c = 0; c < 3; ++c) pr->ptr_[k][c] = poses[3 * (size_t)k + c];
            Solver::Summary& sm = (*sums)[i];
            sm.s = raw[i];
            sm.iterations.resize((size_t)pgo_batch_num_iter_records(b, (int32_t)i));
            check(pgo_batch_get_iter_records(b, (int32_t)i, sm.iterations.data(), (int32_t)sm.iterations.size()));
            sm.num_parameter_blocks = N;
            sm.num_residual_blocks = (int)pr->ia_.size();
          }
          cleanup();
          return;
        }
      } catch (...) {
        cleanup();
        throw;
      }
      cleanup();  // a problem the batched handle does not take (a row with > 256 edges): the thread pool below
    }
    std::vector<pgo_t*> hs;
    try {
      for (Problem* pr : prs) hs.push_back(Prepare(opt, pr));
    } catch (...) {
      for (pgo_t* h : hs) pgo_destroy(h);
      throw;
    }
    std::vector<pgo_summary> raw(prs.size());
    const int st = pgo_solve_batch(hs.data(), (int32_t)hs.size(), raw.data(), max_concurrency);
    const std::string msg = st != PGO_OK ? std::string(pgo_last_error()) : std::string();
    sums->assign(prs.size(), Solver::Summary());
    for (size_t i = 0; i < prs.size(); ++i) {
      (*sums)[i].s = raw[i];
      if (st == PGO_OK) Finish(prs[i], hs[i], PGO_OK, &(*sums)[i]);
      else pgo_destroy(hs[i]);
    }
    if (st != PGO_OK) throw std::runtime_error(std::string("pgo: ") + pgo_strerror(st) + ": " + msg);
  }
};

inline void Solve(const Solver::Options& opt, Problem* problem, Solver::Summary* summary) { SolverAccess::Solve(opt, problem, summary); }
// the parameter blocks moved, in place, to the prolonged solution of the problem's coarse graph at `stride` (pgo_coarsen ->
// solve -> pgo_prolong); call Solve next.  coarse_summary (or nullptr) receives the coarse solve's summary.  information: the
// coarse graph carries propagated information matrices (pgo_coarsen_info) and is solved with info_weighting = 1
inline void InitializeHierarchical(Problem* problem, int stride, const Solver::Options& opt = Solver::Options(),
                                   Solver::Summary* coarse_summary = nullptr, bool information = false) {
  SolverAccess::InitializeHierarchical(opt, problem, stride, coarse_summary, information);
}
// Solve with graduated non-convexity: the parameter blocks end at the final solve's poses, summary->weights at the weights
inline void SolveGnc(const Solver::Options& opt, const GncOptions& gnc, Problem* problem, GncSummary* summary) {
  SolverAccess::SolveGnc(opt, gnc, problem, summary);
}
// Solve with max-mixture blocks: rounds of selection and short solves until the selection stands, then a final solve; the
// parameter blocks end at its poses, summary->selection at the components in force, summary->weights at their information scales
inline void SolveMixture(const Solver::Options& opt, const MixtureOptions& mixture, Problem* problem, MixtureSummary* summary) {
  SolverAccess::SolveMixture(opt, mixture, problem, summary);
}
// Judge the problem's loop blocks by odometry cycle consistency; with options.apply the verdict becomes the problem's residual
// block weights, which every Solve, SolveGnc and InitializeHierarchical that follows honours
inline void LoopSupport(const Solver::Options& opt, const LoopSupportOptions& options, Problem* problem, LoopSupportSummary* summary) {
  SolverAccess::LoopSupport(opt, options, problem, summary);
}
// The parameter blocks moved, in place, to the chordal start (pgo_chordal_init: no estimate plays a part except on the constant
// blocks); the problem's residual block weights are honoured, and with options.apply_weights the blocks the reject rounds
// dropped get the weight 0.  Call Solve next.
inline void ChordalInit(const Solver::Options& opt, const ChordalOptions& options, Problem* problem, ChordalSummary* summary = nullptr) {
  SolverAccess::ChordalInit(opt, options, problem, summary);
}
// All-pose marginal covariances by posterior sampling at the problem's current parameter blocks (after Solve: the estimate's);
// METHOD 2 problems (switchable blocks) are refused
inline void SamplePosterior(const Solver::Options& opt, const SampleOptions& options, Problem* problem, SampleSummary* summary) {
  SolverAccess::SamplePosterior(opt, options, problem, summary);
}
// many independent problems at once; summaries->size() == problems.size() afterwards
inline void SolveBatch(const Solver::Options& opt, const std::vector<Problem*>& problems, std::vector<Solver::Summary>* summaries,
                       int max_concurrency = 8) {
  SolverAccess::SolveBatch(opt, problems, summaries, max_concurrency);
}

}  // namespace pgo

#endif
