// Pose marginal covariances (ceres::Covariance with a constant parameter block): Sigma = (J'J)^-1 at the handle's current
// poses, by PCG on 3 x (poses per pass) right-hand sides at once (covariance.hip.h), and the loop-edge gate on the same
// system (pgo_edge_gate: right-hand sides S J' of candidate edges, three columns each, P = J Sigma J' on the device).  The system is the undamped one of the LM
// loop, A = S J'J S + I_fixed (k_prepare at radius = infinity), right-hand side S e_k, Sigma = S X.  The preconditioner is the
// handle's own (one level + the coarse level where the handle has it), set up for D'D = 0 and applied column by column.
// pgo_edge_gate_joint is the same call plus the joint covariance of all candidates from the solved columns (k_gate_cross after
// every pass) and the sequential elimination on it (k_gate_joint_step, one launch per candidate).
// With pgo_covariance_options.solver = 1 the columns go through the handle's direct solve instead (Session::pass_direct):
// its factorisation once per call at D'D = 0, up to 768 columns per pass, iterative refinement against the same A.
// pgo_posterior_sample is the same session on dense right-hand sides b = S J' eps (sample.hip.h): one column per draw
// delta ~ N(0, (J'J)^-1), and the second moment of the draws per pose.
#include <functional>

#include "solver_handle.hip.h"
#include "covariance.hip.h"
#include "sample.hip.h"

namespace {

// largest true relative residual |S e - A x| / |S e| a column may end with when residual replacement no longer lowers it
// (the double-precision floor of an ill-conditioned system: MIT's columns stop near 2e-7 at rtol 1e-10, INTEL with information
// weighting near 1.5e-6)
constexpr double COV_RES_FLOOR_MAX = 1e-5;
// solver = 1: columns per pass at most, the memory the panels of a pass may take, refinement steps beyond the first
constexpr int DIRECT_COLS_MAX = 768;
constexpr int64_t DIRECT_PANEL_BYTES = (int64_t)512 << 20;
constexpr int DIRECT_EXTRA_STEPS = 3;

struct DevScratch {   // buffers of one call, freed on every return path
  std::vector<void*> p;
  ~DevScratch() {
    for (void* q : p) (void)hipFree(q);
  }
  template <class T>
  int alloc(T** out, int64_t n) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, (size_t)std::max<int64_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return fail(PGO_ERR_NOMEM, std::string("covariance: hipMalloc: ") + hipGetErrorString(e));
    p.push_back(q);
    *out = (T*)q;
    return PGO_OK;
  }
};

int spmm(pgo_handle* h, int m, int64_t ld, const double* p, double* y, double* part, int g) {
  for (int c0 = 0; c0 < m; c0 += dev::COV_MC) {
    dev::SpmmArgs A;
    A.inc_ptr = h->inc_ptr;
    A.inc_col = h->inc_col;
    A.hoff = h->hoff;
    A.hd = h->hd;
    A.d2 = h->d2;
    A.n = h->S.n_loc;
    A.c0 = c0;
    A.nc = std::min(dev::COV_MC, m - c0);
    A.ld = ld;
    A.p = p;
    A.y = y;
    A.part = part;
    if (A.nc <= 3) hipLaunchKernelGGL(dev::k_spmm<3>, dim3(g), dim3(dev::WG), 0, h->stream, A);
    else if (A.nc <= 6) hipLaunchKernelGGL(dev::k_spmm<6>, dim3(g), dim3(dev::WG), 0, h->stream, A);
    else if (A.nc <= 12) hipLaunchKernelGGL(dev::k_spmm<12>, dim3(g), dim3(dev::WG), 0, h->stream, A);
    else hipLaunchKernelGGL(dev::k_spmm<24>, dim3(g), dim3(dev::WG), 0, h->stream, A);
    PGOC(h->check_launch("k_spmm"));
  }
  return PGO_OK;
}

// The rigid-body coarse level for handles that were created without it (direct solves, the inexact mode, pcg_coarse_poses = 0)
// on graphs of >= 512 poses: the plan sized it (plan.co_cov, plan_coarse_for_covariance); its structure is built once, here, and
// used by covariance calls only -- the LM loop's plan does not know it.
int coarse_for_covariance(pgo_handle* h) {
  if (h->plan.co.on || h->co_cov_ready || h->S.n_loc < 512) return PGO_OK;
  if (h->plan.co_cov.no) return fail(h->plan.co_cov.no.status, h->plan.co_cov.no.why);
  if (!h->plan.co_cov.on) return PGO_OK;
  PGOC(h->coarse_build(0, nullptr, nullptr));   // (one rank: the edge lists are not read)
  h->co_cov_ready = true;
  return PGO_OK;
}

// the level is on for the duration of a covariance call only
struct CoarseOn {
  pgo_handle* h;
  explicit CoarseOn(pgo_handle* hh) : h(hh) { h->co_for_call = h->co_cov_ready; }
  ~CoarseOn() { h->co_for_call = false; }
};

// the undamped system at the current poses: linearisation (when the LM loop's is not current), METHOD 2's switch
// elimination without damping, D'D = 0 and the preconditioner for it.  Afterwards the LM loop's own set-up is redone by its
// next iteration from unchanged inputs (prepare_system; METHOD 2: refresh_switch_system), so its results do not change.
int setup_system(pgo_handle* h, bool with_preconditioner) {
  if (!h->lin_valid) {   // (not for METHOD 2: refused earlier) Jacobi scales and J'J at the current poses, as pgo_lm_begin
    PGOC(h->launch_jacobi_scale(0));
    PGOC(h->linearize(false));
    if (h->opt.jacobi_scaling) {
      PGOC(h->launch_jacobi_scale(1));
      PGOC(h->linearize(true));
    }
  }
  const double undamped = std::numeric_limits<double>::infinity();
  if (h->has_sw) {   // switches eliminated per edge with zero damping: the pose marginal of the joint system
    h->sw_fresh = false;   // the next LM iteration re-assembles for its radius (refresh_switch_system)
    PGOC(h->switch_prepare(undamped));
    PGOC(h->assemble_enqueue());
  }
  return h->prepare_system(undamped, with_preconditioner);   // (a handle on the direct solve does not set the preconditioner up per iteration)
}

// the right-hand sides of one pass: unit vectors S e_rows[c] (pgo_pose_covariance), or with rec != nullptr the sparse
// columns S J' of the candidates cand[0 .. m / 3) (pgo_edge_gate), or with panel != nullptr the dense columns of a panel
// of their own, column c at panel + c * ld (pgo_posterior_sample)
struct PassRhs {
  const int32_t* rows = nullptr;
  const dev::GateRec* rec = nullptr;
  const int32_t* cand = nullptr;
  const double* panel = nullptr;
};

// One call on the undamped system: the checks and the set-up both entry points share, the PCG panels, and the solve of a pass.
struct Session {
  pgo_handle* h;
  std::string fn;             // the entry point, for messages
  pgo_covariance_options o;
  int64_t N = 0, n3 = 0, ld = 0;
  int g = 1, gs = 1, gp = 1;  // grids of the vector kernels, of k_spmm, and the larger of both
  DevScratch buf;
  double *X = nullptr, *R = nullptr, *Z = nullptr, *P = nullptr, *AP = nullptr, *part_a = nullptr, *part_b = nullptr;
  // solver = 1: the factorisation's launch arguments, the row-major panel of the sweeps and its companions, the pass width
  bool direct = false;
  pgo_handle::DirectLaunch dl;
  pgo_handle::DirectPanel panel = {};
  double* part_c = nullptr;
  int direct_cols = 0;
  dev::CovCol* cs = nullptr;
  uint8_t* rmask = nullptr;
  std::vector<dev::CovCol> hc;
  std::vector<double> hpart;
  std::unique_ptr<CoarseOn> coarse_on;
  int passes = 0, it_max = 0;
  int64_t it_total = 0;
  double rel_max = 0.0;

  Session(pgo_handle* hh, const char* name) : h(hh), fn(name) {}

  // options and the cases that are refused
  int check(const pgo_covariance_options* opt_or_null) {
    if (opt_or_null) o = *opt_or_null;
    else pgo_covariance_options_default(&o);
    const long long kp = knob("cov_poses_per_pass");
    if (kp >= 0) o.poses_per_pass = (int32_t)kp;
    if (o.solver != 0 && o.solver != 1) return fail(PGO_ERR_INVALID_ARG, fn + ": solver is 0 (PCG) or 1 (the handle's direct solve)");
    direct = o.solver == 1;
    if (!(o.rtol > 0.0) || !std::isfinite(o.rtol) || (!direct && (o.max_iters < 1 || o.poses_per_pass < 1 || o.poses_per_pass > dev::COV_MAX_COLS / 3)))
      return fail(PGO_ERR_INVALID_ARG, fn + ": rtol > 0, max_iters >= 1 and poses_per_pass in 1..16 required");
    const long long kc = direct ? knob("cov_direct_cols") : -1;
    if (kc >= 0 && (kc < 3 || kc > DIRECT_COLS_MAX || kc % 3 != 0))
      return fail(PGO_ERR_INVALID_ARG, fn + ": the cov_direct_cols knob is a multiple of 3 in 3..768");
    direct_cols = (int)kc;
    if ((h->comm && h->comm->world > 1) || h->co_multi()) return fail(PGO_ERR_UNSUPPORTED, fn + ": one rank only");
    if (h->batch_mode) return fail(PGO_ERR_UNSUPPORTED, fn + ": not on batched handles");
    // information weighting: even the columns whose true residual reaches 1e-5 differ from a sparse direct inverse by ~1e-3 on
    // INTEL (others stall at 2e-5) -- refused rather than returning blocks of that quality
    if (h->info_mode) return fail(PGO_ERR_UNSUPPORTED, fn + ": not available with info_weighting = 1");
    if (!h->has_anchor())   // (opt.fixed_pose, or a pose made constant by pgo_set_active)
      return fail(PGO_ERR_UNSUPPORTED, fn + ": fixed_pose = -1 leaves the gauge free (J'J is singular)");
    // solver = 1 never falls back: a PCG handle, or a handle that pgo_set_active took off the direct solve (a cut chain)
    if (direct && !(h->direct() && h->dl_ready))
      return fail(PGO_ERR_UNSUPPORTED, fn + ": solver = 1 needs a handle on the direct solve (pgo_handle_info.linear_solver = 2)");
    N = h->S.n_poses;
    return PGO_OK;
  }
  int need_switches() {
    if (h->has_sw && !h->lin_valid)
      return fail(PGO_ERR_INVALID_ARG, fn + ": METHOD 2 needs the switches of a solve: call pgo_lm_begin or pgo_solve first");
    return PGO_OK;
  }
  int64_t internal(int64_t i) const { return h->perm.empty() ? i : (int64_t)h->perm[i]; }
  int64_t caller(int64_t k) const {   // internal row -> caller's pose
    if (h->perm.empty()) return k;
    for (int64_t i = 0; i < N; ++i)
      if (h->perm[i] == k) return i;
    return k;
  }

  // finite poses, the coarse level, the undamped system and its preconditioner, a positive diagonal on every row
  int open() {
    HIPC(hipSetDevice(h->device));
    {   // a non-finite pose is named before anything is evaluated at it
      std::vector<double> x((size_t)3 * N);
      HIPC(hipMemcpyAsync(x.data(), h->poses, x.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      PGOC(h->sync());
      for (int64_t k = 0; k < N; ++k)
        if (!std::isfinite(x[3 * k]) || !std::isfinite(x[3 * k + 1]) || !std::isfinite(x[3 * k + 2]))
          return fail(PGO_ERR_NUMERIC, fn + ": pose " + std::to_string(caller(k)) + " is not finite");
    }
    if (!direct) {   // (the coarse level is the preconditioner's: not built for the direct solve)
      PGOC(coarse_for_covariance(h));
      coarse_on.reset(new CoarseOn(h));
    }
    PGOC(setup_system(h, !direct));
    n3 = 3 * N;
    ld = n3;
    g = std::min(std::max(1, (int)((n3 + dev::WG - 1) / dev::WG)), 1024);
    gs = std::min(std::max(1, (int)((N + dev::WG - 1) / dev::WG)), 1024);
    gp = std::max(g, gs);
    // every row of A needs a positive diagonal: a pose without edges has none
    DevScratch tmp;
    int32_t* bad = nullptr;
    PGOC(tmp.alloc(&bad, gs));
    hipLaunchKernelGGL(dev::k_cov_check_rows<>, dim3(gs), dim3(dev::WG), 0, h->stream, (int)N, (const double*)h->hd, (const double*)h->d2, bad);
    PGOC(h->check_launch("k_cov_check_rows"));
    std::vector<int32_t> hb((size_t)gs);
    HIPC(hipMemcpyAsync(hb.data(), bad, hb.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    PGOC(h->sync());
    const int32_t first = *std::min_element(hb.begin(), hb.end());
    if (first < N)
      return fail(PGO_ERR_NUMERIC, fn + ": pose " + std::to_string(caller(first)) +
                                       " has a singular diagonal block in J'J (no edge constrains it, or a non-finite Jacobian)");
    // the direct solve's factorisation of this system, once per call (its dense column: the gradient, not used).  What it
    // overwrites (the dl_* buffers) every direct solve of the LM loop computes afresh.
    if (direct) PGOC(h->direct_factor(h->gs, false, &dl));
    return PGO_OK;
  }

  // poses (pgo_pose_covariance) or candidates (pgo_edge_gate) per pass.  solver = 1: the library's choice, 3 x this <= 768
  // columns, fewer where the panels of a pass would exceed 512 MiB; poses_per_pass is not read.
  int per_pass() const {
    if (!direct) return o.poses_per_pass;
    if (direct_cols > 0) return direct_cols / 3;
    const int64_t n3_ = 3 * N, g_ = std::max<int64_t>(1, std::min<int64_t>((n3_ + dev::WG - 1) / dev::WG, 1024));   // (= gp: g >= gs)
    const int64_t per_col = (int64_t)sizeof(double) * (4 * n3_ + 6 * h->plan.dl.dl_nseg + h->plan.dl.dl_nU + 2 * h->plan.dl.dl_Kp + 3 * g_);
    return (int)std::max<int64_t>(1, std::min<int64_t>(DIRECT_COLS_MAX, DIRECT_PANEL_BYTES / per_col) / 3);
  }

  // the panels of a pass of up to mcap columns
  int alloc(int mcap) {
    PGOC(buf.alloc(&X, mcap * ld));
    PGOC(buf.alloc(&R, mcap * ld));
    if (direct) {
      const int64_t ldt = ((int64_t)mcap + 63) / 64 * 64;
      panel.ld = (int)ldt;
      PGOC(buf.alloc(&AP, mcap * ld));
      PGOC(buf.alloc(&panel.T, n3 * ldt));
      PGOC(buf.alloc(&panel.E, (int64_t)h->plan.dl.dl_nseg * 3 * ldt));
      PGOC(buf.alloc(&panel.E2, (int64_t)h->plan.dl.dl_nseg * 3 * ldt));
      PGOC(buf.alloc(&panel.Wm, (int64_t)std::max(1, h->plan.dl.dl_nU) * ldt));
      PGOC(buf.alloc(&panel.G, (int64_t)h->plan.dl.dl_Kp * ldt));
      PGOC(buf.alloc(&panel.Y, (int64_t)h->plan.dl.dl_Kp * ldt));
      PGOC(buf.alloc(&part_a, (int64_t)mcap * gp));
      PGOC(buf.alloc(&part_b, (int64_t)mcap * gp));
      PGOC(buf.alloc(&part_c, (int64_t)mcap * gp));
      PGOC(buf.alloc(&rmask, mcap));
      return PGO_OK;
    }
    PGOC(buf.alloc(&Z, mcap * ld));
    PGOC(buf.alloc(&P, mcap * ld));
    PGOC(buf.alloc(&AP, mcap * ld));
    PGOC(buf.alloc(&part_a, (int64_t)mcap * gp));
    PGOC(buf.alloc(&part_b, (int64_t)mcap * gp));
    PGOC(buf.alloc(&cs, mcap));
    PGOC(buf.alloc(&rmask, mcap));
    hc.resize((size_t)mcap);
    return PGO_OK;
  }

  int launch_rhs(int m, const PassRhs& B) {
    double* p0 = direct ? AP : P;   // (solver = 1 has no search directions: the kernel's zeros go into the product's panel)
    if (B.panel)
      hipLaunchKernelGGL(dev::k_cov_rhs<dev::RhsDense>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, dev::RhsDense{B.panel, ld}, X, R, p0, part_a);
    else if (B.rec)
      hipLaunchKernelGGL(dev::k_cov_rhs<dev::RhsSparse>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, dev::RhsSparse{B.rec, B.cand, h->scale}, X, R, p0, part_a);
    else
      hipLaunchKernelGGL(dev::k_cov_rhs<dev::RhsUnit>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, dev::RhsUnit{B.rows, h->scale}, X, R, p0, part_a);
    return h->check_launch("k_cov_rhs");
  }
  int launch_resid(int m, const PassRhs& B) {
    if (B.panel)
      hipLaunchKernelGGL(dev::k_cov_resid<dev::RhsDense>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, dev::RhsDense{B.panel, ld}, (const double*)AP, part_b);
    else if (B.rec)
      hipLaunchKernelGGL(dev::k_cov_resid<dev::RhsSparse>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, dev::RhsSparse{B.rec, B.cand, h->scale}, (const double*)AP, part_b);
    else
      hipLaunchKernelGGL(dev::k_cov_resid<dev::RhsUnit>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, dev::RhsUnit{B.rows, h->scale}, (const double*)AP, part_b);
    return h->check_launch("k_cov_resid");
  }
  void launch_replace(int m, const PassRhs& B) {
    if (B.panel)
      hipLaunchKernelGGL(dev::k_cov_replace<dev::RhsDense>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, dev::RhsDense{B.panel, ld}, (const double*)AP, R,
                         (const uint8_t*)rmask);
    else if (B.rec)
      hipLaunchKernelGGL(dev::k_cov_replace<dev::RhsSparse>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, dev::RhsSparse{B.rec, B.cand, h->scale}, (const double*)AP, R,
                         (const uint8_t*)rmask);
    else
      hipLaunchKernelGGL(dev::k_cov_replace<dev::RhsUnit>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, dev::RhsUnit{B.rows, h->scale}, (const double*)AP, R,
                         (const uint8_t*)rmask);
  }

  // A X = B for the m columns of one pass (every one a non-zero right-hand side): start, PCG in chunks, the true residual,
  // residual replacement and restart.  who(c) names column c's pose or candidate in messages.  X holds the solution.
  int pass(int m, const PassRhs& B, const std::function<std::string(int)>& who) {
    if (direct) return pass_direct(m, B, who);
    const int every = std::max(1, h->opt.pcg_check_every);
    // start: X = 0, R = B, Z = M^-1 R, P = Z
    // columns known stopped at the latest host check: no preconditioner apply.  (The apply is the LM loop's start-up kernel: it
    // also overwrites the loop's per-solve vectors y, r and the gather vector, which every PCG solve initialises afresh.)
    std::vector<uint8_t> hdone((size_t)m, 0);
    auto precond_open = [&]() -> int {
      for (int c = 0; c < m; ++c)
        if (!hdone[c]) PGOC(h->precondition(R + c * ld, Z + c * ld, nullptr, h->part[3]));
      return PGO_OK;
    };
    PGOC(launch_rhs(m, B));
    PGOC(precond_open());
    // (k_cov_dot skips done columns: cs must read "running" before the start kernel has written it)
    HIPC(hipMemsetAsync(cs, 0, (size_t)m * sizeof(dev::CovCol), h->stream));
    hipLaunchKernelGGL(dev::k_cov_dot<>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, (const double*)R, (const double*)Z, (const dev::CovCol*)cs, part_b);
    hipLaunchKernelGGL(dev::k_cov_start<>, dim3(m), dim3(dev::WG), 0, h->stream, cs, (const double*)part_a, (const double*)part_b, g, o.rtol);
    hipLaunchKernelGGL(dev::k_cov_pupdate<>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, (const dev::CovCol*)cs, (const double*)Z, P);
    PGOC(h->check_launch("covariance PCG start"));
    int it = 0;
    std::vector<double> res_prev((size_t)m, std::numeric_limits<double>::infinity()), res((size_t)m, 0.0);
    while (true) {
      // PCG until every column has stopped on its recurrence residual
      while (true) {
        const int chunk = std::min(every, o.max_iters - it);
        for (int s = 0; s < chunk; ++s) {
          PGOC(spmm(h, m, ld, P, AP, part_a, gs));
          hipLaunchKernelGGL(dev::k_cov_alpha<>, dim3(m), dim3(dev::WG), 0, h->stream, cs, (const double*)part_a, gs);
          hipLaunchKernelGGL(dev::k_cov_update1<>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, (const dev::CovCol*)cs, X, R, (const double*)P,
                             (const double*)AP, part_a);
          PGOC(h->check_launch("k_cov_update1"));
          PGOC(precond_open());
          hipLaunchKernelGGL(dev::k_cov_dot<>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, (const double*)R, (const double*)Z, (const dev::CovCol*)cs,
                             part_b);
          hipLaunchKernelGGL(dev::k_cov_beta<>, dim3(m), dim3(dev::WG), 0, h->stream, cs, (const double*)part_a, (const double*)part_b, g);
          hipLaunchKernelGGL(dev::k_cov_pupdate<>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, (const dev::CovCol*)cs, (const double*)Z, P);
          PGOC(h->check_launch("covariance PCG iteration"));
        }
        it += chunk;
        HIPC(hipMemcpyAsync(hc.data(), cs, (size_t)m * sizeof(dev::CovCol), hipMemcpyDeviceToHost, h->stream));
        PGOC(h->sync());
        bool all = true;
        for (int c = 0; c < m; ++c) {
          if (hc[c].done >= 2)
            return fail(PGO_ERR_NUMERIC, fn + ": PCG breakdown on column " + std::to_string(c % 3) + " of " + who(c) +
                                             (hc[c].done == 2 ? " (p'Ap <= 0)" : " (r'z <= 0)"));
          hdone[c] = hc[c].done == 1;
          all = all && hdone[c];
        }
        if (all) break;
        if (it >= o.max_iters) {
          for (int c = 0; c < m; ++c)
            if (!hc[c].done)
              return fail(PGO_ERR_NUMERIC, fn + ": PCG reached max_iters = " + std::to_string(o.max_iters) + " on " + who(c) +
                                               " (relative residual " + std::to_string(std::sqrt(hc[c].rr / hc[c].bb)) + ")");
        }
      }
      // the TRUE residual |b - A x| / |b| of every column (one more product): the recurrence drifts from it on
      // ill-conditioned systems.  Columns above rtol restart from X with the true residual (residual replacement) as long
      // as that lowers it by 10 % or more.  Once it no longer does, the column has reached what double precision allows for this
      // system: accepted when that floor is <= COV_RES_FLOOR_MAX (reported in max_rel_residual), else PGO_ERR_NUMERIC.
      PGOC(spmm(h, m, ld, X, AP, part_a, gs));
      PGOC(launch_resid(m, B));
      hpart.resize((size_t)m * g);
      HIPC(hipMemcpyAsync(hpart.data(), part_b, hpart.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      PGOC(h->sync());
      std::vector<uint8_t> mask((size_t)m, 0);
      bool any = false;
      for (int c = 0; c < m; ++c) {
        double s = 0.0;
        for (int b = 0; b < g; ++b) s += hpart[(size_t)c * g + b];
        res[c] = hc[c].bb > 0.0 ? std::sqrt(s / hc[c].bb) : 0.0;
        if (!(res[c] <= o.rtol)) {
          if (!(res[c] <= 0.9 * res_prev[c]) || it >= o.max_iters) {   // no further gain from a replacement
            if (res[c] <= COV_RES_FLOOR_MAX) continue;
            char msg[200];
            snprintf(msg, sizeof msg, ": the true residual of %s stalls at %.3e relative (rtol %.1e)", who(c).c_str(), res[c], o.rtol);
            return fail(PGO_ERR_NUMERIC, fn + msg);
          }
          mask[c] = 1;
          hdone[c] = 0;
          any = true;
        }
      }
      if (!any) break;
      res_prev = res;
      HIPC(hipMemcpyAsync(rmask, mask.data(), (size_t)m, hipMemcpyHostToDevice, h->stream));
      launch_replace(m, B);
      hipLaunchKernelGGL(dev::k_cov_reopen<>, dim3(1), dim3(64), 0, h->stream, cs, (const uint8_t*)rmask, m);
      PGOC(h->check_launch("k_cov_replace"));
      PGOC(precond_open());
      hipLaunchKernelGGL(dev::k_cov_dot<>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, (const double*)R, (const double*)Z, (const dev::CovCol*)cs, part_b);
      hipLaunchKernelGGL(dev::k_cov_restart<>, dim3(m), dim3(dev::WG), 0, h->stream, cs, (const double*)part_b, g, (const uint8_t*)rmask);
      hipLaunchKernelGGL(dev::k_cov_pupdate<>, dim3(g, m), dim3(dev::WG), 0, h->stream, n3, ld, (const dev::CovCol*)cs, (const double*)Z, P);
      PGOC(h->check_launch("covariance PCG restart"));
      PGOC(h->sync());   // (mask is read by the kernels above)
    }
    for (int c = 0; c < m; ++c) {
      it_max = std::max(it_max, hc[c].iters);
      it_total += hc[c].iters;
      rel_max = std::max(rel_max, res[c]);
    }
    ++passes;
    return PGO_OK;
  }

  // The same, solver = 1:  X = A^-1 B by the handle's direct solve (direct_panel_solve) and iterative refinement against A
  // (k_spmm):  one step always, then the TRUE residual of every column; a column above rtol takes another step, up to three
  // more, while the last one lowered its residual by 10 % or more (the replacement rule of pass()); acceptance as there.
  // A column decides from its own residual only, and a column that rests takes no part in a step (the mask).
  int pass_direct(int m, const PassRhs& B, const std::function<std::string(int)>& who) {
    std::vector<uint8_t> mask((size_t)m, 1);
    const dim3 gt((unsigned)(panel.ld / 32), (unsigned)((n3 + 31) / 32)), bt(32, 8);
    auto step = [&]() -> int {   // X += A^-1 R on the columns of rmask
      hipLaunchKernelGGL(dev::k_cov_to_panel<>, gt, bt, 0, h->stream, n3, ld, m, (const double*)R, (const uint8_t*)rmask, (int64_t)panel.ld, panel.T);
      PGOC(h->check_launch("k_cov_to_panel"));
      PGOC(h->direct_panel_solve(dl, panel));
      hipLaunchKernelGGL(dev::k_cov_from_panel<>, gt, bt, 0, h->stream, n3, ld, m, (const double*)panel.T, (int64_t)panel.ld, (const uint8_t*)rmask, X);
      return h->check_launch("k_cov_from_panel");
    };
    auto sums = [&](const double* part, std::vector<double>* out) -> int {   // per column, the partials in fixed order
      hpart.resize((size_t)m * g);
      HIPC(hipMemcpyAsync(hpart.data(), part, hpart.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      PGOC(h->sync());
      out->assign((size_t)m, 0.0);
      for (int c = 0; c < m; ++c)
        for (int b = 0; b < g; ++b) (*out)[c] += hpart[(size_t)c * g + b];
      return PGO_OK;
    };
    std::vector<double> bb, rr, res((size_t)m, 0.0), res_prev((size_t)m, std::numeric_limits<double>::infinity());
    HIPC(hipMemcpyAsync(rmask, mask.data(), (size_t)m, hipMemcpyHostToDevice, h->stream));
    PGOC(launch_rhs(m, B));   // X = 0, R = B, |B|^2
    PGOC(sums(part_a, &bb));
    PGOC(step());
    PGOC(spmm(h, m, ld, X, AP, part_c, gs));
    for (int extra = 0;; ++extra) {
      launch_replace(m, B);   // R = B - A X on the columns of mask, and their step
      PGOC(h->check_launch("k_cov_replace"));
      PGOC(step());
      PGOC(spmm(h, m, ld, X, AP, part_c, gs));
      PGOC(launch_resid(m, B));
      PGOC(sums(part_b, &rr));
      bool any = false;
      for (int c = 0; c < m; ++c) {
        res[c] = bb[c] > 0.0 ? std::sqrt(rr[c] / bb[c]) : 0.0;
        mask[c] = 0;
        if (res[c] <= o.rtol) continue;
        if (extra < DIRECT_EXTRA_STEPS && res[c] <= 0.9 * res_prev[c]) {
          mask[c] = 1;
          any = true;
        } else if (!(res[c] <= COV_RES_FLOOR_MAX)) {
          char msg[260];
          snprintf(msg, sizeof msg, ": the true residual of %s is %.3e relative after %d refinement steps of the direct solve (the odometry chain "
                   "alone may be singular where J'J is not: solver = 0 still applies)", who(c).c_str(), res[c], extra + 1);
          return fail(PGO_ERR_NUMERIC, fn + msg);
        }
      }
      if (!any) break;
      res_prev = res;
      HIPC(hipMemcpyAsync(rmask, mask.data(), (size_t)m, hipMemcpyHostToDevice, h->stream));   // (read before the next sums() returns)
    }
    for (int c = 0; c < m; ++c) rel_max = std::max(rel_max, res[c]);
    ++passes;
    return PGO_OK;
  }

  void fill(pgo_covariance_report* report, int32_t columns, double t0) const {
    if (!report) return;
    report->columns = columns;
    report->passes = passes;
    report->pcg_iters_max = it_max;
    report->pcg_iters_total = (int32_t)std::min<int64_t>(it_total, INT32_MAX);
    report->max_rel_residual = rel_max;
    report->seconds = wall_s() - t0;
  }
};

}  // namespace

extern "C" {

void pgo_covariance_options_default(pgo_covariance_options* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->rtol = 1e-10;
  o->max_iters = 20000;
  o->poses_per_pass = 8;
  o->cross = 0;
}

int pgo_pose_covariance(pgo_t* h, int32_t n, const int32_t* poses, const pgo_covariance_options* opt_or_null, double* out,
                        pgo_covariance_report* report) {
  const double t0 = wall_s();
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_pose_covariance: null handle");
  if (n < 0 || (n > 0 && (!poses || !out))) return fail(PGO_ERR_INVALID_ARG, "pgo_pose_covariance: bad argument");
  Session S(h, "pgo_pose_covariance");
  PGOC(S.check(opt_or_null));
  const pgo_covariance_options& o = S.o;
  const int64_t N = S.N;
  for (int32_t k = 0; k < n; ++k)
    if (poses[k] < 0 || poses[k] >= N)
      return fail(PGO_ERR_INVALID_ARG, "pgo_pose_covariance: pose index " + std::to_string(poses[k]) + " (entry " + std::to_string(k) + ") out of range");
  PGOC(S.need_switches());
  if (report) memset(report, 0, sizeof *report);
  if (n == 0) return PGO_OK;
  PGOC(S.open());

  const int64_t ld = S.ld;
  const int kpp = S.per_pass();
  const int mcap = 3 * std::min<int64_t>(kpp, n);
  PGOC(S.alloc(mcap));
  double* gath;
  int32_t *rows, *rows_out;
  const int n_out_max = o.cross ? 3 * n : mcap;
  PGOC(S.buf.alloc(&rows, mcap));
  PGOC(S.buf.alloc(&rows_out, n_out_max));
  PGOC(S.buf.alloc(&gath, (int64_t)mcap * n_out_max));
  if (o.cross) {
    std::vector<int32_t> ro((size_t)3 * n);
    for (int32_t j = 0; j < n; ++j)
      for (int a = 0; a < 3; ++a) ro[3 * j + a] = (int32_t)(3 * S.internal(poses[j]) + a);
    HIPC(hipMemcpyAsync(rows_out, ro.data(), ro.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    PGOC(h->sync());
  }
  std::vector<double> hg;
  for (int32_t j0 = 0; j0 < n; j0 += kpp) {
    const int k = (int)std::min<int64_t>(kpp, n - j0), m = 3 * k;
    std::vector<int32_t> rr((size_t)m);
    for (int j = 0; j < k; ++j)
      for (int a = 0; a < 3; ++a) rr[3 * j + a] = (int32_t)(3 * S.internal(poses[j0 + j]) + a);
    HIPC(hipMemcpyAsync(rows, rr.data(), rr.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (!o.cross) HIPC(hipMemcpyAsync(rows_out, rr.data(), rr.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    PassRhs B;
    B.rows = rows;
    PGOC(S.pass(m, B, [&](int c) { return "pose " + std::to_string(poses[j0 + c / 3]); }));
    const int n_out = o.cross ? 3 * n : m;
    hipLaunchKernelGGL(dev::k_cov_gather<>, dim3((unsigned)(((int64_t)m * n_out + 255) / 256)), dim3(256), 0, h->stream, m, ld, (const double*)S.X,
                       (const double*)h->scale, (const int32_t*)rows_out, n_out, gath);
    PGOC(h->check_launch("k_cov_gather"));
    hg.resize((size_t)m * n_out);
    HIPC(hipMemcpyAsync(hg.data(), gath, hg.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PGOC(h->sync());
    // column (pose j0 + jc, component b), row entry i of rows_out
    if (o.cross) {
      const int64_t W = 3 * (int64_t)n;
      for (int c = 0; c < m; ++c)
        for (int64_t i = 0; i < W; ++i) out[i * W + 3 * (int64_t)j0 + c] = hg[(size_t)c * n_out + i];
    } else {
      for (int jc = 0; jc < k; ++jc)
        for (int a = 0; a < 3; ++a)
          for (int b = 0; b < 3; ++b) out[9 * (int64_t)(j0 + jc) + 3 * a + b] = hg[(size_t)(3 * jc + b) * n_out + 3 * jc + a];
    }
  }
  // symmetric blocks: 1/2 (Sigma_ab + Sigma_ba')
  if (o.cross) {
    const int64_t W = 3 * (int64_t)n;
    for (int64_t i = 0; i < W; ++i)
      for (int64_t j = i + 1; j < W; ++j) {
        const double v = 0.5 * (out[i * W + j] + out[j * W + i]);
        out[i * W + j] = out[j * W + i] = v;
      }
  } else {
    for (int32_t j = 0; j < n; ++j) {
      double* B = out + 9 * (int64_t)j;
      for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b) B[3 * a + b] = B[3 * b + a] = 0.5 * (B[3 * a + b] + B[3 * b + a]);
    }
  }
  S.fill(report, 3 * n, t0);
  return PGO_OK;
}

int pgo_gate_evaluate(const double r[3], const double P[9], const double* info6_or_null, double out[3]) {
  if (!r || !P || !out) return fail(PGO_ERR_INVALID_ARG, "pgo_gate_evaluate: null");
  const int st = pgo::gate_evaluate(r, P, info6_or_null, out);
  if (st == pgo::GATE_OMEGA_NOT_PD) return fail(PGO_ERR_INVALID_ARG, "pgo_gate_evaluate: the information matrix is not finite and positive definite");
  if (st == pgo::GATE_M_NOT_PD) return fail(PGO_ERR_NUMERIC, "pgo_gate_evaluate: I + L'PL is not positive definite (P is indefinite or not finite)");
  return PGO_OK;
}

}  // extern "C"

namespace {

bool info6_ok(const double* w) {
  double l[6];
  bool ok = true;
  for (int c = 0; c < 6; ++c) ok = ok && std::isfinite(w[c]);
  return ok && pgo::gate_chol3(w, l);
}

// what pgo_edge_gate_joint asks for beyond pgo_edge_gate
struct JointCall {
  const int8_t* force;
  pgo_gate_joint_options o;
  pgo_gate_joint_result* joint;
  double* P_full;
  pgo_gate_joint_summary* sum;
};

int joint_options(const std::string& fn, int32_t n, const int8_t* force, const pgo_gate_joint_options* opt_or_null, pgo_gate_joint_options* o) {
  if (opt_or_null) *o = *opt_or_null;
  else pgo_gate_joint_options_default(o);
  if (std::isnan(o->chi2_gate) || std::isnan(o->min_info_gain)) return fail(PGO_ERR_INVALID_ARG, fn + ": chi2_gate or min_info_gain is NaN");
  if (n > PGO_GATE_JOINT_MAX)
    return fail(PGO_ERR_UNSUPPORTED, fn + ": " + std::to_string(n) + " candidates, at most " + std::to_string(PGO_GATE_JOINT_MAX) +
                                         " per call (split the set, or use pgo_edge_gate)");
  for (int32_t k = 0; force && k < n; ++k)
    if (force[k] < -1 || force[k] > 1)
      return fail(PGO_ERR_INVALID_ARG, fn + ": force[" + std::to_string(k) + "] = " + std::to_string((int)force[k]) + " is not -1, 0 or 1");
  return PGO_OK;
}

int joint_not_pd(const std::string& fn, int k) {
  return fail(PGO_ERR_NUMERIC, fn + ": the pivot I + L'ML of candidate " + std::to_string(k) + " is not positive definite (P is indefinite or not finite)");
}

// pgo_edge_gate (jc == nullptr) and pgo_edge_gate_joint: one code path, one pass plan
int gate_call(const char* name, pgo_t* h, int32_t n, const int32_t* ia, const int32_t* ib, const double* meas_xyt, const double* info6_or_null,
              const pgo_covariance_options* opt_or_null, pgo_edge_gate_result* out, pgo_covariance_report* report, const JointCall* jc) {
  const double t0 = wall_s();
  const std::string fn(name);
  if (!h) return fail(PGO_ERR_INVALID_ARG, fn + ": null handle");
  if (n < 0 || (n > 0 && (!ia || !ib || !meas_xyt || !out))) return fail(PGO_ERR_INVALID_ARG, fn + ": bad argument");
  Session S(h, name);
  PGOC(S.check(opt_or_null));
  const int64_t N = S.N;
  for (int32_t k = 0; k < n; ++k) {
    if (ia[k] < 0 || ia[k] >= N || ib[k] < 0 || ib[k] >= N)
      return fail(PGO_ERR_INVALID_ARG, fn + ": candidate " + std::to_string(k) + " has a pose index out of range");
    if (ia[k] == ib[k]) return fail(PGO_ERR_INVALID_ARG, fn + ": candidate " + std::to_string(k) + " joins pose " + std::to_string(ia[k]) + " to itself");
    if (info6_or_null && !info6_ok(info6_or_null + 6 * (int64_t)k))
      return fail(PGO_ERR_INVALID_ARG, fn + ": the information matrix of candidate " + std::to_string(k) + " is not finite and positive definite");
  }
  PGOC(S.need_switches());
  if (report) memset(report, 0, sizeof *report);
  if (n == 0) return PGO_OK;
  PGOC(S.open());

  // the candidates on the device, internal pose numbering; r, J and the plan flags of every one
  int32_t *d_ia, *d_ib, *d_flags, *d_cand;
  double *d_meas, *d_info = nullptr;
  dev::GateRec* rec;
  pgo_edge_gate_result* d_out;
  PGOC(S.buf.alloc(&d_ia, n));
  PGOC(S.buf.alloc(&d_ib, n));
  PGOC(S.buf.alloc(&d_flags, n));
  PGOC(S.buf.alloc(&d_cand, n));
  PGOC(S.buf.alloc(&d_meas, 3 * (int64_t)n));
  if (info6_or_null) PGOC(S.buf.alloc(&d_info, 6 * (int64_t)n));
  PGOC(S.buf.alloc(&rec, n));
  PGOC(S.buf.alloc(&d_out, n));
  std::vector<int32_t> ha((size_t)n), hb((size_t)n), flags((size_t)n);
  for (int32_t k = 0; k < n; ++k) {
    ha[k] = (int32_t)S.internal(ia[k]);
    hb[k] = (int32_t)S.internal(ib[k]);
  }
  HIPC(hipMemcpyAsync(d_ia, ha.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  HIPC(hipMemcpyAsync(d_ib, hb.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  HIPC(hipMemcpyAsync(d_meas, meas_xyt, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (d_info) HIPC(hipMemcpyAsync(d_info, info6_or_null, (size_t)6 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(dev::k_gate_eval<>, dim3((unsigned)((n + dev::WG - 1) / dev::WG)), dim3(dev::WG), 0, h->stream, (int)n, (const int32_t*)d_ia,
                     (const int32_t*)d_ib, (const double*)d_meas, (const double*)h->poses, (const double*)h->scale, rec, d_flags);
  PGOC(h->check_launch("k_gate_eval"));
  HIPC(hipMemcpyAsync(flags.data(), d_flags, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  PGOC(h->sync());
  // the pass plan: candidates with status 1, and those whose right-hand sides are zero (both endpoints constant), take no columns
  std::vector<int32_t> plan, rest;
  for (int32_t k = 0; k < n; ++k) (flags[k] == 2 ? plan : rest).push_back(k);
  const int32_t n_solve = (int32_t)plan.size();
  plan.insert(plan.end(), rest.begin(), rest.end());
  HIPC(hipMemcpyAsync(d_cand, plan.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  PGOC(h->sync());
  // the joint gate: C = [J_q Sigma J_p'] over all candidates (zero where a candidate takes no columns), the working state
  const int64_t W = 3 * (int64_t)n;
  double *d_C = nullptr, *d_M = nullptr, *d_rho = nullptr;
  int32_t* d_status = nullptr;
  int8_t* d_force = nullptr;
  pgo_gate_joint_result* d_joint = nullptr;
  if (jc) {
    PGOC(S.buf.alloc(&d_C, W * W));
    PGOC(S.buf.alloc(&d_M, W * W));
    PGOC(S.buf.alloc(&d_rho, W));
    PGOC(S.buf.alloc(&d_status, n));
    PGOC(S.buf.alloc(&d_joint, n));
    if (jc->force) {
      PGOC(S.buf.alloc(&d_force, n));
      HIPC(hipMemcpyAsync(d_force, jc->force, (size_t)n, hipMemcpyHostToDevice, h->stream));
    }
    HIPC(hipMemsetAsync(d_C, 0, (size_t)(W * W) * sizeof(double), h->stream));
  }
  const int kpp = S.per_pass();
  if (n_solve > 0) PGOC(S.alloc(3 * std::min<int32_t>(kpp, n_solve)));
  for (int32_t j0 = 0; j0 < n_solve; j0 += kpp) {
    const int k = (int)std::min<int32_t>(kpp, n_solve - j0), m = 3 * k;
    PassRhs B;
    B.rec = rec;
    B.cand = d_cand + j0;
    PGOC(S.pass(m, B, [&](int c) { return "candidate " + std::to_string(plan[j0 + c / 3]); }));
    hipLaunchKernelGGL(dev::k_gate_reduce<>, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, h->stream, k, (const int32_t*)(d_cand + j0), (const dev::GateRec*)rec, (const double*)S.X,
                       S.ld, (const double*)h->scale, (const double*)d_info, d_out);
    PGOC(h->check_launch("k_gate_reduce"));
    if (jc) {   // the blocks between this pass's candidates and all candidates with columns, from the columns just solved
      hipLaunchKernelGGL(dev::k_gate_cross<>, dim3((unsigned)(((int64_t)n_solve * k + dev::WG - 1) / dev::WG)), dim3(dev::WG), 0, h->stream, (int)n_solve,
                         (const int32_t*)d_cand, k, (const int32_t*)(d_cand + j0), (const dev::GateRec*)rec, (const double*)S.X, S.ld, (const double*)h->scale, W, d_C);
      PGOC(h->check_launch("k_gate_cross"));
    }
  }
  if (n > n_solve) {
    const int k = n - n_solve;
    hipLaunchKernelGGL(dev::k_gate_reduce<>, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, h->stream, k, (const int32_t*)(d_cand + n_solve),
                       (const dev::GateRec*)rec, (const double*)nullptr, S.ld, (const double*)h->scale, (const double*)d_info, d_out);
    PGOC(h->check_launch("k_gate_reduce"));
  }
  HIPC(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(pgo_edge_gate_result), hipMemcpyDeviceToHost, h->stream));
  if (jc) {
    // P = 1/2 (C + C'), then the elimination on it in place.  Shape: one launch per candidate, a grid of workgroups over the
    // trailing rows (a kernel boundary between two candidates, no barrier across workgroups); the "gate_joint_shape" knob = 0
    // walks all candidates in ONE launch of one workgroup instead -- measured 1.8 x slower at the cap with everything
    // accepted ("Joint gate").
    hipLaunchKernelGGL(dev::k_gate_symmetrise<>, dim3((unsigned)((W * W + dev::WG - 1) / dev::WG)), dim3(dev::WG), 0, h->stream, W, (const double*)d_C, d_M);
    PGOC(h->check_launch("k_gate_symmetrise"));
    if (jc->P_full) HIPC(hipMemcpyAsync(jc->P_full, d_M, (size_t)(W * W) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PGOC(h->sync());   // (the copy of P has left before the elimination overwrites it)
    hipLaunchKernelGGL(dev::k_gate_joint_begin<>, dim3((unsigned)((n + dev::WG - 1) / dev::WG)), dim3(dev::WG), 0, h->stream, (int)n, (const dev::GateRec*)rec, d_rho,
                       d_status);
    PGOC(h->check_launch("k_gate_joint_begin"));
    dev::GateJointArgs A;
    A.n = n;
    A.M = d_M;
    A.rho = d_rho;
    A.info6 = d_info;
    A.status = d_status;
    A.force = d_force;
    A.chi2_gate = jc->o.chi2_gate;
    A.min_info_gain = jc->o.min_info_gain;
    A.joint = d_joint;
    if (knob("gate_joint_shape") != 0) {
      for (int32_t k = 0; k < n; ++k) {
        A.k0 = k;
        A.k1 = k + 1;
        const int rows = 3 * (n - 1 - k), per_wg = 3 * (dev::GATE_JOINT_WG / 256);
        hipLaunchKernelGGL(dev::k_gate_joint_step<>, dim3((unsigned)std::min(std::max(1, (rows + per_wg - 1) / per_wg), 64)), dim3(dev::GATE_JOINT_WG), 0, h->stream, A);
      }
    } else {
      A.k0 = 0;
      A.k1 = n;
      hipLaunchKernelGGL(dev::k_gate_joint_step<>, dim3(1), dim3(dev::GATE_JOINT_WG), 0, h->stream, A);
    }
    PGOC(h->check_launch("k_gate_joint_step"));
    HIPC(hipMemcpyAsync(jc->joint, d_joint, (size_t)n * sizeof(pgo_gate_joint_result), hipMemcpyDeviceToHost, h->stream));
  }
  PGOC(h->sync());
  for (int32_t k = 0; k < n; ++k)
    if (out[k].status == 0 && !(std::isfinite(out[k].chi2_marginal) && std::isfinite(out[k].info_gain)))
      return fail(PGO_ERR_NUMERIC, fn + ": I + L'PL of candidate " + std::to_string(k) + " is not positive definite");
  if (jc) {
    for (int32_t k = 0; k < n; ++k)
      if (jc->joint[k].status == 0 && !(std::isfinite(jc->joint[k].chi2_cond) && std::isfinite(jc->joint[k].info_gain_cond))) return joint_not_pd(fn, k);
    pgo::gate_joint_summarise(n, jc->joint, jc->sum);
  }
  S.fill(report, 3 * n_solve, t0);
  return PGO_OK;
}

}  // namespace

extern "C" {

int pgo_edge_gate(pgo_t* h, int32_t n, const int32_t* ia, const int32_t* ib, const double* meas_xyt, const double* info6_or_null,
                  const pgo_covariance_options* opt_or_null, pgo_edge_gate_result* out, pgo_covariance_report* report) {
  return gate_call("pgo_edge_gate", h, n, ia, ib, meas_xyt, info6_or_null, opt_or_null, out, report, nullptr);
}

void pgo_gate_joint_options_default(pgo_gate_joint_options* o) {
  if (!o) return;
  o->chi2_gate = 7.814727903251179;
  o->min_info_gain = 0.0;
}

int pgo_gate_joint_evaluate(int32_t n, const double* r, const double* P, const double* info6_or_null, const int32_t* status_or_null,
                            const int8_t* force_or_null, const pgo_gate_joint_options* opt_or_null, pgo_gate_joint_result* joint,
                            pgo_gate_joint_summary* sum) {
  const std::string fn = "pgo_gate_joint_evaluate";
  if (n < 0 || !sum || (n > 0 && (!r || !P || !joint))) return fail(PGO_ERR_INVALID_ARG, fn + ": bad argument");
  pgo_gate_joint_options o;
  PGOC(joint_options(fn, n, force_or_null, opt_or_null, &o));
  for (int32_t k = 0; k < n; ++k) {
    if (status_or_null && status_or_null[k] != 0 && status_or_null[k] != 1) return fail(PGO_ERR_INVALID_ARG, fn + ": status[" + std::to_string(k) + "] is not 0 or 1");
    if (info6_or_null && !info6_ok(info6_or_null + 6 * (int64_t)k))
      return fail(PGO_ERR_INVALID_ARG, fn + ": the information matrix of candidate " + std::to_string(k) + " is not finite and positive definite");
  }
  const int64_t W = 3 * (int64_t)n;
  std::vector<double> rho(r, r + W), M(P, P + W * W), B((size_t)std::max<int64_t>(3 * W, 1));
  int bad = -1;
  const int st = pgo::gate_joint_serial(n, rho.data(), M.data(), info6_or_null, status_or_null, force_or_null, o.chi2_gate, o.min_info_gain, joint, B.data(), &bad);
  if (st != pgo::GATE_OK) return joint_not_pd(fn, bad);
  pgo::gate_joint_summarise(n, joint, sum);
  return PGO_OK;
}

int pgo_edge_gate_joint(pgo_t* h, int32_t n, const int32_t* ia, const int32_t* ib, const double* meas_xyt, const double* info6_or_null,
                        const int8_t* force_or_null, const pgo_gate_joint_options* jopt_or_null, const pgo_covariance_options* opt_or_null,
                        pgo_edge_gate_result* out, pgo_gate_joint_result* joint, double* P_full_or_null, pgo_gate_joint_summary* sum,
                        pgo_covariance_report* report) {
  const std::string fn = "pgo_edge_gate_joint";
  if (n < 0 || !sum || (n > 0 && !joint)) return fail(PGO_ERR_INVALID_ARG, fn + ": bad argument");
  JointCall jc;
  jc.force = force_or_null;
  jc.joint = joint;
  jc.P_full = P_full_or_null;
  jc.sum = sum;
  PGOC(joint_options(fn, n, force_or_null, jopt_or_null, &jc.o));
  memset(sum, 0, sizeof *sum);
  return gate_call("pgo_edge_gate_joint", h, n, ia, ib, meas_xyt, info6_or_null, opt_or_null, out, report, &jc);
}

}  // extern "C"

// ====================================================================== posterior sampling
namespace {

// What pgo_posterior_sample and pgo_debug_sample_rhs share: the refusals, the open session, the tables of the right-hand side.
struct SampleCall {
  Session S;
  pgo_handle* h;
  int32_t* d_orig = nullptr;   // local edge -> the caller's edge
  int32_t* d_inv = nullptr;    // internal row -> the caller's pose (nullptr: the identity)
  SampleCall(pgo_handle* hh, const char* name) : S(hh, name), h(hh) {}

  int open(const pgo_covariance_options& o) {
    if (h->has_sw || h->opt.method == 2)   // (its pose marginal needs noise on the switch rows too)
      return fail(PGO_ERR_UNSUPPORTED, S.fn + ": METHOD 2 is not supported (METHOD 0 and 1 only)");
    PGOC(S.check(&o));
    PGOC(S.open());
    const int64_t EL = h->S.n_edges_local;
    PGOC(S.buf.alloc(&d_orig, EL));
    if (EL > 0) HIPC(hipMemcpyAsync(d_orig, h->S.orig_edge.data(), (size_t)EL * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (!h->perm.empty()) {
      std::vector<int32_t> inv((size_t)S.N);
      for (int64_t i = 0; i < S.N; ++i) inv[(size_t)h->perm[i]] = (int32_t)i;
      PGOC(S.buf.alloc(&d_inv, S.N));
      HIPC(hipMemcpyAsync(d_inv, inv.data(), inv.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
      PGOC(h->sync());   // (`inv` dies with this scope)
    }
    return h->sync();
  }

  // b (m columns at stride ld, samples sample0 ..) = S J' eps + S R eps_p;  unit: without the scales (0 on constant poses stays)
  int rhs(int m, int32_t sample0, uint64_t seed, int unit, double* b) {
    dev::SampleRhsArgs A;
    A.jr = h->jr;
    A.inc_ptr = h->inc_ptr;
    A.inc_edge = h->inc_edge;
    A.orig = d_orig;
    A.scale = h->scale;
    A.n = (int32_t)S.N;
    A.m = m;
    A.sample0 = sample0;
    A.seed = seed;
    A.ld = S.ld;
    A.b = b;
    const dim3 grid((unsigned)((S.N + dev::WG - 1) / dev::WG), m);
    if (unit) hipLaunchKernelGGL(dev::k_sample_rhs<true>, grid, dim3(dev::WG), 0, h->stream, A);
    else hipLaunchKernelGGL(dev::k_sample_rhs<false>, grid, dim3(dev::WG), 0, h->stream, A);
    PGOC(h->check_launch("k_sample_rhs"));
    if (h->pri_n > 0) {
      dev::SamplePriorArgs Q;
      Q.row = h->pri_row_s.in(h->pri_tab.p);
      Q.order = h->pri_order_s.in(h->pri_tab.p);
      Q.rec = h->pri_rec_s.in(h->pri_tab.p);
      Q.scale = h->scale;
      Q.n = h->pri_n;
      Q.m = m;
      Q.sample0 = sample0;
      Q.unit = unit;
      Q.seed = seed;
      Q.ld = S.ld;
      Q.b = b;
      hipLaunchKernelGGL(dev::k_sample_prior<>, dim3(h->prior_grid(), m), dim3(dev::WG), 0, h->stream, Q);
      PGOC(h->check_launch("k_sample_prior"));
    }
    return PGO_OK;
  }
};

}  // namespace

extern "C" {

void pgo_sample_options_default(pgo_sample_options* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->rtol = 1e-10;
  o->max_iters = 20000;
  o->samples_per_pass = 24;
  o->solver = 0;
  o->first_sample = 0;
  o->seed = 0;
}

int pgo_sample_noise_eval(uint64_t seed, int32_t stream, int64_t index, int32_t sample, double z[3]) {
  if (!z) return fail(PGO_ERR_INVALID_ARG, "pgo_sample_noise_eval: null");
  if ((stream != 0 && stream != 1) || index < 0 || index > (int64_t)UINT32_MAX || sample < 0)
    return fail(PGO_ERR_INVALID_ARG, "pgo_sample_noise_eval: stream is 0 (edges) or 1 (priors), 0 <= index < 2^32, sample >= 0");
  pgo::sample_triple(seed, (uint32_t)stream, (uint32_t)index, (uint32_t)sample, z);
  return PGO_OK;
}

int pgo_posterior_sample(pgo_t* h, int32_t n_samples, const pgo_sample_options* opt_or_null, double* delta_out, double* cov_out,
                         pgo_covariance_report* report) {
  const double t0 = wall_s();
  const std::string fn = "pgo_posterior_sample";
  if (!h) return fail(PGO_ERR_INVALID_ARG, fn + ": null handle");
  pgo_sample_options so;
  if (opt_or_null) so = *opt_or_null;
  else pgo_sample_options_default(&so);
  if (n_samples < 1) return fail(PGO_ERR_INVALID_ARG, fn + ": n_samples >= 1 required");
  if (!delta_out && !cov_out) return fail(PGO_ERR_INVALID_ARG, fn + ": delta_out and cov_out are both null");
  if (so.solver == 0 && (so.samples_per_pass < 1 || so.samples_per_pass > dev::COV_MAX_COLS))
    return fail(PGO_ERR_INVALID_ARG, fn + ": samples_per_pass in 1..48 required");
  if (so.first_sample < 0 || (int64_t)so.first_sample + n_samples > (int64_t)INT32_MAX)
    return fail(PGO_ERR_INVALID_ARG, fn + ": first_sample >= 0 and first_sample + n_samples < 2^31 required");
  pgo_covariance_options co;
  pgo_covariance_options_default(&co);
  co.rtol = so.rtol;
  co.max_iters = so.max_iters;
  co.solver = so.solver;
  SampleCall C(h, "pgo_posterior_sample");
  Session& S = C.S;
  if (report) memset(report, 0, sizeof *report);
  PGOC(C.open(co));
  const int64_t N = S.N, n3 = S.n3, ld = S.ld;
  {   // every pose constant: b is identically zero
    std::vector<double> sc((size_t)n3);
    HIPC(hipMemcpyAsync(sc.data(), h->scale, sc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PGOC(h->sync());
    if (std::all_of(sc.begin(), sc.end(), [](double v) { return v == 0.0; }))
      return fail(PGO_ERR_INVALID_ARG, fn + ": every pose is constant (the right-hand side of a sample is zero)");
  }
  // samples per pass.  solver = 1: the library's choice, as the columns of pgo_pose_covariance
  const int per = S.direct ? 3 * S.per_pass() : so.samples_per_pass;
  const int mcap = (int)std::min<int64_t>(per, n_samples);
  PGOC(S.alloc(mcap));
  // b in a panel of its own: the true-residual and replacement steps read it again; after a pass it stages the deltas
  double *Bp, *acc, *d_cov = nullptr;
  PGOC(S.buf.alloc(&Bp, (int64_t)mcap * ld));
  PGOC(S.buf.alloc(&acc, 6 * N));
  if (cov_out) PGOC(S.buf.alloc(&d_cov, 9 * N));
  HIPC(hipMemsetAsync(acc, 0, (size_t)(6 * N) * sizeof(double), h->stream));
  for (int32_t s0 = 0; s0 < n_samples; s0 += per) {
    const int m = (int)std::min<int32_t>(per, n_samples - s0);
    const int32_t first = so.first_sample + s0;
    PGOC(C.rhs(m, first, so.seed, 0, Bp));
    PassRhs B;
    B.panel = Bp;
    PGOC(S.pass(m, B, [&](int c) { return "sample " + std::to_string(first + c); }));
    hipLaunchKernelGGL(dev::k_sample_accum<>, dim3(S.gs), dim3(dev::WG), 0, h->stream, (int32_t)N, m, ld, (const double*)S.X, (const double*)h->scale,
                       (const int32_t*)C.d_inv, acc, delta_out ? Bp : nullptr);
    PGOC(h->check_launch("k_sample_accum"));
    if (delta_out) {
      HIPC(hipMemcpyAsync(delta_out + (int64_t)s0 * n3, Bp, (size_t)m * n3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      PGOC(h->sync());
    }
  }
  if (cov_out) {
    hipLaunchKernelGGL(dev::k_sample_finish<>, dim3(S.gs), dim3(dev::WG), 0, h->stream, (int32_t)N, (double)n_samples, (const double*)acc,
                       (const int32_t*)C.d_inv, d_cov);
    PGOC(h->check_launch("k_sample_finish"));
    HIPC(hipMemcpyAsync(cov_out, d_cov, (size_t)(9 * N) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  PGOC(h->sync());
  S.fill(report, n_samples, t0);
  return PGO_OK;
}

int pgo_debug_sample_rhs(pgo_t* h, uint64_t seed, int32_t sample, double* eps_out, double* b_out) {
  const std::string fn = "pgo_debug_sample_rhs";
  if (!h) return fail(PGO_ERR_INVALID_ARG, fn + ": null handle");
  if (sample < 0 || (!eps_out && !b_out)) return fail(PGO_ERR_INVALID_ARG, fn + ": sample >= 0 and an output required");
  pgo_covariance_options co;
  pgo_covariance_options_default(&co);
  SampleCall C(h, "pgo_debug_sample_rhs");
  Session& S = C.S;
  PGOC(C.open(co));
  const int64_t E = h->n_edges_total, EL = h->S.n_edges_local;
  if (eps_out && E > 0) {
    double* d_eps;
    PGOC(S.buf.alloc(&d_eps, 3 * E));
    hipLaunchKernelGGL(dev::k_sample_eps<>, dim3((unsigned)std::min<int64_t>((EL + dev::WG - 1) / dev::WG, 1024)), dim3(dev::WG), 0, h->stream, EL,
                       (const int32_t*)C.d_orig, seed, sample, d_eps);
    PGOC(h->check_launch("k_sample_eps"));
    HIPC(hipMemcpyAsync(eps_out, d_eps, (size_t)(3 * E) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PGOC(h->sync());
  }
  if (b_out) {
    double* b;
    PGOC(S.buf.alloc(&b, S.ld));
    PGOC(C.rhs(1, sample, seed, 1, b));
    PGOC(h->download_pose_vector(b_out, b));
  }
  return PGO_OK;
}

}  // extern "C"
