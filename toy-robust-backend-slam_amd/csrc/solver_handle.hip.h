#pragma once
// The solver handle of the pose-graph backend: device buffers, launch helpers and the declarations of the pieces that
// live in the translation units around it --
//   solver_create.hip   pgo_handle::create: shard structure -> the plan (plan.h: every choice made once) -> device (direct_build, coarse_build)
//   solver_lm.hip       Ceres' TrustRegionMinimizer + LevenbergMarquardtStrategy policy (lm_begin, lm_iteration, ...)
//   solver_pcg.hip      block-Jacobi PCG, its preconditioners' set-up, the coarse level
//   solver_direct.hip   the direct chain + low-rank solve
//   solver_launch.hip   the launch sequences several units need, each stated once: K1, K2, K3, the reductions, the halo exchange,
//                       z = M^-1 b, the Jacobi scales, the switch elimination, pose vectors in and out
//   solver_batch.hip    pgo_batch: many independent problems in one handle
//   solver_abi.hip      the [gpu] part of the C-ABI, test hooks, debug / bench entry points
//   solver_window.hip   pgo_window_solve: many tiny windows of the graph, one workgroup each (window.hip.h)
//   solver_score.hip    pgo_trajectory_error, pgo_edge_weights: scoring a solve on the device (score.hip.h, traj_error.h)
//   solver_coarsen.hip  pgo_coarsen, pgo_prolong: a coarse graph along the odometry chain and back (coarsen.hip.h, coarsen.h)
//   solver_gnc.hip      pgo_set_edge_weights, pgo_gnc_update, pgo_gnc_solve: the edge weight plane and GNC-TLS (gnc.hip.h, gnc.h)
//   solver_support.hip  pgo_loop_support: loop edges judged by odometry cycle consistency (loop_support.hip.h, loop_support.h)
//   solver_chordal.hip  pgo_chordal_init: a linear start, chordal rotations then positions (chordal.hip.h, chordal.h)
//   solver_mixture.hip  pgo_set_mixtures, pgo_mixture_select, pgo_mixture_solve: max-mixture edges (mixture.hip.h, mixture.h)
//   solver_prior.hip    pgo_set_priors, pgo_get_prior_residuals, pgo_prior_eval: absolute pose priors (prior.hip.h, prior.h)
// Every kernel header declares its kernels `static`: a translation unit carries the kernels it launches.
// The add-on calls (the last eight units) share the helpers below: requires() for their refusals, reserve() and the Layouts of
// scratch.h for their staging and work buffers.
//
// Replaces, for DCS-ceres/main.cpp METHOD 0/1 (paths relative to /root/reference/DCS-ceres):
//   main.cpp:66-68,95-153   problem assembly  -> pgo_create (shard structure + device upload)
//   main.cpp:154-163        ceres::Solve      -> pgo_solve / pgo_lm_begin + pgo_lm_step
// The minimiser follows Ceres' TrustRegionMinimizer + LevenbergMarquardtStrategy defaults
// (SURVEY.md R9); the linear solve is block-Jacobi PCG on the Jacobi-scaled normal equations.
//
// There is NO CPU fallback here: every [gpu] entry point fails with PGO_ERR_NO_DEVICE when no
// gfx950 device is visible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <functional>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "comm.h"
#include "kernels.hip.h"
#include "trust_region.h"
#include "solo.hip.h"
#include "direct.hip.h"
#include "coarse.hip.h"
#include "pgo_internal.h"
#include "plan.h"
#include "scratch.h"

using pgo::fail;
namespace dev = pgo::dev;

#define HIPC(expr)                                                                       \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) return fail(PGO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)
#define PGOC(expr)            \
  do {                        \
    int _s = (expr);          \
    if (_s != PGO_OK) return _s; \
  } while (0)

// The library reads two documented environment variables only -- PGO_FORCE_COLLECTIVES, PGO_GRAPH_COLLECTIVES (create()) --
// and never lets the environment override a pgo_options field.

using pgo::knob;
using pgo::require_device;

// the refusals pgo_coarsen_plan / pgo_loop_support_plan share with the calls on a handle
static inline int no_chain(const std::string& who, int32_t gap) {
  return fail(PGO_ERR_UNSUPPORTED, who + ": poses " + std::to_string(gap) + " and " + std::to_string(gap + 1) + " are not joined by an edge");
}
static inline int not_finite(const std::string& who, int64_t e) {
  return fail(PGO_ERR_NUMERIC, who + ": the measurement of edge " + std::to_string(e) + " is not finite");
}

static inline double wall_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct PartRef {   // one array of per-workgroup partials for reduce_to_scal
  const double* p;
  int n;
  int is_max;
};
namespace {
constexpr int N_SCAL = 16;
constexpr int N_PART = 6;
}  // namespace

struct pgo_handle {
  pgo_options opt;
  pgo::ShardStructure S;
  // Every choice made once per handle (plan.h): written by create(), read-only afterwards.  What changes during a handle's life
  // is the live state below, and the solver in force is derived from both where it is needed (direct(), takeover(), coarse_on()).
  pgo::Plan plan;
  const pgo::CoarsePlan& CO() const { return plan.co.on ? plan.co : plan.co_cov; }   // the coarse level that is (or can be) built
  pgo_comm* comm = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<void*> allocs;
  int64_t device_bytes = 0;

  int64_t n_full = 0;  // world * rows_per_rank  (>= N; tail rows are padding)
  // graph
  double *poses = nullptr, *cand = nullptr, *scale = nullptr;
  int32_t *e_ia = nullptr, *e_ib = nullptr;
  double *e_mx = nullptr, *e_my = nullptr, *e_mt = nullptr;
  uint8_t* e_flags = nullptr;
  double* jr = nullptr;
  // information matrices (6 planes over the local edges); info_mode = opt.info_weighting with them present
  double* e_info = nullptr;
  bool info_mode = false;
  int rec_doubles = dev::REC;
  int32_t* e_orig = nullptr;   // local edge -> caller's edge index (device copy, for pgo_edge_chi2)
  double* chi2_buf = nullptr;  // [n_edges_total], allocated at the first pgo_edge_chi2
  int64_t n_edges_total = 0;
  int32_t *inc_ptr = nullptr, *inc_edge = nullptr, *inc_col = nullptr, *tile_row = nullptr;
  uint8_t* inc_rowoff = nullptr;
  int4* tile_desc = nullptr;
  // normal equations
  double *hoff = nullptr, *hd = nullptr, *gs = nullptr, *d2 = nullptr, *minv = nullptr, *hdd = nullptr;
  // CG
  double *y = nullptr, *r = nullptr, *z = nullptr, *ap = nullptr, *p_full = nullptr;
  // second preconditioner level (coarse.hip.h): additive coarse correction on the rigid-body modes of pose aggregates
  int co_ncb = 0;
  double *co_pb = nullptr, *co_cap = nullptr, *co_nm = nullptr, *co_dwork = nullptr, *co_rc = nullptr, *co_cy = nullptr, *co_ec = nullptr;
  int32_t *co_cb_i = nullptr, *co_cb_j = nullptr, *co_cb_ptr = nullptr, *co_cb_q = nullptr, *co_cb_row = nullptr;
  int coarse_build(int32_t E, const int32_t* ia, const int32_t* ib);   // the level the plan sized (CO()): block lists, buffers
  int coarse_factor();     // per LM iteration: basis, Galerkin matrix, Cholesky + inverse factor
  double* co_ainv = nullptr;   // explicit inverse N'N (coarse orders <= COARSE_EXPLICIT_RANK: one product per apply)
  int32_t* co_ok = nullptr;    // device flag: the factorisation of this LM iteration is usable
  int32_t* co_dead = nullptr;  // aggregates without a pose in the coarse space (identity on their coarse diagonal)
  int co_ndead = 0;
  bool co_flag_pending = false;   // pcg() left co_ok in scal[15] for the host fetch of lm_iteration_tail
  int co_off_iters = 0;        // LM iterations whose PCG solve found the level switched off (co_ok = 0)
  bool co_cov_ready = false;   // plan.co_cov was built, for pgo_pose_covariance only (solver_covariance.hip): the LM loop runs without it
  bool co_for_call = false;    // ... and a covariance call is using it now (CoarseOn)
  bool co_built() const { return plan.co.on || co_cov_ready; }
  bool coarse_on() const { return plan.co.on || co_for_call; }
  bool co_multi() const { return co_built() && CO().co_multi; }
  int coarse_solve(double* dot_part, const int32_t* done);   // e_c = (P'(H + D'D)P)^-1 P' r  (+ partials of r_c . e_c)
  // several ranks (coarse.hip.h, "several ranks"): replicated coarse problem, aggregates numbered globally
  int co_ncb_max = 0;             // blocks per rank in the gathered list (the largest rank's count)
  uint8_t* co_live = nullptr;     // [N] poses with an edge
  double* co_red = nullptr;       // [Kp + 2]: r_c (global), then the r.z / r.r sums -- one all-reduce
  double* co_gvals = nullptr;     // [world x co_ncb_max x 9] block values, rank r's at r x co_ncb_max x 9
  int32_t *co_gi = nullptr, *co_gj = nullptr;   // [world x co_ncb_max] their coarse coordinates (-1: padding)
  double* co_dotp = nullptr;      // [co_ndot] partials of r_c . e_c
  int coarse_setup_multi(int32_t E, const int32_t* ia, const int32_t* ib, int world, int rank, const std::vector<int32_t>& cbi,
                         const std::vector<int32_t>& cbj, const std::vector<int32_t>& dead, std::vector<int32_t>* gdead);
  int coarse_assemble_multi();
  int coarse_restrict_reduce(const double* rz_part, int n_rz, const double* rr_part, int n_rr, const int32_t* done);
  // single-reduction PCG loop (k_cg_sr_*: one all-reduce per iteration; several ranks, inexact mode, chain preconditioner)
  double* sr_s = nullptr;   // s = A p, carried by recurrence
  dev::CgState* st = nullptr;
  dev::CgState* h_st = nullptr;  // pinned
  // reductions
  double* part[N_PART] = {nullptr};
  double* fold_buf = nullptr;   // 6 x 16: reduce_to_scal's intermediate for partial arrays too long for one workgroup
  double* scal = nullptr;
  double* h_scal = nullptr;  // pinned
  int* bad = nullptr;
  // block-Jacobi over groups of B poses (B > 1): explicit dense inverses
  double* ginv = nullptr;
  // chain (block-tridiagonal) preconditioner over 64-pose segments (opt.pcg_chain_len): C planes, W planes, S^-1 planes
  double *chain_c = nullptr, *chain_w = nullptr, *chain_s = nullptr;
  int32_t* chain_dup_rows = nullptr;   // rows whose block (i, i-1) sums several edges (k_chain_dupfix)
  int n_chain_dup = 0;
  // halo exchange of the search direction (world > 1, opt.halo_exchange)
  int32_t *halo_send_rows = nullptr, *halo_recv_rows = nullptr;
  double *halo_send_buf = nullptr, *halo_recv_buf = nullptr;
  std::vector<int64_t> halo_send_off3, halo_recv_off3;  // offsets in doubles (3 per row)
  // overlap of the halo exchange with the SpMV (opt.halo_overlap): the blocks with owned columns (MODE 4 of k_spmv) are
  // multiplied while the exchange runs on a second stream; the few blocks with remote columns follow (k_spmv_remote)
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_pack = nullptr, ev_halo = nullptr;
  int32_t *rr_rows = nullptr, *rr_ptr = nullptr, *rr_slots = nullptr;
  // METHOD 2: switch variables (one per local edge; only robust edges use theirs), eliminated per edge
  bool has_sw = false;
  double *sw = nullptr, *sw_cand = nullptr, *sw_js = nullptr, *sw_sigma = nullptr, *sw_c = nullptr, *sw_gamma = nullptr,
         *sw_gs = nullptr, *sw_den = nullptr, *sw_hss = nullptr, *diag_full = nullptr, *gs_full = nullptr;
  double sw_norm2 = 0.0, xnorm2_pose = 0.0;
  bool sw_fresh = false;  // elimination coefficients / reduced system match the current point AND radius
  // internal pose numbering (opt.pose_ordering): perm[i] = internal position of the caller's pose i; empty = identity
  std::vector<int32_t> perm;
  int fixed_internal = -1;  // opt.fixed_pose in the internal numbering
  // A caller-ordered pose vector (3 doubles per pose) to the device in the internal numbering, and back.  dst / src are the
  // device rows [row0, row0 + rows) (rows < 0: all poses).  With a permutation the vector is staged on the host; the identity
  // ordering copies straight from / to the caller's memory.  Both synchronise the stream; download leaves 0 in the rows outside
  // the range (the peers' rows of a sharded handle).
  int upload_pose_vector(double* dst, const double* caller_src, int64_t row0 = 0, int64_t rows = -1);
  int download_pose_vector(double* caller_dst, const double* src, int64_t row0 = 0, int64_t rows = -1);
  // captured slice of PCG iterations (world == 1)
  hipGraphExec_t cg_graph_exec = nullptr;
  int cg_graph_len = 0;
  bool graph_failed = false;
  int graph_collectives = 1;   // PGO_GRAPH_COLLECTIVES: 0 = never capture collectives, 1 = all-reduce / all-gather, 2 = also the p2p halo exchange
  int last_pcg_iters = 0;  // iteration count of the previous PCG solve of this handle (slice scheduling)
  double t_enqueue = 0.0;  // host seconds spent enqueueing PCG iterations (launch calls only, no waiting), and how many
  int64_t n_enqueued = 0;
  // small graphs on one rank: the direction update rides in the next SpMV (k_spmv MODE 5) -- two launches per PCG
  // iteration instead of three; p_full / p_full2 alternate by iteration parity
  double* p_full2 = nullptr;
  // batched handle (pgo_batch_*): the block-diagonal union of independent problems, each starting at a multiple of 256 rows
  bool batch_mode = false;
  std::vector<uint8_t> fixed_mask_h;    // set before create(): constant rows (one anchor per problem + the padding rows)
  std::vector<int32_t> tile_breaks_h;   // set before create(): rows at which a row tile must start (problem starts)
  uint8_t* fixed_mask = nullptr;
  int32_t* prob_of_256 = nullptr;       // problem of each 256-row block
  double* prob_radius = nullptr;        // trust-region radius per problem
  double* edge_cost = nullptr;          // cost per local edge (k_edge_eval -> k_prob_reduce)
  // batched handles: the whole PCG solve of an LM iteration as ONE launch, one workgroup per problem (solo.hip.h, solver_batch.hip)
  // direct solve for small chain-like graphs (direct.hip.h): T (odometry chain) + V'V (the other edges) by Woodbury
  // The plan says how a handle starts (plan.dl.direct) and whether the direct solve may take over (plan.dl.dl_possible); which solver
  // is in force now follows from that and the live state: the adaptive rule's side, a failed take-over, a cut chain.
  bool on_direct = false;    // the adaptive PCG / direct rule (lm_iteration) is on the direct solve
  bool dl_gave_up = false;   // the take-over's set-up failed once: PCG for good
  bool takeover() const { return plan.dl.dl_possible && !dl_gave_up && !act_chain_cut; }
  bool direct() const { return !act_chain_cut && (plan.dl.direct || (takeover() && on_direct)); }
  int32_t *dl_chain_edge = nullptr, *dl_lr_edge = nullptr, *dl_va = nullptr, *dl_vb = nullptr;
  double *dl_trec = nullptr, *dl_fac = nullptr, *dl_pre = nullptr, *dl_vrec = nullptr, *dl_Z = nullptr, *dl_cap = nullptr, *dl_dwork = nullptr,
         *dl_nm = nullptr, *dl_cy = nullptr, *dl_cvec = nullptr, *dl_x1 = nullptr, *dl_E = nullptr, *dl_E2 = nullptr;
  double* dl_pre2 = nullptr;   // the finer segmentation of k_dlr_solve1 (up to 256 segments of <= 16 poses)
  double *dl_ksep = nullptr, *dl_R = nullptr, *dl_Wm = nullptr;
  double dl_rel = 0.0;  // |g - (H + D'D) y| / |g| of the latest direct solve
  bool dl_retry = false;   // the current LM iteration is being redone by PCG after a failed direct solve
  int dl_fallbacks = 0;    // how often that happened
  int dl_switched_at = 0;       // LM iteration after which it first did
  int dl_last_probe = 0, dl_dear_run = 0;
  bool dl_ready = false;        // the direct solve's buffers exist
  void clear_direct_buffers() {   // after a failed direct_build(): every pointer it may have set (the memory is freed by the caller)
    dl_chain_edge = dl_lr_edge = dl_va = dl_vb = nullptr;
    dl_trec = dl_fac = dl_pre = dl_vrec = dl_Z = dl_cap = dl_dwork = dl_nm = dl_cy = dl_cvec = dl_x1 = dl_E = dl_E2 = nullptr;
    dl_pre2 = dl_ksep = dl_R = dl_Wm = nullptr;
    dl_ready = false;
  }

  // LM state (TrustRegionMinimizer)
  bool lm_active = false, lin_valid = false, lm_done = false;
  int iter = 0, successful = 0, total_pcg = 0, termination = 0;
  double cost = 0, initial_cost = 0, x_norm = 0, gmax = 0;
  pgo::TrustRegion tr = pgo::tr_begin(0.0);   // radius, decrease factor, invalid-step run, previous step successful
  double t_eval = 0, t_asm = 0, t_lin = 0, t_cand = 0, t_total = 0;   // (t_cand stays 0: the candidate is evaluated with the model terms, inside t_lin)
  std::vector<pgo_iter_record> recs;

  ~pgo_handle() {
    if (device >= 0) (void)hipSetDevice(device);
    if (ev_pack) (void)hipEventDestroy(ev_pack);
    if (ev_halo) (void)hipEventDestroy(ev_halo);
    if (comm_stream) (void)hipStreamDestroy(comm_stream);
    for (void* p : allocs) (void)hipFree(p);
    if (cg_graph_exec) (void)hipGraphExecDestroy(cg_graph_exec);
    if (h_st) (void)hipHostFree(h_st);
    if (h_scal) (void)hipHostFree(h_scal);
    if (stream) (void)hipStreamDestroy(stream);
  }

  // collectives are skipped for a single rank unless PGO_FORCE_COLLECTIVES=1 (lets a 1-GPU box
  // exercise the RCCL calls themselves: at world == 1 they are identities)
  bool force_collectives = false;
  bool multi_rank() const { return comm && (comm->world > 1 || force_collectives); }

  template <class T>
  int dalloc(T** out, int64_t n) {
    void* p = nullptr;
    size_t bytes = (size_t)std::max<int64_t>(n, 1) * sizeof(T);
    // (one hipMalloc per buffer on purpose: all buffers of a handle carved out of ONE allocation were measured 5-12 % slower in
    // K1 / K2 / K3 -- DESIGN.md section 8, round 3 (g))
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return fail(PGO_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    allocs.push_back(p);
    device_bytes += (int64_t)bytes;
    e = hipMemsetAsync(p, 0, bytes, stream);
    if (e != hipSuccess) return fail(PGO_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
    *out = (T*)p;
    return PGO_OK;
  }
  template <class T>
  int upload(T* dst, const std::vector<T>& src) {
    if (src.empty()) return PGO_OK;
    HIPC(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    return PGO_OK;
  }
  int sync() {
    HIPC(hipStreamSynchronize(stream));
    return PGO_OK;
  }
  int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(PGO_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return PGO_OK;
  }
  // a scratch buffer of at least `bytes`: grown on demand (to at least twice its size) and kept; *moved: it was (re)allocated
  // and holds nothing.  (The stream is idle: every call that uses such a buffer ends with a synchronisation.)
  int reserve(pgo::Scratch& s, int64_t bytes, bool* moved = nullptr) {
    if (moved) *moved = bytes > s.cap;
    if (bytes <= s.cap) return PGO_OK;
    const int64_t want = std::max<int64_t>(bytes, 2 * s.cap);
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, (size_t)want);
    if (e != hipSuccess) return fail(PGO_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    if (s.p) {
      allocs.erase(std::remove(allocs.begin(), allocs.end(), s.p), allocs.end());
      (void)hipFree(s.p);
      device_bytes -= s.cap;
    }
    allocs.push_back(q);
    device_bytes += want;
    s.p = q;
    s.cap = want;
    return PGO_OK;
  }
  // what a call needs of its handle; the first unmet need, in this order, is its PGO_ERR_UNSUPPORTED
  enum : unsigned { METHOD_01 = 1, NO_INFO = 2, ONE_RANK = 4, NOT_BATCH = 8, PLAIN_HANDLE = METHOD_01 | NO_INFO | ONE_RANK | NOT_BATCH };
  int requires(const char* who, unsigned needs) const {
    const char* what = nullptr;
    if ((needs & METHOD_01) && opt.method != 0 && opt.method != 1) what = ": METHOD 0 and 1 only";
    else if ((needs & NO_INFO) && (opt.info_weighting || info_mode)) what = ": info_weighting is not supported";
    else if ((needs & ONE_RANK) && (comm || force_collectives)) what = ": one rank without a communicator only";
    else if ((needs & NOT_BATCH) && batch_mode) what = ": not on a batched handle";
    return what ? fail(PGO_ERR_UNSUPPORTED, std::string(who) + what) : PGO_OK;
  }
  void solve_is_stale() {   // as after pgo_set_poses: pgo_lm_step refuses until pgo_lm_begin
    lin_valid = false;
    lm_active = false;
  }
  // workgroups for `units` of work, or what the test hook `knob_name` asks for
  int launch_grid(const char* knob_name, int64_t units) const {
    const long long k = knob(knob_name);
    return (int)std::min<int64_t>(k > 0 ? k : std::max<int64_t>(units, 1), 65535);
  }

  // ---- reductions to scalars: scal[first..first+k) = reduce(parts) [+ all-reduce], no host sync
  int reduce_to_scal(std::initializer_list<PartRef> parts, int first, bool allreduce_max = false);
  int reduce_parts(std::initializer_list<PartRef> parts, double* out, double* ar, int ar_n, bool allreduce_max);
  int fetch_scal(int first, int count) {
    HIPC(hipMemcpyAsync(h_scal + first, scal + first, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, stream));
    return sync();
  }
  int allgather(double* full, int stride = 3) {
    if (multi_rank()) PGOC(comm->allgather_inplace(full, (int64_t)stride * S.rows_per_rank, stream));
    return PGO_OK;
  }
  // make the owned rows of the gather vector visible where the peers need them: either everything
  // (all-gather) or only the rows their off-diagonal blocks reference (halo exchange)
  int share_gather_vector(double* full);
  int pack_halo_rows(const double* full);                // the halo exchange's two ends (k_pack_rows / k_unpack_rows and their grid)
  int unpack_halo_rows(double* full, hipStream_t on);

  // ---- K1
  dev::EdgeArgs edge_args(const double* x, const double* sw_vals, int apply_loss) const {
    dev::EdgeArgs A;
    A.poses = x;
    A.ia = e_ia;
    A.ib = e_ib;
    A.mx = e_mx;
    A.my = e_my;
    A.mt = e_mt;
    A.flags = e_flags;
    A.n_edges = S.n_edges_local;
    A.apply_loss = apply_loss;
    A.phi = opt.phi;
    A.huber_delta = loss_huber;
    A.sw = has_sw ? sw_vals : nullptr;
    A.sw_js = sw_js;
    A.sc_lambda = opt.sc_prior_lambda;
    A.info = e_info;
    A.cost_out = edge_cost;
    A.loss0 = loss_cls[0];
    A.loss1 = loss_cls[1];
    A.loss2 = loss_cls[2];
    A.loss3 = loss_cls[3];
    A.w = w_set ? e_w : nullptr;
    return A;
  }
  // robust losses (pgo_set_losses): the loss of each class; an edge's class sits in bits 2-3 of its flags byte
  pgo::LossClass loss_cls[pgo::MAX_LOSS_CLASSES] = {};
  int loss_n = 1;
  bool loss_general = false;       // K1's general instantiation: anything but one Huber / Trivial class
  double loss_huber = 0.0;         // the default instantiation's Huber scale (<= 0: no loss)
  std::vector<uint8_t> kind_local;   // edge kind per local edge (the default classes)
  void default_losses() {          // a new handle: Huber(huber_delta), Trivial when huber_delta <= 0
    loss_n = 1;
    loss_general = false;
    loss_huber = opt.huber_delta;
    for (auto& L : loss_cls) L = pgo::make_loss_class(opt.huber_delta > 0.0 ? PGO_LOSS_HUBER : PGO_LOSS_TRIVIAL, opt.huber_delta);
  }
  int set_losses(int32_t n_classes, const pgo_loss* losses, const uint8_t* edge_class);
  // active sets (pgo_set_active): an edge mask in bit 4 of the flags bytes, the resolved constant poses in fixed_mask
  bool act_edges = false;             // some edge is inactive: K1 runs its LOSSES instantiations, which test the bit
  bool act_anchor = false;            // pose_constant names at least one pose (a gauge without opt.fixed_pose)
  std::vector<uint8_t> act_const_h;   // the resolved constant rows, internal numbering; empty = no active set in force
  uint8_t* act_mask = nullptr;        // solo handles: device copy, allocated at the first pgo_set_active and kept
  int32_t n_active_edges = 0, n_constant_poses = 0;   // resolved (pgo_handle_info)
  bool act_chain_cut = false;         // an edge of the direct solve's chain is inactive: PCG until it is active again
  int co_dead_cap = 0;                // entries co_dead can hold
  bool has_anchor() const {   // (... or a positive definite pose prior on a pose that is free NOW: pgo_set_active may change that)
    if (fixed_internal >= 0 || act_anchor) return true;
    for (int32_t r : pri_pd_rows)
      if (act_const_h.empty() || !act_const_h[r]) return true;
    return false;
  }
  void coarse_dead_list(std::vector<int32_t>* dead) const;
  int set_active(const uint8_t* edge_active, const uint8_t* pose_constant);
  // edge weights (pgo_set_edge_weights) and graduated non-convexity (pgo_gnc_update, pgo_gnc_solve; solver_gnc.hip, gnc.hip.h,
  // gnc.h): one double in [0, 1] per local edge.  The plane is allocated at its first use and kept; while one is in force K1 runs
  // its LOSSES instantiations, which read it.  gnc_buf holds a call's select bytes, the per-workgroup partials and the folded
  // statistics (made at the first call and kept, reserve), and the caller's edge -> local edge table of k_gnc_update.
  double* e_w = nullptr;
  bool w_set = false;
  pgo::Scratch gnc_buf;
  double* gnc_x = nullptr;   // pgo_gnc_solve: the poses a round started from (allocated at the first call, kept)
  int weights_alloc();                            // the plane, before anything changes
  // a call that writes the plane: weights_begin before anything changes (*fresh: no plane is in force), then, where the call
  // enqueues its uploads, weights_ones on a fresh plane (`ones` is the host source: it lives until the call's synchronisation)
  int weights_begin(bool* fresh) {
    *fresh = !w_set;
    return weights_alloc();
  }
  int weights_ones(std::vector<double>* ones) {
    ones->assign((size_t)S.n_edges_local, 1.0);
    return upload(e_w, *ones);
  }
  int set_edge_weights(const double* w_or_null);
  int get_edge_weights(double* w_out);
  int gnc_update(double cbar, double mu, const uint8_t* select_or_null, bool reset_selected, pgo_gnc_stats* out);
  int gnc_solve(const pgo_gnc_options* o, pgo_gnc_summary* summary, pgo_gnc_round* rounds, int32_t rounds_cap);
  // max-mixture edges (pgo_set_mixtures, pgo_mixture_select, pgo_mixture_solve; solver_mixture.hip, mixture.hip.h, mixture.h).
  // The table of the mixtures in force, in the caller's mixture order: mix_edge_h = the caller's edge, mix_loc_h = its local
  // edge, mix_ptr_h = its components (CSR).  mix_tab = the device copy -- local edge [n] | ptr [n + 1] | the applied selection
  // [n] (-1: none yet) | the component records --, written when the table is set; mix_work = a call's partials, statistics and
  // per-edge outputs.  Both are grown on demand and kept (reserve).  mix_applied: a select has written the planes since the
  // table was set.  The poses a round of pgo_mixture_solve started from share gnc_x.
  int32_t mix_n = 0;
  bool mix_applied = false;
  std::vector<int32_t> mix_edge_h, mix_loc_h, mix_ptr_h;
  pgo::Scratch mix_tab, mix_work;
  std::vector<uint8_t> mix_host;   // host image of a call's outputs
  int mixtures_clear();
  int set_mixtures(const char* who, int32_t n_mix, const int32_t* edge, const int32_t* comp_ptr, const pgo_mix_component* comps);
  int set_mixture_null(const uint8_t* select_or_null, double pi_null, double scale_null);
  int mixture_select(const char* who, int32_t apply, pgo_mix_stats* stats, int32_t* chosen, double* q);
  int mixture_selection(int32_t* chosen_out);
  int mixture_solve(const pgo_mixture_options* o, pgo_mixture_summary* summary, pgo_mixture_round* rounds, int32_t rounds_cap);
  // absolute pose priors (pgo_set_priors, pgo_get_prior_residuals; solver_prior.hip, prior.hip.h, prior.h).  pri_tab = the
  // priors in force sorted by internal row -- row [n] | caller's position [n] | mean planes [3][n] | information planes [6][n] |
  // the record of k_prior_eval<true> [9][n] --, pri_out = the outputs of pgo_get_prior_residuals; both are grown on demand and
  // kept (reserve).  pri_dense = the scaled blocks as dense planes [6][n_loc] for the direct solve's k_dlr_setup: allocated at
  // the first pgo_set_priors of a handle whose plan allows the direct solve, zeroed whenever the priors change.
  int32_t pri_n = 0;
  std::vector<int32_t> pri_pd_rows;   // internal rows of the positive definite priors: each is a gauge while its pose is free (has_anchor)
  pgo::LossClass pri_loss = {};
  pgo::Scratch pri_tab, pri_out;
  double* pri_dense = nullptr;
  pgo::Span<int32_t> pri_row_s, pri_order_s;
  pgo::Span<double> pri_mean_s, pri_info_s, pri_rec_s;
  int set_priors(int32_t n, const int32_t* pose, const double* mean_xyt, const double* info6, const pgo_loss* loss_or_null);
  int get_prior_residuals(const double* poses_or_null, double* d_out, double* chi2_out);
  // the two launch helpers (solver_launch.hip); called with pri_n > 0 only -- a handle without priors launches neither kernel
  int prior_grid() const { return (int)std::min<int64_t>(((int64_t)pri_n + dev::WG - 1) / dev::WG, dev::PRIOR_MAX_GRID); }
  int prior_eval_enqueue(const double* x, int apply_loss, bool with_jac, double* cost_part, double* d_out = nullptr, double* chi2_out = nullptr);
  int prior_add_enqueue();
  dev::SwitchArrays switch_arrays() const {
    dev::SwitchArrays W;
    W.flags = e_flags;
    W.n_edges = S.n_edges_local;
    W.lambda = opt.sc_prior_lambda;
    W.sw = sw;
    W.cand = sw_cand;
    W.js = sw_js;
    W.sigma = sw_sigma;
    W.c = sw_c;
    W.gamma = sw_gamma;
    W.gs = sw_gs;
    W.den = sw_den;
    W.hss = sw_hss;
    return W;
  }
  void launch_eval(const double* x, const double* sw_vals, int apply_loss, bool with_jac);
  // evaluates at x; on return h_scal[slot] = cost, h_scal[slot+1] = #bad flags (needs fetch by caller)
  int eval_enqueue(const double* x, const double* sw_vals, int apply_loss, bool with_jac, int slot);

  // ---- K2
  dev::AsmArgs asm_args() const {
    dev::AsmArgs A;
    A.jr = jr;
    A.inc_ptr = inc_ptr;
    A.inc_edge = inc_edge;
    A.inc_col = inc_col;
    A.tile_row = tile_row;
    A.inc_rowoff = inc_rowoff;
    A.tile_desc = tile_desc;
    A.scale = scale;
    A.n_tiles = S.n_tiles();
    A.n_loc = S.n_loc;
    A.lo = S.lo;
    A.inc_stride = plan.own.inc_stride;
    A.hoff = hoff;
    A.hd = hd;
    A.gs = gs;
    A.sw_js = sw_js;
    A.sw_c = sw_c;
    A.sw_gamma = sw_gamma;
    A.diag_full = diag_full;
    A.gs_full = gs_full;
    A.chain_rec = plan.all.chain_len ? chain_c : nullptr;
    A.chain_seg = plan.all.chain_len ? plan.all.chain_len : 1;
    return A;
  }
  int assemble_enqueue();

  // ---- K3
  dev::SpmvArgs spmv_args(const double* p, double* yout, double* dot_part, int with_d2, const int32_t* done) const {
    dev::SpmvArgs A;
    A.inc_ptr = inc_ptr;
    A.inc_col = inc_col;
    A.tile_row = tile_row;
    A.tile_desc = tile_desc;
    A.n_tiles = S.n_tiles();
    A.n_loc = S.n_loc;
    A.lo = S.lo;
    A.with_d2 = with_d2;
    A.nt = 1;   // non-temporal H-stream loads in k_spmv: 179 -> 166 us at 1M poses
    A.inc_stride = plan.own.inc_stride;
    A.hoff = hoff;
    A.hd = hd;
    A.d2 = d2;
    A.hdd = hdd;
    A.p = p;
    A.y = yout;
    A.dot_part = dot_part;
    A.done = done;
    A.z = nullptr;
    A.p_new = nullptr;
    A.part_rz = A.part_rr = nullptr;
    A.n_rz = A.n_rr = A.parity = 0;
    A.st = nullptr;
    return A;
  }
  int spmv_enqueue(const double* p, double* yout, double* dot_part, int with_d2, const int32_t* done);

  // PCG step "make p visible to the peers, then A p" with the halo exchange hidden behind the interior tiles.
  // *n_part = number of dot partials written to dot_part.
  int spmv_with_halo(double* full, double* yout, double* dot_part, const int32_t* done, int* n_part);

  dev::CgVec cg_vec(double* z_out = nullptr) const {   // z_out: where z = M^-1 r goes instead of the handle's z
    dev::CgVec V;
    V.n_loc = S.n_loc;
    V.lo = S.lo;
    V.minv = minv;
    V.y = y;
    V.r = r;
    V.z = z_out ? z_out : z;
    V.ap = ap;
    V.p = p_full;
    V.st = st;
    V.fused = 0;
    V._pad = 0;
    return V;
  }

  dev::ChainPre chain_pre() const {
    dev::ChainPre CP;
    CP.cw = chain_w;
    CP.cs = chain_s;
    CP.n_loc = S.n_loc;
    CP.n_pad = plan.own.chain_pad;
    return CP;
  }
  dev::GroupPre group_pre() const {
    dev::GroupPre GP;
    GP.ginv = ginv;
    GP.B = plan.own.grp_B;
    GP.nb = plan.own.grp_nb;
    GP.nb_pad = plan.own.grp_pad;
    GP.n_groups = plan.own.n_groups;
    return GP;
  }
  // ---- launched once (solver_launch.hip)
  // z = M^-1 b with the handle's preconditioner.  First level: the PCG start-up kernel of the handle's family (chain, pose
  // groups, 3x3 blocks); it also starts y, r and the gather vector and writes cg_init_parts() partials of r.z and b.b.
  int cg_init_parts() const { return plan.all.chain_len > 0 ? plan.own.g_chain : (plan.own.grp_B > 1 ? plan.own.g_grp : plan.own.g_vec); }
  int launch_cg_init(const double* b, double* z_out, double* part_rz, double* part_bb);
  // the coarse level's share P e_c added to z (and to the gather vector p, unless null), one rank or several
  int launch_coarse_prolong(double* z_inout, double* p_or_null);
  // both levels: launch_cg_init into part[0] / part[1], then (coarse_on()) coarse_solve with its partials of r_c . e_c in
  // dot_part, then the prolongation.  Several ranks: r_c comes with the all-reduce of the start-up sums (coarse_restrict_reduce).
  int precondition(const double* b, double* z_out, double* p_or_null, double* dot_part);
  void launch_cg_sr_chain(const dev::CgVec& V, double* part_gamma, double* part_rr);
  void launch_cg_update1_chain(const dev::CgVec& V, int par, const double* pap, int n_pap, double* part_rz, double* part_rr);
  // Jacobi scales from the diagonal of J'J: pass 0 writes unit scales (0 on the constant poses), pass 1 the column norms
  int launch_jacobi_scale(int pass);
  int scatter_owned(const double* src);   // the owned rows of src into the gather vector p_full
  // METHOD 2: the switches' elimination coefficients for `radius` (partials: part[2] max |g_s|, part[3] sum s^2; g_sw() each)
  int g_sw() const { return std::min(std::max(1, (S.n_edges_local + dev::WG - 1) / dev::WG), 1024); }
  int switch_prepare(double radius);

  // window solves (pgo_window_solve, solver_window.hip): the lists of a call are resolved on the host into win_host, uploaded
  // into win_in; win_work holds the per-edge records and the outputs.  Both buffers are grown on demand and kept.
  std::vector<int32_t> win_edge_local;      // caller's edge -> local edge (built at the first call)
  std::vector<int32_t> win_pos, win_owner;  // row -> list position in the window being resolved / window that lists it (-1 when idle)
  std::vector<uint8_t> win_host;            // host image of win_in
  std::vector<uint32_t> win_sort;
  pgo::Scratch win_in, win_work;
  bool win_lds_set = false;
  // pose_idx / edge_idx / anchor: this handle's caller numbering (a batch: the union's); `who` prefixes the error texts
  int window_solve(const char* who, int32_t n_windows, const int32_t* pose_ptr, const int32_t* pose_idx, const int32_t* edge_ptr,
                   const int32_t* edge_idx, const int32_t* anchor, int32_t max_iters, int32_t commit, double* poses_out,
                   pgo_window_result* results, pgo_iter_record* records);

  // scoring (pgo_trajectory_error, pgo_edge_weights; solver_score.hip): score_in stages what a call uploads (the reference and
  // the mask, or the caller's poses), score_work holds the partials and the outputs; both are grown on demand and kept
  // (reserve).  score_perm / score_eorig: device copies of perm and of S.orig_edge, made at the first call that needs them.
  pgo::Scratch score_in, score_work;
  int32_t *score_perm = nullptr, *score_eorig = nullptr;
  int perm_device(const int32_t** out = nullptr) {   // *out = the device copy of perm, made at its first use; nullptr: the identity
    if (!perm.empty() && !score_perm) {
      PGOC(dalloc(&score_perm, (int64_t)S.n_poses));
      PGOC(upload(score_perm, perm));
    }
    if (out) *out = perm.empty() ? nullptr : score_perm;
    return PGO_OK;
  }
  std::vector<uint8_t> score_host;   // host image of score_in
  int trajectory_error(const double* ref, const uint8_t* mask, const pgo_traj_options* opt, pgo_traj_error* out, double* per_pose);
  int edge_weights(const double* poses_or_null, pgo_edge_weight* out);

  // hierarchical initialisation (pgo_coarsen, pgo_prolong; solver_coarsen.hip).  The tables in the caller's numbering are built
  // at the first call and kept: cs_tab = chain [N] | endpoints a [E] | b [E] | local edge [E] (-1: a chain edge) | kind bytes [E].
  // cs_comp holds C (N x 3) and Cend of stride cs_stride (0: none yet), cs_work the scan scratch and the outputs of a call (or the
  // coarse poses pgo_prolong uploads); both are grown on demand and kept (reserve).  The device copy of perm is perm_device's.
  bool cs_ready = false;
  std::vector<int32_t> cs_ea_h, cs_eb_h, cs_loc_h;
  int32_t* cs_tab = nullptr;
  const int32_t* cs_chain() const { return cs_tab; }
  const int32_t* cs_ea() const { return cs_chain() + S.n_poses; }
  const int32_t* cs_eb() const { return cs_ea() + n_edges_total; }
  const int32_t* cs_eloc() const { return cs_eb() + n_edges_total; }
  const uint8_t* cs_ekind() const { return reinterpret_cast<const uint8_t*>(cs_eloc() + n_edges_total); }
  pgo::Scratch cs_comp, cs_work;
  int32_t cs_stride = 0;
  std::vector<uint8_t> cs_host;   // host image of a call's outputs
  int64_t cs_bad = -1;            // the smallest edge whose measurement is not finite (-1: none), found when the tables were built
  int coarsen_tables(const char* who, bool all_finite = true);   // all_finite: such an edge is PGO_ERR_NUMERIC
  // with_info (pgo_coarsen_info): cs_cov = the covariances of C | of Cend, cs_wbad[e] = the information of caller's edge e fails
  // gate_chol3 (found once, on the host)
  pgo::Scratch cs_cov;
  std::vector<uint8_t> cs_wbad;
  bool cs_wbad_ready = false;
  int coarsen_info_check();
  int coarsen(int32_t stride, pgo_graph** coarse_out, int32_t* origin, int32_t origin_cap, int32_t* n_coarse_edges, bool with_info = false,
              double* cov = nullptr);
  int prolong(int32_t stride, const double* coarse_xyt);

  // loop support (pgo_loop_support; solver_support.hip).  It walks the tables of pgo_coarsen (cs_tab).  ls_traj = the trajectory
  // T (N x 5) | the segment ends | the key poses, computed at the first call and kept (measurements never change on a handle).
  // ls_tab = the table of a selection -- the loops sorted by (lo, edge) | first [N + 1] | slot of every edge | M^-1 per slot --,
  // built on the host at the first call for that selection (ls_sel_h: its bytes) and kept; ls_work = a call's per-slot results,
  // records, chunk totals and statistics.  Both are grown on demand and kept (reserve).
  bool ls_traj_ready = false, ls_tab_ready = false;
  double* ls_traj = nullptr;
  std::vector<uint8_t> ls_sel_h;
  int32_t ls_n_sel = 0;
  pgo::Scratch ls_tab, ls_work;
  std::vector<uint8_t> ls_host;   // host image of a call's outputs
  int loop_support(const pgo_loop_support_options* o, const uint8_t* select_or_null, pgo_loop_support_record* out, pgo_loop_support_stats* stats);
  int support_trajectory_alloc();     // ls_traj, before anything is enqueued
  int support_trajectory_enqueue();   // T's three launches unless ls_traj_ready (the caller sets it after its synchronisation)

  // chordal initialisation (pgo_chordal_init; solver_chordal.hip).  It starts from the trajectory above and walks the tables of
  // pgo_coarsen.  ch_tab = the slot table -- rp [N + 1] | col | edge and orientation per slot | caller's edge -> local edge [E] --,
  // built on the host at the first call and kept (ch_slots: its slot count); ch_work = a call's
  // weights, mask, system, PCG vectors, partials, state and outputs.  Both are grown on demand and kept (reserve).
  bool ch_tab_ready = false;
  int64_t ch_slots = 0;
  pgo::Scratch ch_tab, ch_work;
  std::vector<uint8_t> ch_host;   // host image of a call's uploads, then of its outputs
  int chordal_init(const pgo_chordal_options* o, double* poses_out, double* res_out, pgo_chordal_summary* summary);

  int create(int32_t N, const double* poses_h, int32_t E, const int32_t* ia, const int32_t* ib, const double* meas,
             const double* info6, const uint8_t* kind);
  int linearize(bool reuse_records, bool assemble = true);
  int refresh_switch_system();
  int lm_begin();
  int lm_iteration(bool* stop);
  int lm_iteration_tail(bool* stop, pgo_iter_record& R, double it0, double t0, int k_it, double rel);
  // LM diagonal for `radius` (a batched handle: per problem, prob_radius) + the PCG preconditioner's set-up -- which a handle on
  // the direct solve skips unless it is asked for
  int prepare_system(double radius, bool preconditioner_also_on_direct = false);
  int pcg(int* iters, double* rel);
  int32_t direct_chain_lists(std::vector<int32_t>* chain, std::vector<int32_t>* lr, std::vector<int32_t>* va, std::vector<int32_t>* vb) const;
  int direct_build();   // the buffers and lists of the direct solve the plan sized (create, or lm_iteration's take-over)
  int direct_solve();
  int direct_enqueue(const double* rhs, int refine);
  struct DirectLaunch {   // the argument blocks of a factorisation's launches, for the solves that follow it
    dev::DlrArgs A;
    dev::DlrColsArgs C;
    dev::DlrSepArgs SA;
  };
  int direct_factor(const double* rhs, bool fine_prefix, DirectLaunch* L);
  int direct_sweep(const dev::DlrColsArgs& Q, bool panel_rhs = false);
  int direct_separator_fix(const dev::DlrSepArgs& SA, double* X, int ld, int ncols);
  struct DirectPanel {   // ld columns at once (a multiple of 64): T [3n][ld] right-hand sides in, solutions out
    double *T, *E, *E2;  // E, E2 [dl_nseg][3][ld]
    double *Wm;          // [dl_nU][ld]
    double *G, *Y;       // [dl_Kp][ld]
    int ld;
  };
  int direct_panel_solve(const DirectLaunch& L, const DirectPanel& P);
  int factor_chain();
  int prepare_preconditioner();
  void fill_summary(pgo_summary* s) const;
};

