// Scoring a solve on the device (include/pgo.h, "scoring"): pgo_trajectory_error and pgo_edge_weights -- the host halves.  The
// poses stay where they are, in the handle's internal ordering; the reference and the mask go up in one staging buffer, the
// kernels of score.hip.h walk the caller's numbering, and one copy-out ends the call.  Neither call touches the LM state, the
// record buffer or the candidate poses.  pgo_trajectory_error_eval, the serial host evaluation of the same statement
// (traj_error.h), lives here too.
#include "solver_handle.hip.h"
#include "score.hip.h"

namespace {
int check_traj_options(const char* who, const pgo_traj_options* opt, pgo_traj_options* o) {
  pgo_traj_options_default(o);
  if (opt) *o = *opt;
  if (o->align != 0 && o->align != 1) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": align must be 0 or 1");
  if (o->rpe_delta < 0) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": rpe_delta < 0");
  return PGO_OK;
}
struct TrajOut {   // what k_traj_fold<2> leaves: the record, and behind it the first pose that is not finite (-1: none)
  pgo_traj_error e;
  int32_t bad, _pad;
};
static_assert(sizeof(TrajOut) == sizeof(pgo_traj_error) + 8, "the index sits right behind the record");
}  // namespace

int pgo_handle::trajectory_error(const double* ref, const uint8_t* mask, const pgo_traj_options* opt, pgo_traj_error* out,
                                 double* per_pose) {
  const char* who = "pgo_trajectory_error";
  PGOC(requires(who, ONE_RANK | NOT_BATCH));
  if (!ref || !out) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": null pointer");
  pgo_traj_options o;
  PGOC(check_traj_options(who, opt, &o));
  HIPC(hipSetDevice(device));
  const int64_t N = S.n_poses;
  const int64_t nc = (N + dev::SCORE_CHUNK - 1) / dev::SCORE_CHUNK;
  // ---- buffers, before anything is enqueued: staging = state | ref | mask;  work = out (+ the index) | psum | pmax | pidx | per-pose
  pgo::Layout LI, LW;
  const auto i_state = LI.add<double>(dev::SCORE_STATE), i_ref = LI.add<double>(3 * N);
  const auto i_mask = LI.add<uint8_t>(mask ? N : 0);
  const auto w_out = LW.add<TrajOut>(1);
  const auto w_psum = LW.add<double>(dev::SCORE_NSUM * nc), w_pmax = LW.add<double>(dev::SCORE_NMAX * nc);
  const auto w_pidx = LW.add<int32_t>(dev::SCORE_NIDX * nc);
  const auto w_pp = LW.add<double>(per_pose ? 2 * N : 0);
  PGOC(reserve(score_in, LI.bytes()));
  PGOC(reserve(score_work, LW.bytes()));
  dev::TrajArgs A;
  PGOC(perm_device(&A.perm));
  // ---- upload
  score_host.assign((size_t)LI.bytes(), 0);
  i_state.in(score_host.data())[6] = 1.0;   // the identity transform (phi, c, s, tx, ty at 5..9): what the error pass reads when
                                            // no alignment runs
  memcpy(i_ref.in(score_host.data()), ref, (size_t)i_ref.bytes());
  if (mask) memcpy(i_mask.in(score_host.data()), mask, (size_t)N);
  HIPC(hipMemcpyAsync(score_in.p, score_host.data(), score_host.size(), hipMemcpyHostToDevice, stream));
  A.est = poses;
  A.ref = i_ref.in(score_in.p);
  A.mask = mask ? i_mask.in(score_in.p) : nullptr;
  A.n = (int32_t)N;
  A.n_chunks = (int32_t)nc;
  A.delta = o.rpe_delta;
  A._pad = 0;
  A.psum = w_psum.in(score_work.p);
  A.pmax = w_pmax.in(score_work.p);
  A.pidx = w_pidx.in(score_work.p);
  A.state = i_state.in(score_in.p);
  A.per_pose = per_pose ? w_pp.in(score_work.p) : nullptr;
  A.out = &w_out.in(score_work.p)->e;
  const int grid = launch_grid("score_grid", nc);
  if (o.align) {
    hipLaunchKernelGGL(dev::k_traj_centroid<>, dim3(grid), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_traj_centroid"));
    hipLaunchKernelGGL(dev::k_traj_fold<0>, dim3(1), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_traj_fold<0>"));
    hipLaunchKernelGGL(dev::k_traj_moments<>, dim3(grid), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_traj_moments"));
    hipLaunchKernelGGL(dev::k_traj_fold<1>, dim3(1), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_traj_fold<1>"));
  }
  hipLaunchKernelGGL(dev::k_traj_errors<>, dim3(grid), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_traj_errors"));
  hipLaunchKernelGGL(dev::k_traj_fold<2>, dim3(1), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_traj_fold<2>"));
  // ---- one copy-out: the record with the index behind it, and the per-pose array
  TrajOut res;
  std::vector<double> pp;
  HIPC(hipMemcpyAsync(&res, w_out.in(score_work.p), sizeof res, hipMemcpyDeviceToHost, stream));
  if (per_pose) {
    pp.resize((size_t)(2 * N));
    HIPC(hipMemcpyAsync(pp.data(), A.per_pose, (size_t)w_pp.bytes(), hipMemcpyDeviceToHost, stream));
  }
  PGOC(sync());
  if (res.bad >= 0) return fail(PGO_ERR_NUMERIC, std::string(who) + ": pose " + std::to_string(res.bad) + " is not finite");
  *out = res.e;
  if (per_pose) memcpy(per_pose, pp.data(), (size_t)(2 * N * 8));
  return PGO_OK;
}

int pgo_handle::edge_weights(const double* poses_or_null, pgo_edge_weight* out) {
  const char* who = "pgo_edge_weights";
  if (const int s = requires(who, METHOD_01)) return fail(s, std::string(pgo_last_error()) + " (METHOD 2: pgo_get_switches)");
  PGOC(requires(who, NO_INFO | ONE_RANK | NOT_BATCH));
  if (!out) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": null pointer");
  HIPC(hipSetDevice(device));
  const int64_t N = S.n_poses, EL = S.n_edges_local;   // (one rank: every edge is local)
  if (EL == 0) return PGO_OK;
  pgo::Layout LI, LW;   // staging = the caller's poses;  work = the records
  const auto i_x = LI.add<double>(poses_or_null ? 3 * N : 0);
  const auto w_rec = LW.add<pgo_edge_weight>(EL);
  if (poses_or_null) PGOC(reserve(score_in, LI.bytes()));
  PGOC(reserve(score_work, LW.bytes()));
  if (!score_eorig) {
    PGOC(dalloc(&score_eorig, EL));
    PGOC(upload(score_eorig, S.orig_edge));
  }
  const double* x = poses;
  if (poses_or_null) {   // (the handle's candidate buffer belongs to the LM loop: the caller's poses go through the staging buffer)
    score_host.resize((size_t)LI.bytes());
    double* hp = i_x.in(score_host.data());
    if (perm.empty()) memcpy(hp, poses_or_null, (size_t)i_x.bytes());
    else
      for (int64_t i = 0; i < N; ++i) memcpy(hp + 3 * (int64_t)perm[i], poses_or_null + 3 * i, 3 * sizeof(double));
    HIPC(hipMemcpyAsync(score_in.p, hp, (size_t)i_x.bytes(), hipMemcpyHostToDevice, stream));
    x = i_x.in(score_in.p);
  }
  dev::EdgeArgs A = edge_args(x, nullptr, 0);
  const int grid = (int)std::min<int64_t>((EL + dev::WG - 1) / dev::WG, 8192);
  hipLaunchKernelGGL(dev::k_edge_weights<>, dim3(grid), dim3(dev::WG), 0, stream, A, (int32_t)(opt.method == 1), (const int32_t*)score_eorig,
                     w_rec.in(score_work.p));
  PGOC(check_launch("k_edge_weights"));
  std::vector<pgo_edge_weight> tmp((size_t)EL);   // (nothing reaches the caller's array unless the whole call succeeds)
  HIPC(hipMemcpyAsync(tmp.data(), w_rec.in(score_work.p), (size_t)w_rec.bytes(), hipMemcpyDeviceToHost, stream));
  PGOC(sync());
  memcpy(out, tmp.data(), (size_t)w_rec.bytes());
  return PGO_OK;
}

extern "C" {

void pgo_traj_options_default(pgo_traj_options* o) {
  if (!o) return;
  o->align = 0;
  o->rpe_delta = 1;
}

int pgo_trajectory_error_eval(int32_t n, const double* est, const double* ref, const uint8_t* mask, const pgo_traj_options* opt,
                              pgo_traj_error* out, double* per_pose) {
  const char* who = "pgo_trajectory_error_eval";
  if (!est || !ref || !out) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": null pointer");
  if (n < 1) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": n < 1");
  pgo_traj_options o;
  PGOC(check_traj_options(who, opt, &o));
  const int64_t bad = pgo::traj_error_serial(n, est, ref, mask, o.align, o.rpe_delta, out, per_pose);
  if (bad >= 0) return fail(PGO_ERR_NUMERIC, std::string(who) + ": pose " + std::to_string(bad) + " is not finite");
  return PGO_OK;
}

int pgo_trajectory_error(pgo_t* h, const double* ref, const uint8_t* mask, const pgo_traj_options* opt, pgo_traj_error* out,
                         double* per_pose) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_trajectory_error: null handle");
  return h->trajectory_error(ref, mask, opt, out, per_pose);
}

int pgo_edge_weights(pgo_t* h, const double* poses_or_null, pgo_edge_weight* out) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_edge_weights: null handle");
  return h->edge_weights(poses_or_null, out);
}

}  // extern "C"
