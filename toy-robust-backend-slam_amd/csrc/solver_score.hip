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
int64_t up16(int64_t b) { return (b + 15) / 16 * 16; }
}  // namespace

int pgo_handle::trajectory_error(const double* ref, const uint8_t* mask, const pgo_traj_options* opt, pgo_traj_error* out,
                                 double* per_pose) {
  const char* who = "pgo_trajectory_error";
  if (comm || force_collectives) return fail(PGO_ERR_UNSUPPORTED, std::string(who) + ": one rank without a communicator only");
  if (batch_mode) return fail(PGO_ERR_UNSUPPORTED, std::string(who) + ": not on a batched handle");
  if (!ref || !out) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": null pointer");
  pgo_traj_options o;
  PGOC(check_traj_options(who, opt, &o));
  const long long grid_knob = knob("score_grid");
  HIPC(hipSetDevice(device));
  const int64_t N = S.n_poses;
  const int64_t nc = (N + dev::SCORE_CHUNK - 1) / dev::SCORE_CHUNK;
  // ---- buffers, before anything is enqueued: staging = state | ref | mask;  work = out (+ the index) | psum | pmax | pidx | per-pose
  const int64_t i_state = 0, i_ref = i_state + dev::SCORE_STATE * 8, i_mask = i_ref + 3 * N * 8, i_all = i_mask + (mask ? up16(N) : 0);
  const int64_t w_out = 0, w_psum = w_out + up16((int64_t)sizeof(pgo_traj_error) + 8),
                w_pmax = w_psum + dev::SCORE_NSUM * nc * 8, w_pidx = w_pmax + dev::SCORE_NMAX * nc * 8,
                w_pp = up16(w_pidx + dev::SCORE_NIDX * nc * 4), w_all = w_pp + (per_pose ? 2 * N * 8 : 0);
  PGOC(win_reserve(&score_in, &score_in_cap, i_all));
  PGOC(win_reserve(&score_work, &score_work_cap, w_all));
  if (!perm.empty() && !score_perm) {
    PGOC(dalloc(&score_perm, N));
    PGOC(upload(score_perm, perm));
  }
  // ---- upload
  score_host.assign((size_t)i_all, 0);
  reinterpret_cast<double*>(score_host.data() + i_state)[6] = 1.0;   // the identity transform (phi, c, s, tx, ty at 5..9): what the
                                                                      // error pass reads when no alignment runs
  memcpy(score_host.data() + i_ref, ref, (size_t)(3 * N * 8));
  if (mask) memcpy(score_host.data() + i_mask, mask, (size_t)N);
  HIPC(hipMemcpyAsync(score_in, score_host.data(), (size_t)i_all, hipMemcpyHostToDevice, stream));
  char* wk = static_cast<char*>(score_work);
  dev::TrajArgs A;
  A.est = poses;
  A.perm = perm.empty() ? nullptr : score_perm;
  A.ref = reinterpret_cast<const double*>(static_cast<char*>(score_in) + i_ref);
  A.mask = mask ? reinterpret_cast<const uint8_t*>(static_cast<char*>(score_in) + i_mask) : nullptr;
  A.n = (int32_t)N;
  A.n_chunks = (int32_t)nc;
  A.delta = o.rpe_delta;
  A._pad = 0;
  A.psum = reinterpret_cast<double*>(wk + w_psum);
  A.pmax = reinterpret_cast<double*>(wk + w_pmax);
  A.pidx = reinterpret_cast<int32_t*>(wk + w_pidx);
  A.state = reinterpret_cast<double*>(static_cast<char*>(score_in) + i_state);
  A.per_pose = per_pose ? reinterpret_cast<double*>(wk + w_pp) : nullptr;
  A.out = reinterpret_cast<pgo_traj_error*>(wk + w_out);
  const int grid = (int)(grid_knob > 0 ? std::min<long long>(grid_knob, 65535) : std::min<int64_t>(nc, 65535));
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
  struct {
    pgo_traj_error e;
    int32_t bad, _pad;
  } res;
  static_assert(sizeof res == sizeof(pgo_traj_error) + 8, "the index sits right behind the record");
  std::vector<double> pp;
  HIPC(hipMemcpyAsync(&res, wk + w_out, sizeof res, hipMemcpyDeviceToHost, stream));
  if (per_pose) {
    pp.resize((size_t)(2 * N));
    HIPC(hipMemcpyAsync(pp.data(), wk + w_pp, (size_t)(2 * N * 8), hipMemcpyDeviceToHost, stream));
  }
  PGOC(sync());
  if (res.bad >= 0) return fail(PGO_ERR_NUMERIC, std::string(who) + ": pose " + std::to_string(res.bad) + " is not finite");
  *out = res.e;
  if (per_pose) memcpy(per_pose, pp.data(), (size_t)(2 * N * 8));
  return PGO_OK;
}

int pgo_handle::edge_weights(const double* poses_or_null, pgo_edge_weight* out) {
  const char* who = "pgo_edge_weights";
  if (opt.method != 0 && opt.method != 1) return fail(PGO_ERR_UNSUPPORTED, std::string(who) + ": METHOD 0 and 1 only (METHOD 2: pgo_get_switches)");
  if (opt.info_weighting || info_mode) return fail(PGO_ERR_UNSUPPORTED, std::string(who) + ": info_weighting is not supported");
  if (comm || force_collectives) return fail(PGO_ERR_UNSUPPORTED, std::string(who) + ": one rank without a communicator only");
  if (batch_mode) return fail(PGO_ERR_UNSUPPORTED, std::string(who) + ": not on a batched handle");
  if (!out) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": null pointer");
  HIPC(hipSetDevice(device));
  const int64_t N = S.n_poses, EL = S.n_edges_local;   // (one rank: every edge is local)
  if (EL == 0) return PGO_OK;
  const int64_t w_all = EL * (int64_t)sizeof(pgo_edge_weight);
  if (poses_or_null) PGOC(win_reserve(&score_in, &score_in_cap, 3 * N * 8));
  PGOC(win_reserve(&score_work, &score_work_cap, w_all));
  if (!score_eorig) {
    PGOC(dalloc(&score_eorig, EL));
    PGOC(upload(score_eorig, S.orig_edge));
  }
  const double* x = poses;
  if (poses_or_null) {   // (the handle's candidate buffer belongs to the LM loop: the caller's poses go through the staging buffer)
    score_host.resize((size_t)(3 * N * 8));
    double* hp = reinterpret_cast<double*>(score_host.data());
    if (perm.empty()) memcpy(hp, poses_or_null, (size_t)(3 * N * 8));
    else
      for (int64_t i = 0; i < N; ++i) memcpy(hp + 3 * (int64_t)perm[i], poses_or_null + 3 * i, 3 * sizeof(double));
    HIPC(hipMemcpyAsync(score_in, hp, (size_t)(3 * N * 8), hipMemcpyHostToDevice, stream));
    x = static_cast<const double*>(score_in);
  }
  dev::EdgeArgs A = edge_args(x, nullptr, 0);
  const int grid = (int)std::min<int64_t>((EL + dev::WG - 1) / dev::WG, 8192);
  hipLaunchKernelGGL(dev::k_edge_weights<>, dim3(grid), dim3(dev::WG), 0, stream, A, (int32_t)(opt.method == 1), (const int32_t*)score_eorig,
                     static_cast<pgo_edge_weight*>(score_work));
  PGOC(check_launch("k_edge_weights"));
  std::vector<pgo_edge_weight> tmp((size_t)EL);   // (nothing reaches the caller's array unless the whole call succeeds)
  HIPC(hipMemcpyAsync(tmp.data(), score_work, (size_t)w_all, hipMemcpyDeviceToHost, stream));
  PGOC(sync());
  memcpy(out, tmp.data(), (size_t)w_all);
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
