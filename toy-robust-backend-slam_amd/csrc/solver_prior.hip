// Absolute pose priors (include/pgo.h, "pose priors"): the host halves of pgo_set_priors and pgo_get_prior_residuals, and
// pgo_prior_eval, the host evaluation of the same statement (prior.h).  The kernels (prior.hip.h) are launched from the two
// choke points every evaluation and assembly passes through, eval_enqueue and assemble_enqueue (solver_launch.hip).
#include "solver_handle.hip.h"
#include "prior.hip.h"

// every argument is checked before anything changes; then the table is rewritten, sorted by internal row, and the running solve
// (if any) is stale.  n = 0: no priors -- neither kernel is launched again and the handle computes what a fresh one does.
int pgo_handle::set_priors(int32_t n, const int32_t* pose, const double* mean, const double* info6, const pgo_loss* loss) {
  const std::string who = "pgo_set_priors";
  PGOC(requires(who.c_str(), METHOD_01 | ONE_RANK | NOT_BATCH));
  if (n < 0) return fail(PGO_ERR_INVALID_ARG, who + ": n < 0");
  if (n > 0 && (!pose || !mean || !info6)) return fail(PGO_ERR_INVALID_ARG, who + ": null pointer");
  if (loss && !pgo::loss_valid(*loss)) return fail(PGO_ERR_INVALID_ARG, who + ": loss: unknown type or a scale that is not finite and > 0");
  const int64_t N = S.n_poses;
  std::vector<int32_t> pd_rows;
  {
    std::vector<uint8_t> seen((size_t)N, 0);
    for (int32_t k = 0; k < n; ++k) {
      const std::string pk = who + ": prior " + std::to_string(k) + ": ";
      if (pose[k] < 0 || pose[k] >= N) return fail(PGO_ERR_INVALID_ARG, pk + "pose " + std::to_string(pose[k]) + " out of range");
      if (seen[pose[k]]) return fail(PGO_ERR_INVALID_ARG, pk + "pose " + std::to_string(pose[k]) + " already has a prior (at most one per pose)");
      seen[pose[k]] = 1;
      for (int c = 0; c < 3; ++c)
        if (!std::isfinite(mean[3 * (int64_t)k + c])) return fail(PGO_ERR_INVALID_ARG, pk + "the mean is not finite");
      const pgo::PriorInfoClass cls = pgo::prior_info_class(info6 + 6 * (int64_t)k);
      if (cls == pgo::PRIOR_INFO_NOT_FINITE) return fail(PGO_ERR_INVALID_ARG, pk + "the information is not finite");
      if (cls == pgo::PRIOR_INFO_INDEFINITE)
        return fail(PGO_ERR_INVALID_ARG, pk + "the information has a negative eigenvalue (positive semi-definite required)");
      if (cls == pgo::PRIOR_INFO_PD) pd_rows.push_back(perm.empty() ? pose[k] : perm[pose[k]]);
    }
  }
  if (n == 0) {   // (the buffers are kept)
    pri_n = 0;
    pri_pd_rows.clear();
    solve_is_stale();
    return PGO_OK;
  }
  HIPC(hipSetDevice(device));
  // ---- the table, sorted by internal row (rows are unique: the order is total)
  std::vector<int32_t> order((size_t)n);
  for (int32_t k = 0; k < n; ++k) order[k] = k;
  auto row_of = [&](int32_t k) { return perm.empty() ? pose[k] : perm[pose[k]]; };
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return row_of(a) < row_of(b); });
  pgo::Layout L;
  const auto s_row = L.add<int32_t>(n);   // (the upload: s_row to s_info)
  const auto s_order = L.add<int32_t>(n);
  const auto s_mean = L.add<double>(3 * (int64_t)n);
  const auto s_info = L.add<double>(6 * (int64_t)n);
  const auto s_rec = L.add<double>((int64_t)dev::PRIOR_REC * n);
  std::vector<uint8_t> host((size_t)s_info.end(), 0);
  {
    int32_t* row_h = s_row.in(host.data());
    int32_t* order_h = s_order.in(host.data());
    double* mean_h = s_mean.in(host.data());
    double* info_h = s_info.in(host.data());
    for (int32_t j = 0; j < n; ++j) {
      const int32_t k = order[j];
      row_h[j] = row_of(k);
      order_h[j] = k;
      for (int c = 0; c < 3; ++c) mean_h[(size_t)c * n + j] = mean[3 * (int64_t)k + c];
      for (int c = 0; c < 6; ++c) info_h[(size_t)c * n + j] = info6[6 * (int64_t)k + c];
    }
  }
  // ---- device buffers, before anything changes
  if (plan.own.g_edge + dev::PRIOR_MAX_GRID > plan.own.part_cap)   // (plan.h sizes part_cap for it: the partials are appended to K1's)
    return fail(PGO_ERR_UNSUPPORTED, who + ": no room for the cost partials behind K1's");
  const bool may_solve_directly = plan.dl.direct || plan.dl.dl_possible;
  if (may_solve_directly && !pri_dense) PGOC(dalloc(&pri_dense, 6 * (int64_t)S.n_loc));
  PGOC(reserve(pri_tab, L.bytes()));
  // ---- apply
  HIPC(hipMemcpyAsync(pri_tab.p, host.data(), host.size(), hipMemcpyHostToDevice, stream));
  HIPC(hipMemsetAsync(s_rec.in(pri_tab.p), 0, (size_t)s_rec.bytes(), stream));   // (k_prior_eval<true> writes it; never read uninitialised)
  if (pri_dense) HIPC(hipMemsetAsync(pri_dense, 0, (size_t)6 * S.n_loc * sizeof(double), stream));   // rows that lost their prior
  pri_row_s = s_row;
  pri_order_s = s_order;
  pri_mean_s = s_mean;
  pri_info_s = s_info;
  pri_rec_s = s_rec;
  pri_n = n;
  pri_pd_rows.swap(pd_rows);
  pri_loss = loss ? pgo::make_loss_class(loss->type, loss->a) : pgo::make_loss_class(PGO_LOSS_TRIVIAL, 0.0);
  solve_is_stale();
  return sync();   // (`host` dies with this scope)
}

int pgo_handle::get_prior_residuals(const double* poses_or_null, double* d_out, double* chi2_out) {
  const std::string who = "pgo_get_prior_residuals";
  PGOC(requires(who.c_str(), METHOD_01 | ONE_RANK | NOT_BATCH));
  if (pri_n == 0) return PGO_OK;
  HIPC(hipSetDevice(device));
  pgo::Layout L;
  const auto s_d = L.add<double>(3 * (int64_t)pri_n);   // (the download: s_d to s_chi2)
  const auto s_chi2 = L.add<double>(pri_n);
  PGOC(reserve(pri_out, L.bytes()));
  const double* x = poses;
  if (poses_or_null) {
    PGOC(upload_pose_vector(cand, poses_or_null));
    x = cand;
  }
  HIPC(hipMemsetAsync(bad, 0, sizeof(int), stream));
  PGOC(prior_eval_enqueue(x, 0, false, part[5], s_d.in(pri_out.p), s_chi2.in(pri_out.p)));
  std::vector<uint8_t> host((size_t)L.bytes());
  HIPC(hipMemcpyAsync(host.data(), pri_out.p, host.size(), hipMemcpyDeviceToHost, stream));
  PGOC(sync());
  if (d_out) memcpy(d_out, s_d.in(host.data()), (size_t)s_d.bytes());
  if (chi2_out) memcpy(chi2_out, s_chi2.in(host.data()), (size_t)s_chi2.bytes());
  return PGO_OK;
}

// ====================================================================== C-ABI
int pgo_set_priors(pgo_t* h, int32_t n, const int32_t* pose, const double* mean_xyt, const double* info6, const pgo_loss* loss_or_null) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_set_priors: null handle");
  return h->set_priors(n, pose, mean_xyt, info6, loss_or_null);
}

int32_t pgo_num_priors(const pgo_t* h) { return h ? h->pri_n : 0; }

int pgo_get_prior_residuals(pgo_t* h, const double* poses_or_null, double* d_out, double* chi2_out) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_get_prior_residuals: null handle");
  return h->get_prior_residuals(poses_or_null, d_out, chi2_out);
}

int pgo_prior_eval(const double pose[3], const double mean[3], const double info6[6], const pgo_loss* loss_or_null, double d[3],
                   double* chi2, double rho[3]) {
  const std::string who = "pgo_prior_eval";
  if (!pose || !mean || !info6) return fail(PGO_ERR_INVALID_ARG, who + ": null pointer");
  if (loss_or_null && !pgo::loss_valid(*loss_or_null))
    return fail(PGO_ERR_INVALID_ARG, who + ": loss: unknown type or a scale that is not finite and > 0");
  for (int c = 0; c < 3; ++c)
    if (!std::isfinite(pose[c]) || !std::isfinite(mean[c])) return fail(PGO_ERR_INVALID_ARG, who + ": the pose or the mean is not finite");
  const pgo::PriorInfoClass cls = pgo::prior_info_class(info6);
  if (cls == pgo::PRIOR_INFO_NOT_FINITE) return fail(PGO_ERR_INVALID_ARG, who + ": the information is not finite");
  if (cls == pgo::PRIOR_INFO_INDEFINITE)
    return fail(PGO_ERR_INVALID_ARG, who + ": the information has a negative eigenvalue (positive semi-definite required)");
  const pgo::LossClass L = loss_or_null ? pgo::make_loss_class(loss_or_null->type, loss_or_null->a) : pgo::make_loss_class(PGO_LOSS_TRIVIAL, 0.0);
  double dd[3], q[3], s, r[3];
  pgo::prior_eval(L, pose[0], pose[1], pose[2], mean[0], mean[1], mean[2], info6[0], info6[1], info6[2], info6[3], info6[4], info6[5], dd[0],
                  dd[1], dd[2], q[0], q[1], q[2], s, r);
  if (d) memcpy(d, dd, sizeof dd);
  if (chi2) *chi2 = s;
  if (rho) memcpy(rho, r, sizeof r);
  return PGO_OK;
}
