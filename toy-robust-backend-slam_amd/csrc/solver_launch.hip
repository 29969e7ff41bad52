// The handle's launch helpers for the kernels several translation units need (K1, K2, K3, the reductions to scalars, the
// halo exchange, the preconditioner apply z = M^-1 b of both levels, the Jacobi scales, METHOD 2's switch elimination): defined
// ONCE here, so that the other units do not carry copies of those kernels -- and so that a test hook runs the lines the LM loop
// runs.  The caller <-> internal numbering of a pose vector is stated here too.
#include "solver_handle.hip.h"
#include "prior.hip.h"

int pgo_handle::reduce_to_scal(std::initializer_list<PartRef> parts, int first, bool allreduce_max) {
  return reduce_parts(parts, scal + first, scal + first, (int)parts.size(), allreduce_max);
}

// k_finalize of the partial arrays into out[0 .. #parts); several ranks: then the all-reduce of ar[0 .. ar_n), which holds out
int pgo_handle::reduce_parts(std::initializer_list<PartRef> parts, double* out, double* ar, int ar_n, bool allreduce_max) {
  dev::FinArgs F;
  memset(&F, 0, sizeof F);
  int k = 0;
  for (const PartRef& pr : parts) {
    F.part[k] = pr.p;
    F.n[k] = pr.n;
    F.is_max[k] = pr.is_max;
    if (!pr.is_max && pr.n > 4096 && fold_buf) {
      // k_finalize is ONE workgroup: tens of thousands of partials (k_spmv_1: one per tile) go through 16 workgroups first
      hipLaunchKernelGGL(dev::k_fold_partials<>, dim3(16), dim3(dev::WG), 0, stream, pr.p, pr.n, fold_buf + 16 * k, (const int32_t*)nullptr);
      PGOC(check_launch("k_fold_partials"));
      F.part[k] = fold_buf + 16 * k;
      F.n[k] = 16;
    }
    ++k;
  }
  F.count = k;
  F.out = out;
  hipLaunchKernelGGL(dev::k_finalize<>, dim3(1), dim3(dev::WG), 0, stream, F);
  PGOC(check_launch("k_finalize"));
  if (multi_rank()) PGOC(comm->allreduce(ar, ar_n, allreduce_max, stream));
  return PGO_OK;
}

// the halo exchange's two ends: the rows the peers read, out of the gather vector into the send buffer, and the received rows into it
static unsigned halo_rows_grid(int64_t n_rows) { return (unsigned)std::min<int64_t>((3 * n_rows + 255) / 256, 2048); }

int pgo_handle::pack_halo_rows(const double* full) {
  const int64_t ns = (int64_t)S.halo_send_row.size();
  if (ns == 0) return PGO_OK;
  hipLaunchKernelGGL(dev::k_pack_rows<>, dim3(halo_rows_grid(ns)), dim3(256), 0, stream, ns, (const int32_t*)halo_send_rows, full, halo_send_buf);
  return check_launch("k_pack_rows");
}

int pgo_handle::unpack_halo_rows(double* full, hipStream_t on) {
  const int64_t nr = (int64_t)S.halo_recv_row.size();
  if (nr == 0) return PGO_OK;
  hipLaunchKernelGGL(dev::k_unpack_rows<>, dim3(halo_rows_grid(nr)), dim3(256), 0, on, nr, (const int32_t*)halo_recv_rows, (const double*)halo_recv_buf, full);
  return check_launch("k_unpack_rows");
}

int pgo_handle::share_gather_vector(double* full) {
  if (!multi_rank()) return PGO_OK;
  if (!plan.all.use_halo) return allgather(full, dev::PS);
  PGOC(pack_halo_rows(full));
  PGOC(comm->exchange(halo_send_buf, halo_send_off3.data(), halo_recv_buf, halo_recv_off3.data(), stream));
  PGOC(unpack_halo_rows(full, stream));
  return PGO_OK;
}

void pgo_handle::launch_eval(const double* x, const double* sw_vals, int apply_loss, bool with_jac) {
  dev::EdgeArgs A = edge_args(x, sw_vals, apply_loss);
  if (loss_general || act_edges || w_set) {   // per-class losses (pgo_set_losses), an edge mask (pgo_set_active) or a weight plane
                                              // (pgo_set_edge_weights): the general instantiation
    if (info_mode) {
      if (with_jac) hipLaunchKernelGGL((dev::k_edge_eval<true, true, true>), dim3(plan.own.g_edge), dim3(dev::WG), 0, stream, A, jr, part[5], bad);
      else hipLaunchKernelGGL((dev::k_edge_eval<false, true, true>), dim3(plan.own.g_edge), dim3(dev::WG), 0, stream, A, jr, part[5], bad);
    } else {
      if (with_jac) hipLaunchKernelGGL((dev::k_edge_eval<true, false, true>), dim3(plan.own.g_edge), dim3(dev::WG), 0, stream, A, jr, part[5], bad);
      else hipLaunchKernelGGL((dev::k_edge_eval<false, false, true>), dim3(plan.own.g_edge), dim3(dev::WG), 0, stream, A, jr, part[5], bad);
    }
  } else if (info_mode) {
    if (with_jac) hipLaunchKernelGGL((dev::k_edge_eval<true, true>), dim3(plan.own.g_edge), dim3(dev::WG), 0, stream, A, jr, part[5], bad);
    else hipLaunchKernelGGL((dev::k_edge_eval<false, true>), dim3(plan.own.g_edge), dim3(dev::WG), 0, stream, A, jr, part[5], bad);
  } else {
    if (with_jac) hipLaunchKernelGGL((dev::k_edge_eval<true, false>), dim3(plan.own.g_edge), dim3(dev::WG), 0, stream, A, jr, part[5], bad);
    else hipLaunchKernelGGL((dev::k_edge_eval<false, false>), dim3(plan.own.g_edge), dim3(dev::WG), 0, stream, A, jr, part[5], bad);
  }
}

int pgo_handle::eval_enqueue(const double* x, const double* sw_vals, int apply_loss, bool with_jac, int slot) {
  HIPC(hipMemsetAsync(bad, 0, sizeof(int), stream));
  launch_eval(x, sw_vals, apply_loss, with_jac);
  PGOC(check_launch("k_edge_eval"));
  // pose priors (pgo_set_priors): their cost partials are appended to K1's, so that ONE cost scalar comes back with no further
  // host synchronisation; a handle without priors launches nothing more and reduces the partials it always did
  int n_cost = plan.own.g_edge;
  if (pri_n > 0) {
    PGOC(prior_eval_enqueue(x, apply_loss, with_jac, part[5] + n_cost));
    n_cost += prior_grid();
  }
  // the flag rides along as a "partial array" of length 1 after conversion to double
  hipLaunchKernelGGL(dev::k_flag_to_double<>, dim3(1), dim3(1), 0, stream, bad, part[4]);
  return reduce_to_scal({{part[5], n_cost, 0}, {part[4], 1, 0}}, slot);
}

// k_prior_eval at x: the workgroups' cost partials into cost_part[0 .. prior_grid()), the `bad` flag, with_jac: the per-prior
// records k_prior_add reads; d_out / chi2_out (device, the caller's prior order): pgo_get_prior_residuals
int pgo_handle::prior_eval_enqueue(const double* x, int apply_loss, bool with_jac, double* cost_part, double* d_out, double* chi2_out) {
  dev::PriorArgs A;
  A.poses = x;
  A.row = pri_row_s.in(pri_tab.p);
  A.mean = pri_mean_s.in(pri_tab.p);
  A.info = pri_info_s.in(pri_tab.p);
  A.rec = pri_rec_s.in(pri_tab.p);
  A.n = pri_n;
  A.apply_loss = apply_loss;
  A.loss = pri_loss;
  A.order = pri_order_s.in(pri_tab.p);
  A.d_out = d_out;
  A.chi2_out = chi2_out;
  if (with_jac) hipLaunchKernelGGL(dev::k_prior_eval<true>, dim3(prior_grid()), dim3(dev::WG), 0, stream, A, cost_part, bad);
  else hipLaunchKernelGGL(dev::k_prior_eval<false>, dim3(prior_grid()), dim3(dev::WG), 0, stream, A, cost_part, bad);
  return check_launch("k_prior_eval");
}

// k_prior_add: the priors' blocks and gradients, with the current Jacobi scales, onto what k_assemble left in hd / gs
int pgo_handle::prior_add_enqueue() {
  dev::PriorAddArgs A;
  A.row = pri_row_s.in(pri_tab.p);
  A.rec = pri_rec_s.in(pri_tab.p);
  A.scale = scale;
  A.hd = hd;
  A.gs = gs;
  A.dense = pri_dense;
  A.n = pri_n;
  A.n_loc = S.n_loc;
  A.lo = S.lo;
  hipLaunchKernelGGL(dev::k_prior_add<>, dim3(launch_grid("prior_add_grid", ((int64_t)pri_n + dev::WG - 1) / dev::WG)), dim3(dev::WG), 0, stream, A);
  return check_launch("k_prior_add");
}

int pgo_handle::assemble_enqueue() {
  if (S.n_tiles() == 0) {
    if (pri_n == 0) return PGO_OK;
    // a graph without edges: k_assemble, which overwrites hd and gs, does not run -- k_prior_add adds to zeros
    HIPC(hipMemsetAsync(hd, 0, (size_t)6 * S.n_loc * sizeof(double), stream));
    HIPC(hipMemsetAsync(gs, 0, (size_t)3 * S.n_loc * sizeof(double), stream));
    return prior_add_enqueue();
  }
  if (has_sw) hipLaunchKernelGGL((dev::k_assemble<true, false>), dim3(plan.own.g_asm), dim3(dev::WG), 0, stream, asm_args());
  else if (info_mode) hipLaunchKernelGGL((dev::k_assemble<false, true>), dim3(plan.own.g_asm), dim3(dev::WG), 0, stream, asm_args());
  else hipLaunchKernelGGL((dev::k_assemble<false, false>), dim3(plan.own.g_asm), dim3(dev::WG), 0, stream, asm_args());
  PGOC(check_launch("k_assemble"));
  if (plan.all.chain_len && n_chain_dup > 0) {
    hipLaunchKernelGGL(dev::k_chain_dupfix<>, dim3((n_chain_dup + 63) / 64), dim3(64), 0, stream, (const int32_t*)chain_dup_rows, n_chain_dup,
                       (const int32_t*)inc_ptr, (const int32_t*)inc_col, (const double*)hoff, S.lo, chain_c);
    PGOC(check_launch("k_chain_dupfix"));
  }
  if (pri_n > 0) PGOC(prior_add_enqueue());   // (pose priors, pgo_set_priors: no launch without them)
  return PGO_OK;
}

int pgo_handle::spmv_enqueue(const double* p, double* yout, double* dot_part, int with_d2, const int32_t* done) {
  dev::SpmvArgs A = spmv_args(p, yout, dot_part, with_d2, done);
  if (plan.own.spmv_pipe && plan.own.spmv_one_tile && S.padded) hipLaunchKernelGGL(dev::k_spmv_1<true>, dim3(plan.own.g_spmv), dim3(dev::WG), 0, stream, A);
  else if (plan.own.spmv_pipe && plan.own.spmv_one_tile) hipLaunchKernelGGL(dev::k_spmv_1<false>, dim3(plan.own.g_spmv), dim3(dev::WG), 0, stream, A);
  else if (plan.own.spmv_pipe) hipLaunchKernelGGL(dev::k_spmv_p<>, dim3(plan.own.g_spmv), dim3(dev::WG), 0, stream, A);
  else hipLaunchKernelGGL(dev::k_spmv_t<0>, dim3(plan.own.g_spmv), dim3(dev::WG), 0, stream, A);
  return check_launch("k_spmv");
}

int pgo_handle::spmv_with_halo(double* full, double* yout, double* dot_part, const int32_t* done, int* n_part) {
  if (!plan.own.overlap) {
    PGOC(share_gather_vector(full));
    *n_part = plan.own.g_spmv;
    return spmv_enqueue(full, yout, dot_part, 1, done);
  }
  PGOC(pack_halo_rows(full));
  HIPC(hipEventRecord(ev_pack, stream));
  int used = 0;
  if (S.n_tiles() > 0) {  // enqueued before the exchange so that it also overlaps a host-blocking back-end
    dev::SpmvArgs A = spmv_args(full, yout, dot_part, 1, done);
    hipLaunchKernelGGL(dev::k_spmv_t<4>, dim3(plan.own.g_spmv_loc), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_spmv (owned columns)"));
    used += plan.own.g_spmv_loc;
  }
  HIPC(hipStreamWaitEvent(comm_stream, ev_pack, 0));
  PGOC(comm->exchange(halo_send_buf, halo_send_off3.data(), halo_recv_buf, halo_recv_off3.data(), comm_stream));
  PGOC(unpack_halo_rows(full, comm_stream));
  HIPC(hipEventRecord(ev_halo, comm_stream));
  HIPC(hipStreamWaitEvent(stream, ev_halo, 0));
  if (plan.own.n_rr > 0) {
    dev::RemoteArgs R;
    R.rows = rr_rows;
    R.ptr = rr_ptr;
    R.slots = rr_slots;
    R.inc_col = inc_col;
    R.hoff = hoff;
    R.p = full;
    R.y = yout;
    R.dot_part = dot_part + used;
    R.n_rows = plan.own.n_rr;
    R.lo = S.lo;
    R.done = done;
    hipLaunchKernelGGL(dev::k_spmv_remote<>, dim3(plan.own.g_rr), dim3(dev::WG), 0, stream, R);
    PGOC(check_launch("k_spmv_remote"));
    used += plan.own.g_rr;
  }
  *n_part = used;
  return PGO_OK;
}


// ---- the chain preconditioner's kernels: the (chain_chunk, chain_nw) instantiation the plan chose.  launch(chunk, waves) gets
// both as integral constants; the workgroup is 64 x waves threads.
template <class Launch>
static void chain_dispatch(const pgo::Plan& plan, Launch&& launch) {
  using std::integral_constant;
  if (plan.all.chain_chunk == 2 && plan.own.chain_nw == 4) launch(integral_constant<int, 2>(), integral_constant<int, 4>());
  else if (plan.all.chain_chunk == 2) launch(integral_constant<int, 2>(), integral_constant<int, 1>());
  else if (plan.own.chain_nw == 4) launch(integral_constant<int, 4>(), integral_constant<int, 4>());
  else launch(integral_constant<int, 4>(), integral_constant<int, 1>());
}

void pgo_handle::launch_cg_sr_chain(const dev::CgVec& V, double* part_gamma, double* part_rr) {
  const dev::ChainPre CP = chain_pre();
  chain_dispatch(plan, [&](auto chunk, auto waves) {
    hipLaunchKernelGGL((dev::k_cg_sr_cl<decltype(chunk)::value, decltype(waves)::value>), dim3(plan.own.g_chain), dim3(64 * decltype(waves)::value), 0, stream, V, CP,
                       sr_s, plan.all.chain_steps, plan.own.chain_scan, part_gamma, part_rr);
  });
}

void pgo_handle::launch_cg_update1_chain(const dev::CgVec& V, int par, const double* pap, int n_pap, double* part_rz, double* part_rr) {
  const dev::ChainPre CP = chain_pre();
  chain_dispatch(plan, [&](auto chunk, auto waves) {
    hipLaunchKernelGGL((dev::k_cg_update1_cl<decltype(chunk)::value, decltype(waves)::value>), dim3(plan.own.g_chain), dim3(64 * decltype(waves)::value), 0, stream, V,
                       CP, plan.all.chain_steps, plan.own.chain_scan, par, pap, n_pap, part_rz, part_rr);
  });
}

// ---- z = M^-1 b: the lines the LM loop's PCG, the covariance columns and the debug / bench hooks all run
int pgo_handle::launch_cg_init(const double* b, double* z_out, double* part_rz, double* part_bb) {
  const dev::CgVec V = cg_vec(z_out);
  if (plan.all.chain_len > 0) {
    const dev::ChainPre CP = chain_pre();
    chain_dispatch(plan, [&](auto chunk, auto waves) {
      hipLaunchKernelGGL((dev::k_cg_init_cl<decltype(chunk)::value, decltype(waves)::value>), dim3(plan.own.g_chain), dim3(64 * decltype(waves)::value), 0, stream, V,
                         CP, plan.all.chain_steps, plan.own.chain_scan, b, part_rz, part_bb);
    });
  } else if (plan.own.grp_B > 1) {
    hipLaunchKernelGGL(dev::k_cg_init_g<>, dim3(plan.own.g_grp), dim3(dev::WG), 0, stream, V, group_pre(), b, part_rz, part_bb);
  } else {
    hipLaunchKernelGGL(dev::k_cg_init<>, dim3(plan.own.g_vec), dim3(dev::WG), 0, stream, V, b, part_rz, part_bb);
  }
  return check_launch("k_cg_init");
}

int pgo_handle::launch_coarse_prolong(double* z_inout, double* p_or_null) {
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((S.n_loc + 255) / 256, 512)));   // (at least one workgroup: a rank may own no rows)
  if (co_multi()) {   // global aggregates and basis planes; the kernel finds the owned rows of p itself
    hipLaunchKernelGGL(dev::k_coarse_prolong_m<>, grid, dim3(256), 0, stream, (int)S.n_loc, (int)S.lo, CO().co_agg, (const double*)co_pb, (int64_t)S.n_poses,
                       (const double*)co_ec, z_inout, p_or_null, (const int32_t*)co_ok);
    return check_launch("k_coarse_prolong_m");
  }
  hipLaunchKernelGGL(dev::k_coarse_prolong<>, grid, dim3(256), 0, stream, (int)S.n_loc, CO().co_agg, (const double*)co_pb, (const double*)co_ec, z_inout,
                     p_or_null ? p_or_null + dev::PS * (int64_t)S.lo : (double*)nullptr, (const int32_t*)co_ok);
  return check_launch("k_coarse_prolong");
}

int pgo_handle::precondition(const double* b, double* z_out, double* p_or_null, double* dot_part) {
  PGOC(launch_cg_init(b, z_out, part[0], part[1]));
  if (!coarse_on()) return PGO_OK;
  if (co_multi()) PGOC(coarse_restrict_reduce(part[0], cg_init_parts(), part[1], cg_init_parts(), nullptr));
  PGOC(coarse_solve(dot_part, nullptr));
  return launch_coarse_prolong(z_out ? z_out : z, p_or_null);
}

// ---- launches several units need
// (a batched handle's fixed_internal is -1, pgo_batch_create: fixed_mask carries one anchor per problem and the padding rows)
int pgo_handle::launch_jacobi_scale(int pass) {
  hipLaunchKernelGGL(dev::k_jacobi_scale<>, dim3(plan.own.g_rows), dim3(dev::WG), 0, stream, hd, S.n_loc, S.lo, fixed_internal, pass, scale, (const uint8_t*)fixed_mask);
  return check_launch("k_jacobi_scale");
}

int pgo_handle::scatter_owned(const double* src) {
  hipLaunchKernelGGL(dev::k_scatter_owned<>, dim3(plan.own.g_flat), dim3(dev::WG), 0, stream, (int)S.n_loc, (int)S.lo, src, p_full);
  return check_launch("k_scatter_owned");
}

int pgo_handle::switch_prepare(double radius) {
  hipLaunchKernelGGL(dev::k_switch_prepare<>, dim3(g_sw()), dim3(dev::WG), 0, stream, switch_arrays(), (const double*)jr, radius, opt.min_lm_diagonal,
                     opt.max_lm_diagonal, part[2], part[3]);
  return check_launch("k_switch_prepare");
}

// ---- caller's numbering <-> internal numbering
int pgo_handle::upload_pose_vector(double* dst, const double* caller_src, int64_t row0, int64_t rows) {
  if (rows < 0) rows = S.n_poses - row0;
  if (rows == 0) return PGO_OK;
  std::vector<double> staged;
  const double* src = caller_src + 3 * row0;
  if (!perm.empty()) {
    staged.resize((size_t)3 * rows);
    for (int64_t i = 0; i < S.n_poses; ++i) {
      const int64_t k = perm[i] - row0;
      if (k >= 0 && k < rows) memcpy(&staged[(size_t)3 * k], caller_src + 3 * i, 3 * sizeof(double));
    }
    src = staged.data();
  }
  HIPC(hipMemcpyAsync(dst, src, (size_t)3 * rows * sizeof(double), hipMemcpyHostToDevice, stream));
  return sync();   // `staged` dies with this scope
}

int pgo_handle::download_pose_vector(double* caller_dst, const double* src, int64_t row0, int64_t rows) {
  const int64_t N = S.n_poses;
  if (rows < 0) rows = N - row0;
  if (perm.empty()) {
    if (rows < N) memset(caller_dst, 0, (size_t)3 * N * sizeof(double));
    if (rows > 0) HIPC(hipMemcpyAsync(caller_dst + 3 * row0, src, (size_t)3 * rows * sizeof(double), hipMemcpyDeviceToHost, stream));
    return sync();
  }
  std::vector<double> staged((size_t)3 * rows);
  if (rows > 0) HIPC(hipMemcpyAsync(staged.data(), src, staged.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  PGOC(sync());
  for (int64_t i = 0; i < N; ++i) {
    const int64_t k = perm[i] - row0;
    if (k >= 0 && k < rows) memcpy(caller_dst + 3 * i, &staged[(size_t)3 * k], 3 * sizeof(double));
    else memset(caller_dst + 3 * i, 0, 3 * sizeof(double));
  }
  return PGO_OK;
}
