// The linear solve of an LM iteration by preconditioned CG on the Jacobi-scaled normal equations (north_star: "block-Jacobi-
// preconditioned CG whose SpMV is a CDNA4 HIP kernel"): the PCG loops (textbook, fused direction update for small graphs,
// single reduction for several ranks), the preconditioners' per-iteration set-up, the coarse level's factorisation and apply.
#include "solver_handle.hip.h"

int pgo_handle::coarse_factor() {
  dev::CoarseArgs A;
  A.n_loc = S.n_loc;
  A.agg = CO().co_agg;
  A.n_agg = CO().co_nagg;
  A.K = CO().co_K;
  A.Kp = CO().co_Kp;
  A.poses = poses;
  A.scale = scale;
  A.pb = co_pb;
  A.hoff = hoff;
  A.hd = hd;
  A.d2 = d2;
  A.inc_col = inc_col;
  A.cb_i = co_cb_i;
  A.cb_j = co_cb_j;
  A.cb_ptr = co_cb_ptr;
  A.cb_q = co_cb_q;
  A.cb_row = co_cb_row;
  A.n_cb = co_ncb;
  A.cap = co_cap;
  A.dwork = co_dwork;
  if (co_multi()) PGOC(coarse_assemble_multi());
  else {
    hipLaunchKernelGGL(dev::k_coarse_basis<>, dim3((CO().co_nagg + 3) / 4), dim3(256), 0, stream, A);
    PGOC(check_launch("k_coarse_basis"));
    HIPC(hipMemsetAsync(co_cap, 0, (size_t)CO().co_Kp * CO().co_Kp * sizeof(double), stream));
    HIPC(hipMemsetAsync(co_dwork, 0, (size_t)(CO().co_Kp / 32) * 1024 * sizeof(double), stream));
    hipLaunchKernelGGL(dev::k_coarse_assemble<>, dim3((co_ncb + 3) / 4), dim3(256), 0, stream, A);
    PGOC(check_launch("k_coarse_assemble"));
  }
  if (CO().co_Kp > CO().co_K) {
    hipLaunchKernelGGL(dev::k_coarse_pad<>, dim3(1), dim3(32), 0, stream, co_cap, co_dwork, CO().co_K, CO().co_Kp);
    PGOC(check_launch("k_coarse_pad"));
  }
  if (co_ndead > 0) {
    hipLaunchKernelGGL(dev::k_coarse_dead<>, dim3((3 * co_ndead + 255) / 256), dim3(256), 0, stream, co_cap, co_dwork, (const int32_t*)co_dead,
                       co_ndead, CO().co_Kp);
    PGOC(check_launch("k_coarse_dead"));
  }
  const int nb = CO().co_Kp / 32;
  for (int kb = 0; kb < nb; ++kb) {
    hipLaunchKernelGGL(dev::k_chol_panel<>, dim3(std::max(1, nb - 1)), dim3(dev::CHOL_THREADS), dev::CHOL_LDS_BYTES, stream, co_cap, co_nm, co_dwork, CO().co_Kp, nb, kb);
    PGOC(check_launch("k_chol_panel (coarse level)"));
  }
  // usable?  a probe through the factor: x = A_c^-1 1 must be finite (a pivot lost to rounding leaves NaNs behind it)
  hipLaunchKernelGGL(dev::k_fill<>, dim3((CO().co_Kp + 255) / 256), dim3(256), 0, stream, co_rc, (int64_t)CO().co_Kp, 1.0);
  if (co_ainv) {
    hipLaunchKernelGGL(dev::k_coarse_ainv<>, dim3((CO().co_Kp + 255) / 256, CO().co_Kp), dim3(256), 0, stream, (const double*)co_nm, CO().co_Kp, co_ainv);
    hipLaunchKernelGGL(dev::k_tri_apply<>, dim3(nb), dim3(256), 0, stream, (const double*)co_ainv, CO().co_Kp, nb, (const double*)co_rc, co_ec, 0);
  } else {
    hipLaunchKernelGGL(dev::k_tri_apply<>, dim3(nb), dim3(256), 0, stream, (const double*)co_nm, CO().co_Kp, nb, (const double*)co_rc, co_cy, 0);
    hipLaunchKernelGGL(dev::k_tri_apply<>, dim3(nb), dim3(256), 0, stream, (const double*)co_nm, CO().co_Kp, nb, (const double*)co_cy, co_ec, 1);
  }
  hipLaunchKernelGGL(dev::k_coarse_check<>, dim3(1), dim3(256), 0, stream, (const double*)co_ec, CO().co_Kp, co_ok);
  // (the restriction writes the K coarse unknowns only: the padding entries K .. Kp-1 of r_c must read 0 again)
  hipLaunchKernelGGL(dev::k_fill<>, dim3((CO().co_Kp + 255) / 256), dim3(256), 0, stream, co_rc, (int64_t)CO().co_Kp, 0.0);
  return check_launch("coarse level probe");
}

// several ranks: basis planes of every pose, this rank's Galerkin blocks, all-gather, scatter into the dense matrix (which,
// with its factorisation, is then the same on every rank)
int pgo_handle::coarse_assemble_multi() {
  dev::CoarseMArgs M;
  M.n = S.n_poses;
  M.lo = S.lo;
  M.n_loc = S.n_loc;
  M.agg = CO().co_agg;
  M.n_agg = CO().co_nagg;
  M.poses = poses;
  M.scale = scale;
  M.live = co_live;
  M.pb = co_pb;
  M.hoff = hoff;
  M.hd = hd;
  M.d2 = d2;
  M.inc_col = inc_col;
  M.cb_i = co_cb_i;
  M.cb_j = co_cb_j;
  M.cb_ptr = co_cb_ptr;
  M.cb_q = co_cb_q;
  M.cb_row = co_cb_row;
  M.n_cb = co_ncb;
  M.vals = co_gvals + (int64_t)comm->rank * co_ncb_max * 9;
  hipLaunchKernelGGL(dev::k_coarse_basis_m<>, dim3((CO().co_nagg + 3) / 4), dim3(256), 0, stream, M);
  PGOC(check_launch("k_coarse_basis_m"));
  HIPC(hipMemsetAsync(co_cap, 0, (size_t)CO().co_Kp * CO().co_Kp * sizeof(double), stream));
  HIPC(hipMemsetAsync(co_dwork, 0, (size_t)(CO().co_Kp / 32) * 1024 * sizeof(double), stream));
  if (co_ncb > 0) {
    hipLaunchKernelGGL(dev::k_coarse_assemble_m<>, dim3((co_ncb + 3) / 4), dim3(256), 0, stream, M);
    PGOC(check_launch("k_coarse_assemble_m"));
  }
  if (comm->allgather_inplace(co_gvals, (int64_t)9 * co_ncb_max, stream) != 0)
    return fail(PGO_ERR_COMM, "coarse level: all-gather of the Galerkin blocks failed");
  const int64_t nblk = (int64_t)comm->world * co_ncb_max;
  if (nblk > 0) {
    hipLaunchKernelGGL(dev::k_coarse_scatter<>, dim3((unsigned)((9 * nblk + 255) / 256)), dim3(256), 0, stream, (const double*)co_gvals,
                       (const int32_t*)co_gi, (const int32_t*)co_gj, nblk, co_cap, co_dwork, CO().co_Kp);
    PGOC(check_launch("k_coarse_scatter"));
  }
  return PGO_OK;
}

// several ranks: r_c = P'r of the own aggregates into the zeroed global vector, and the partial sums of r.z and r.r next to it,
// all in ONE all-reduce -- afterwards every rank holds the whole r_c and the reduced (r.z, r.r) at co_red + Kp
int pgo_handle::coarse_restrict_reduce(const double* rz_part, int n_rz, const double* rr_part, int n_rr, const int32_t* done) {
  const int slots = (CO().co_Kp + 2) / 3;
  hipLaunchKernelGGL(dev::k_coarse_restrict_m<>, dim3((slots + 3) / 4), dim3(256), 0, stream, (int)S.n_loc, (int)S.lo, CO().co_agg, CO().co_aoff, CO().co_nown,
                     CO().co_Kp, (const double*)co_pb, (int64_t)S.n_poses, (const double*)r, co_red, done);
  PGOC(check_launch("k_coarse_restrict_m"));
  return reduce_parts({{rz_part, n_rz, 0}, {rr_part, n_rr, 0}}, co_red + CO().co_Kp, co_red, CO().co_Kp + 2, false);
}

int pgo_handle::coarse_solve(double* dot_part, const int32_t* done) {
  const int nb = CO().co_Kp / 32;
  if (!co_multi())   // (several ranks: r_c came with the all-reduce, coarse_restrict_reduce)
    hipLaunchKernelGGL(dev::k_coarse_restrict<>, dim3((CO().co_nagg + 3) / 4), dim3(256), 0, stream, (int)S.n_loc, CO().co_agg, CO().co_nagg, (const double*)co_pb,
                       (const double*)r, co_rc, done);
  if (co_ainv) {
    hipLaunchKernelGGL(dev::k_coarse_matvec<>, dim3(CO().co_ndot), dim3(256), 0, stream, (const double*)co_ainv, CO().co_Kp, (const double*)co_rc, co_ec,
                       dot_part, (const int32_t*)co_ok, done);
  } else {
    hipLaunchKernelGGL(dev::k_tri_apply<>, dim3(nb), dim3(256), 0, stream, (const double*)co_nm, CO().co_Kp, nb, (const double*)co_rc, co_cy, 0);
    hipLaunchKernelGGL(dev::k_tri_apply<>, dim3(nb), dim3(256), 0, stream, (const double*)co_nm, CO().co_Kp, nb, (const double*)co_cy, co_ec, 1);
    hipLaunchKernelGGL(dev::k_coarse_dot<>, dim3(CO().co_ndot), dim3(256), 0, stream, CO().co_Kp, (const double*)co_rc, co_ec, dot_part,
                       (const int32_t*)co_ok, done);
  }
  return check_launch("coarse level solve");
}

// block-Jacobi PCG on (H + D2) y = gs, y0 = 0.  Host checks the residual every
// pcg_check_every iterations; in between the kernels early-out on st->done.
int pgo_handle::pcg(int* iters, double* rel) {
  dev::CgVec V = cg_vec();
  const bool multi = multi_rank();
  const dev::GroupPre GP = group_pre();
  const bool grouped = plan.own.grp_B > 1, chained = plan.all.chain_len > 0;
  const int g_u1 = cg_init_parts();  // grid (= number of partials) of the init / update1 kernels
  const bool sr = plan.all.use_sr && chained;
  // single-reduction loop: "make u visible to the peers, w = A u, reduce (gamma, rr, delta) together, new coefficients"
  auto sr_product_and_scalars = [&](int first) -> int {
    int n_sp = plan.own.g_spmv;
    const int32_t* done = first ? nullptr : &st->done;
    if (plan.own.overlap) PGOC(spmv_with_halo(p_full, ap, part[2], done, &n_sp));
    else {
      PGOC(share_gather_vector(p_full));
      PGOC(spmv_enqueue(p_full, ap, part[2], 1, done));
    }
    PGOC(reduce_to_scal({{part[0], g_u1, 0}, {part[1], g_u1, 0}, {part[2], n_sp, 0}}, 4));
    hipLaunchKernelGGL(dev::k_cg_sr_scal<>, dim3(1), dim3(1), 0, stream, st, (const double*)(scal + 4), opt.pcg_rtol, first);
    return check_launch("k_cg_sr_scal");
  };
  // z = M^-1 b.  One rank: both levels in one call.  Several ranks with the coarse level run the pieces of precondition() below:
  // r_c rides in the all-reduce of the start-up sums and the coarse share is added to the reduced r.z once (k_coarse_fin).
  // (The single-reduction loop has no second level.)
  const bool two_level_multi = coarse_on() && co_multi();
  if (sr || two_level_multi) PGOC(launch_cg_init(gs, nullptr, part[0], part[1]));
  else PGOC(precondition(gs, nullptr, p_full, part[0] + g_u1));
  if (sr) {
    // the start-up kernel left u = M^-1 b in the gather vector (and in z, which becomes p: beta = 0 in the first update)
    HIPC(hipMemsetAsync(sr_s, 0, (size_t)3 * S.n_loc * sizeof(double), stream));
    PGOC(sr_product_and_scalars(1));
  } else {
    // two levels: z (= p) of the start-up kernel got the coarse correction, r.z one more partial
    const int n_rz0 = coarse_on() ? g_u1 + CO().co_ndot : g_u1;
    if (two_level_multi) {
      PGOC(coarse_restrict_reduce(part[0], g_u1, part[1], g_u1, nullptr));
      PGOC(coarse_solve(co_dotp, nullptr));
      hipLaunchKernelGGL(dev::k_coarse_fin<>, dim3(1), dim3(dev::WG), 0, stream, (const double*)(co_red + CO().co_Kp), (const double*)co_dotp, CO().co_ndot,
                         scal + 4);
      PGOC(check_launch("k_coarse_fin"));
      PGOC(launch_coarse_prolong(z, p_full));
    }
    if (coarse_on()) {
      // whether this solve has the level: read back with the model terms (lm_iteration_tail), counted in co_off_iters
      hipLaunchKernelGGL(dev::k_flag_to_double<>, dim3(1), dim3(1), 0, stream, (const int*)co_ok, scal + 15);
      PGOC(check_launch("k_flag_to_double"));
      co_flag_pending = true;
    }
    if (!two_level_multi) PGOC(reduce_to_scal({{part[0], n_rz0, 0}, {part[1], g_u1, 0}}, 4));
    hipLaunchKernelGGL(dev::k_cg_init_fin<>, dim3(1), dim3(1), 0, stream, st, scal + 4, opt.pcg_rtol);
    PGOC(check_launch("k_cg_init_fin"));
    if (!plan.own.overlap) PGOC(share_gather_vector(p_full));
  }
  const int max_it = std::max(0, opt.pcg_max_iters);
  int every = std::max(1, opt.pcg_check_every);
  // one PCG iteration = 3 dependent launches; `par` is the r.z double-buffer parity baked into the arguments
  const bool fused = plan.all.fused_p && !multi;
  double* pbuf[2] = {p_full, p_full2};
  if (fused) HIPC(hipMemsetAsync(p_full2, 0, (size_t)dev::PS * n_full * sizeof(double), stream));  // "p_old" of iteration 0
  auto enqueue_iteration = [&](int par) -> int {
    if (sr) {
      launch_cg_sr_chain(V, part[0], part[1]);
      PGOC(check_launch("k_cg_sr_cl"));
      return sr_product_and_scalars(0);
    }
    int n_sp = plan.own.g_spmv;
    dev::CgVec Vi = V;
    if (fused) {
      // the previous iteration's direction update happens inside this SpMV: p_old = pbuf[par ^ 1] -> p_new = pbuf[par]
      dev::SpmvArgs A = spmv_args(pbuf[par ^ 1], ap, part[0], 1, &st->done);
      A.z = z;
      A.p_new = pbuf[par];
      A.part_rz = part[1];
      A.part_rr = part[2];
      A.n_rz = A.n_rr = g_u1;
      A.parity = par ^ 1;
      A.st = st;
      hipLaunchKernelGGL(dev::k_spmv_t<5>, dim3(plan.own.g_spmv), dim3(dev::WG), 0, stream, A);
      PGOC(check_launch("k_spmv (fused direction update)"));
      Vi.p = pbuf[par];
      Vi.fused = 1;
    } else if (plan.own.overlap) PGOC(spmv_with_halo(p_full, ap, part[0], &st->done, &n_sp));  // p reaches the peers inside
    else PGOC(spmv_enqueue(p_full, ap, part[0], 1, &st->done));
    // p.Ap: every workgroup of the update kernel re-sums the product's partials itself -- up to 2048 of them; more (k_spmv_1:
    // one per tile) are folded to 16 first (k_fold_partials); several ranks: k_finalize + all-reduce
    const bool fold_pap = !multi && n_sp > 2048;
    const double* pap = multi ? scal + 6 : (fold_pap ? part[3] : part[0]);
    const int n_pap = multi ? 1 : (fold_pap ? 16 : n_sp);
    if (multi) PGOC(reduce_to_scal({{part[0], n_sp, 0}}, 6));
    else if (fold_pap) {
      hipLaunchKernelGGL(dev::k_fold_partials<>, dim3(16), dim3(dev::WG), 0, stream, (const double*)part[0], n_sp, part[3], (const int32_t*)&st->done);
      PGOC(check_launch("k_fold_partials"));
    }
    if (chained) launch_cg_update1_chain(Vi, par, pap, n_pap, part[1], part[2]);
    else if (grouped) hipLaunchKernelGGL(dev::k_cg_update1_g<>, dim3(g_u1), dim3(dev::WG), 0, stream, Vi, GP, par, pap, n_pap, part[1], part[2]);
    else hipLaunchKernelGGL(dev::k_cg_update1<>, dim3(g_u1), dim3(dev::WG), 0, stream, Vi, par, pap, n_pap, part[1], part[2]);
    PGOC(check_launch("k_cg_update1"));
    if (fused) return PGO_OK;  // its r.z / r.r partials are booked by the next SpMV, or by k_cg_book at the end of the slice
    if (coarse_on() && co_multi()) {   // second level, several ranks: r_c in the all-reduce of (r.z, r.r), replicated coarse solve
      PGOC(coarse_restrict_reduce(part[1], g_u1, part[2], g_u1, &st->done));
      PGOC(coarse_solve(co_dotp, &st->done));
      hipLaunchKernelGGL(dev::k_cg_update2cm<>, dim3(plan.own.g_vec), dim3(dev::WG), 0, stream, V, par, (const double*)(co_red + CO().co_Kp), (const double*)co_dotp,
                         CO().co_ndot, CO().co_agg, (const double*)co_pb, (int64_t)S.n_poses, (const double*)co_ec);
      PGOC(check_launch("k_cg_update2cm"));
      if (!plan.own.overlap) PGOC(share_gather_vector(p_full));
      return PGO_OK;
    }
    if (coarse_on()) {   // second level (single rank): e_c, its share of r.z as more partials, prolongation inside the direction update
      PGOC(coarse_solve(part[1] + g_u1, &st->done));
      hipLaunchKernelGGL(dev::k_cg_update2c<>, dim3(plan.own.g_vec), dim3(dev::WG), 0, stream, V, par, (const double*)part[1], g_u1 + CO().co_ndot,
                         (const double*)part[2], g_u1, CO().co_agg, (const double*)co_pb, (const double*)co_ec);
      return check_launch("k_cg_update2c");
    }
    if (multi) {
      PGOC(reduce_to_scal({{part[1], g_u1, 0}, {part[2], g_u1, 0}}, 7));
      hipLaunchKernelGGL(dev::k_cg_update2<>, dim3(plan.own.g_flat), dim3(dev::WG), 0, stream, V, par, scal + 7, 1, scal + 8, 1);
      PGOC(check_launch("k_cg_update2"));
      if (!plan.own.overlap) PGOC(share_gather_vector(p_full));
    } else {
      hipLaunchKernelGGL(dev::k_cg_update2<>, dim3(plan.own.g_flat), dim3(dev::WG), 0, stream, V, par, part[1], g_u1, part[2], g_u1);
      PGOC(check_launch("k_cg_update2"));
    }
    return PGO_OK;
  };
  // Launch-bound regime (small graphs): a slice of `every` iterations is captured ONCE per handle into a
  // hipGraph (every argument is fixed for the handle's lifetime; the slice length is even so the parity
  // pattern repeats) and replayed with a single host call per slice.
  // Several ranks: the slice is captured WITH its RCCL calls (all-reduces of the dot products, halo exchange or
  // all-gather of the search direction) when they are pure stream work and everything runs on the one solver stream
  // -- otherwise every PCG iteration costs the host ~7 kernel launches + 3 collective calls, about the device time of
  // an iteration at 8 shards of the 1M-pose graph.  PGO_GRAPH_COLLECTIVES=0 keeps the eager loop; a capture that fails
  // falls back to it for the rest of the handle's life.
  // The point-to-point halo exchange (an ncclSend / ncclRecv group) is NOT captured by default: it has never run against
  // a real peer (no multi-GPU lease yet), and a group of p2p calls inside a graph is the less travelled road -- its
  // first execution should be the plain one.  PGO_GRAPH_COLLECTIVES=2 captures it too.
  bool use_graph = opt.use_graphs && !graph_failed &&
                   (!multi || (comm->capturable() && !plan.own.overlap && graph_collectives > 0 && (!plan.all.use_halo || graph_collectives > 1)));
  if (use_graph) {
    every += every & 1;
    if (!cg_graph_exec || cg_graph_len != every) {
      if (cg_graph_exec) (void)hipGraphExecDestroy(cg_graph_exec);
      cg_graph_exec = nullptr;
      hipGraph_t gr = nullptr;
      HIPC(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
      int st_cap = PGO_OK;
      for (int c = 0; c < every && st_cap == PGO_OK; ++c) st_cap = enqueue_iteration(c & 1);
      if (fused && st_cap == PGO_OK) {
        hipLaunchKernelGGL(dev::k_cg_book<>, dim3(1), dim3(dev::WG), 0, stream, st, (every - 1) & 1, (const double*)part[1], g_u1, (const double*)part[2], g_u1);
        st_cap = check_launch("k_cg_book");
      }
      hipError_t e_end = hipStreamEndCapture(stream, &gr);
      hipError_t e_inst = hipSuccess;
      if (st_cap == PGO_OK && e_end == hipSuccess) {
        e_inst = hipGraphInstantiate(&cg_graph_exec, gr, nullptr, nullptr, 0);
        (void)hipGraphDestroy(gr);
      }
      if (st_cap != PGO_OK || e_end != hipSuccess || e_inst != hipSuccess) {
        if (!multi) {  // single rank: a capture failure is a real error
          PGOC(st_cap);
          if (e_end != hipSuccess) return fail(PGO_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e_end));
          return fail(PGO_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e_inst));
        }
        // with collectives inside: run eagerly from now on (every rank takes the same decision: same library, same calls)
        (void)hipGetLastError();
        cg_graph_exec = nullptr;
        graph_failed = true;
        use_graph = false;
        if (opt.verbose) printf("pgo: hipGraph capture of the PCG slice with collectives failed; eager launches from here on\n");
      } else {
        cg_graph_len = every;
      }
    }
  }
  // Slices enqueued after convergence are not free: each of their launches early-outs on st->done but still costs
  // ~4.5 us of device time (13 us per no-op PCG iteration at 1M poses -- with 100-iteration slices that was 5 % of an LM
  // iteration).  So the slices are short and the FIRST host check comes after as many of them as the previous solve of
  // this handle makes likely (85 % of its iteration count; consecutive LM iterations need similar counts), the
  // following checks after every slice.
  int it = 0;
  int ahead = (last_pcg_iters > 0) ? std::max(1, (int)(0.85 * last_pcg_iters) / every) : 1;
  while (true) {
    const double te0 = wall_s();
    const int it_before = it;
    for (int sl = 0; sl < ahead && it < max_it; ++sl) {
      const int chunk = std::min(every, max_it - it);
      if (use_graph && chunk == every && (it & 1) == 0) {
        HIPC(hipGraphLaunch(cg_graph_exec, stream));
      } else {
        for (int c = 0; c < chunk; ++c) PGOC(enqueue_iteration((it + c) & 1));
        if (fused && chunk > 0) {
          hipLaunchKernelGGL(dev::k_cg_book<>, dim3(1), dim3(dev::WG), 0, stream, st, (it + chunk - 1) & 1, (const double*)part[1], g_u1, (const double*)part[2], g_u1);
          PGOC(check_launch("k_cg_book"));
        }
      }
      it += chunk;
    }
    ahead = 1;
    t_enqueue += wall_s() - te0;
    n_enqueued += it - it_before;
    HIPC(hipMemcpyAsync(h_st, st, sizeof(dev::CgState), hipMemcpyDeviceToHost, stream));
    PGOC(sync());
    if (h_st->done || it >= max_it) break;
  }
  last_pcg_iters = h_st->iters;
  *iters = h_st->iters;
  *rel = (h_st->bb > 0.0) ? std::sqrt(h_st->rr / h_st->bb) : 0.0;
  if (plan.all.verify_residual) {
    // test hook: report |b - A y| / |b| of the solution instead of the recurrence residual the loop stopped on (one more
    // product; the recurrences of either loop drift from it on ill-conditioned systems)
    PGOC(scatter_owned(y));
    PGOC(share_gather_vector(p_full));
    PGOC(spmv_enqueue(p_full, ap, part[0], 1, nullptr));
    hipLaunchKernelGGL(dev::k_residual_norm<>, dim3(plan.own.g_flat), dim3(dev::WG), 0, stream, (int64_t)3 * S.n_loc, (const double*)gs, (const double*)ap, part[1], part[2]);
    PGOC(check_launch("k_residual_norm"));
    PGOC(reduce_to_scal({{part[1], plan.own.g_flat, 0}, {part[2], plan.own.g_flat, 0}}, 4));
    double h2[2] = {0.0, 0.0};
    HIPC(hipMemcpyAsync(h2, scal + 4, sizeof h2, hipMemcpyDeviceToHost, stream));
    PGOC(sync());
    *rel = (h2[1] > 0.0) ? std::sqrt(h2[0] / h2[1]) : 0.0;
  }
  return PGO_OK;
}

// the PCG preconditioner for the current LM diagonal: dense pose-group inverses or the chain factorisation
int pgo_handle::prepare_preconditioner() {
  if (plan.own.grp_B > 1) {
    dev::GroupPrepArgs GA;
    GA.inc_ptr = inc_ptr;
    GA.inc_col = inc_col;
    GA.hoff = hoff;
    GA.hd = hd;
    GA.d2 = d2;
    GA.ginv = ginv;
    GA.n_loc = S.n_loc;
    GA.lo = S.lo;
    GA.B = plan.own.grp_B;
    GA.nb = plan.own.grp_nb;
    GA.n_groups = plan.own.n_groups;
    hipLaunchKernelGGL(dev::k_prepare_groups<>, dim3(plan.own.grp_prep_grid), dim3(dev::WG), plan.own.grp_lds, stream, GA);
    PGOC(check_launch("k_prepare_groups"));
  }
  if (plan.all.chain_len) PGOC(factor_chain());
  if (coarse_on()) PGOC(coarse_factor());
  return PGO_OK;
}

// block LDL' of the chain preconditioner's segments (the records are complete: C part from k_assemble, M part from k_prepare)
int pgo_handle::factor_chain() {
  const int n_seg = (S.n_loc + plan.all.chain_len - 1) / plan.all.chain_len;
  // One THREAD per segment runs the recurrence (64 .. 256 dependent steps), 64 segments per wavefront: 244 wavefronts at 1M
  // poses.  Fewer segments per wavefront (16: four wavefronts per compute unit, each with its own queue of outstanding loads)
  // were measured SLOWER -- 233 us against 123 us: the same 128-byte-per-lane record loads then take four times as many
  // wave instructions through the address coalescer, and 174 instead of 122 MB are written.
  const int spw = 64;
  if (n_seg == 0) return PGO_OK;   // a rank that owns no rows
  if (plan.all.chain_chunk == 2)
    hipLaunchKernelGGL(dev::k_chain_factor<2>, dim3((n_seg + spw - 1) / spw), dim3(spw), 0, stream, (const double*)chain_c, S.n_loc, plan.own.chain_pad,
                       plan.all.chain_len, chain_w, chain_s);
  else
    hipLaunchKernelGGL(dev::k_chain_factor<4>, dim3((n_seg + spw - 1) / spw), dim3(spw), 0, stream, (const double*)chain_c, S.n_loc, plan.own.chain_pad,
                       plan.all.chain_len, chain_w, chain_s);
  return check_launch("k_chain_factor");
}

// LM diagonal for `radius` (per problem in a batched handle) + the preconditioner's set-up
int pgo_handle::prepare_system(double radius, bool preconditioner_also_on_direct) {
  hipLaunchKernelGGL(dev::k_prepare<>, dim3(plan.own.g_rows), dim3(dev::WG), 0, stream, hd, (const double*)diag_full, S.n_loc, S.lo, fixed_internal, radius,
                     opt.min_lm_diagonal, opt.max_lm_diagonal, d2, minv, (const uint8_t*)fixed_mask, (const int32_t*)prob_of_256,
                     (const double*)prob_radius, plan.all.chain_len ? chain_c : (double*)nullptr, hdd);
  PGOC(check_launch("k_prepare"));
  // (the direct solve does not need the preconditioner; its PCG fallback sets it up on demand)
  if (!direct() || preconditioner_also_on_direct) PGOC(prepare_preconditioner());
  return PGO_OK;
}
