// pgo_handle::create -- replaces the problem assembly of DCS-ceres/main.cpp:66-68,95-153: shard structure (structure.cpp) ->
// the plan (plan.h: every choice made once per handle, from facts gathered here) -> device buffers, uploads and kernel
// attributes as the plan sizes them (direct_build, coarse_build).  No decision is taken in this file.

#include "solver_handle.hip.h"

// --------------------------------------------------------------------- create
int pgo_handle::create(int32_t N, const double* poses_h, int32_t E, const int32_t* ia, const int32_t* ib,
                       const double* meas, const double* info6, const uint8_t* kind) {
  const int world = comm ? comm->world : 1, rank = comm ? comm->rank : 0;
  n_edges_total = E;
  info_mode = opt.info_weighting != 0;
  if (info_mode) {
    if (!info6) return fail(PGO_ERR_INVALID_ARG, "info_weighting = 1 needs the information matrices (pgo_create_weighted / pgo_create_from_graph)");
    if (opt.method == 2) return fail(PGO_ERR_UNSUPPORTED, "info_weighting is implemented for METHOD 0 and 1 only");
    for (int32_t e = 0; e < E; ++e) {  // every Omega must have a Cholesky factor
      const double* w = info6 + 6 * (size_t)e;
      const double l00 = w[0] > 0.0 ? std::sqrt(w[0]) : 0.0;
      const double l10 = l00 > 0.0 ? w[1] / l00 : 0.0, l20 = l00 > 0.0 ? w[2] / l00 : 0.0;
      const double d1 = w[3] - l10 * l10;
      const double l11 = d1 > 0.0 ? std::sqrt(d1) : 0.0;
      const double l21 = l11 > 0.0 ? (w[4] - l20 * l10) / l11 : 0.0;
      const double d2v = w[5] - l20 * l20 - l21 * l21;
      if (!(w[0] > 0.0) || !(d1 > 0.0) || !(d2v > 0.0) || !std::isfinite(d2v))
        return fail(PGO_ERR_NUMERIC, "info_weighting: the information matrix of edge " + std::to_string(e) +
                                         " is not positive definite (EDGE2 files are read positionally like EDGE_SE2, "
                                         "reference g2o_util.h:53-66)");
    }
    rec_doubles = dev::REC_INFO;
  }
  const char* fc = getenv("PGO_FORCE_COLLECTIVES");
  force_collectives = fc && fc[0] == '1';
  if (const char* gc = getenv("PGO_GRAPH_COLLECTIVES")) graph_collectives = atoi(gc);
  pgo::PlanEnv env;
  env.world = world;
  env.rank = rank;
  env.has_comm = comm != nullptr;
  env.force_collectives = force_collectives;
  env.batch_mode = batch_mode;
  pgo::PlanKnobs kn;
  kn.pad_tiles = knob("pad_tiles");
  kn.spmv_pipe = knob("spmv_pipe");
  kn.fused_p = knob("fused_p");
  kn.single_reduction = knob("single_reduction");
  kn.verify_residual = knob("verify_residual");
  kn.direct_fail_at = knob("direct_fail_at");
  plan.pre = pgo::plan_pre(opt, env, N, E, ia, ib);
  if (plan.pre.no) return fail(plan.pre.no.status, plan.pre.no.why);
  const int chain_len = plan.pre.chain_len;
  std::vector<int32_t> ia_p, ib_p;
  std::vector<double> poses_p;
  fixed_internal = opt.fixed_pose;
  HIPC(hipSetDevice(device));
  HIPC(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  if (plan.pre.reorder) {
    // chain segments must stay contiguous under the renumbering.  The ordering is host work on the WHOLE edge list
    // (0.7 s at 1M poses): a process-wide cache serves repeated handles on the same graph, and with several ranks only
    // rank 0 computes it -- the others receive it through the communicator (a sum in which they contribute zeros: the one
    // collective both back-ends have for this), so a node does not spend ranks x 0.7 s of CPU on identical work.
    const int seg = plan.pre.order_segment;
    if (world == 1) {
      PGOC(pgo::cached_pose_order(N, E, ia, ib, seg, &perm));
    } else {
      if (rank == 0) PGOC(pgo::cached_pose_order(N, E, ia, ib, seg, &perm));
      else perm.assign((size_t)N, 0);
      std::vector<double> tmp((size_t)N);
      for (int32_t i = 0; i < N; ++i) tmp[i] = (double)perm[i];
      double* d_tmp = nullptr;
      HIPC(hipMalloc((void**)&d_tmp, (size_t)N * sizeof(double)));
      HIPC(hipMemcpyAsync(d_tmp, tmp.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice, stream));
      int st_b = PGO_OK;
      for (int64_t off = 0; off < N && st_b == PGO_OK; off += (1 << 16))   // 512 KiB pieces (a slot of the shm test back-end)
        if (comm->allreduce(d_tmp + off, (int)std::min<int64_t>(N - off, 1 << 16), false, stream) != 0)
          st_b = fail(PGO_ERR_COMM, "pose ordering: broadcast through the communicator failed");
      if (st_b == PGO_OK && hipMemcpyAsync(tmp.data(), d_tmp, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess)
        st_b = fail(PGO_ERR_HIP, "pose ordering: copy back");
      if (st_b == PGO_OK && hipStreamSynchronize(stream) != hipSuccess) st_b = fail(PGO_ERR_HIP, "pose ordering: synchronise");
      (void)hipFree(d_tmp);
      PGOC(st_b);
      for (int32_t i = 0; i < N; ++i) perm[i] = (int32_t)tmp[i];
    }
    ia_p.resize(E);
    ib_p.resize(E);
    for (int32_t e = 0; e < E; ++e) {
      ia_p[e] = perm[ia[e]];
      ib_p[e] = perm[ib[e]];
    }
    poses_p.resize((size_t)3 * N);
    for (int64_t i = 0; i < N; ++i) memcpy(&poses_p[(size_t)3 * perm[i]], poses_h + 3 * i, 3 * sizeof(double));
    ia = ia_p.data();
    ib = ib_p.data();
    poses_h = poses_p.data();
    if (fixed_internal >= 0) fixed_internal = perm[fixed_internal];
  }
  PGOC(pgo::build_shard_structure(N, E, ia, ib, meas, kind, opt.method, world, rank, (int)plan.pre.row_align, &S,
                                  tile_breaks_h.empty() ? nullptr : &tile_breaks_h));
  default_losses();
  kind_local.resize((size_t)S.n_edges_local);   // (pgo_set_losses' default classes follow the edge kind)
  for (int32_t k = 0; k < S.n_edges_local; ++k) kind_local[k] = kind[S.orig_edge[k]];
  if (pgo::plan_padding(kn, env, S.n_tiles())) (void)pgo::pad_tiles_to_slots(&S);
  n_full = (int64_t)world * S.rows_per_rank;
  const int64_t EL = S.n_edges_local, NL = S.n_loc;
  // ---- the plan: every decision, from host facts alone, before the first buffer.  Refusals in the order they always had.
  pgo::ShardFacts F;
  F.N = N;
  F.E = E;
  F.NL = NL;
  F.EL = EL;
  F.n_tiles = S.n_tiles();
  F.n_inc = S.n_inc;
  F.rows_per_rank = S.rows_per_rank;
  F.lo = S.lo;
  for (int t = 0; t < S.n_tiles(); ++t) {
    const int32_t r0 = S.tile_row[t], r1 = S.tile_row[t + 1], n_inc_t = S.inc_ptr[r1] - S.inc_ptr[r0];
    F.tiles_fit_wg = F.tiles_fit_wg && n_inc_t <= dev::WG;
    F.tiles_plain = F.tiles_plain && n_inc_t <= dev::WG && (r1 - r0) * 3 <= dev::WG;
  }
  {
    const pgo::PlanShard sh = pgo::plan_shard(opt, env, kn, plan.pre, F);
    if (sh.no) return fail(sh.no.status, sh.no.why);
    plan.all = sh.all;
    plan.own = sh.own;
  }
  {
    pgo::DirectFacts D;
    D.N = N;
    D.info_mode = info_mode;
    D.has_constant_pose = fixed_internal >= 0;
    D.permuted = !perm.empty();
    if (pgo::plan_direct_gate(opt, env, D).need_chain) {
      std::vector<int32_t> chain, lr, va, vb;
      D.gap = direct_chain_lists(&chain, &lr, &va, &vb);
      D.m = (int)lr.size();
    }
    plan.dl = pgo::plan_direct(opt, env, kn, D);
    if (plan.dl.no) return fail(plan.dl.no.status, plan.dl.no.why);
  }
  // (after the direct solver's decision: auto adds the coarse level only to solves that stay on PCG)
  plan.co = pgo::plan_coarse(opt, env, F, plan.dl.direct, opt.pcg_coarse_poses);
  if (plan.co.no) return fail(plan.co.no.status, plan.co.no.why);
  if (!plan.co.on) plan.co_cov = pgo::plan_coarse_for_covariance(opt, env, F);
  pgo::plan_finish(opt, &plan);
  const pgo::PlanOwn& O = plan.own;

  PGOC(dalloc(&poses, 3 * n_full));
  PGOC(dalloc(&cand, 3 * n_full));
  PGOC(dalloc(&scale, 3 * n_full));
  PGOC(dalloc(&p_full, dev::PS * n_full));
  PGOC(dalloc(&e_ia, EL));
  PGOC(dalloc(&e_ib, EL));
  PGOC(dalloc(&e_mx, EL));
  PGOC(dalloc(&e_my, EL));
  PGOC(dalloc(&e_mt, EL));
  PGOC(dalloc(&e_flags, EL));
  PGOC(dalloc(&jr, EL * rec_doubles));
  if (info6) PGOC(dalloc(&e_info, 6 * std::max<int64_t>(EL, 1)));
  PGOC(dalloc(&inc_ptr, NL + 1));
  PGOC(dalloc(&inc_edge, S.n_inc));
  PGOC(dalloc(&inc_col, S.n_inc));
  PGOC(dalloc(&tile_row, (int64_t)S.tile_row.size()));
  PGOC(dalloc(&inc_rowoff, std::max<int64_t>(S.n_inc, 1)));
  PGOC(dalloc(&hoff, 9 * O.inc_stride));
  PGOC(dalloc(&hd, 6 * NL));
  PGOC(dalloc(&gs, 3 * NL));
  PGOC(dalloc(&d2, 3 * NL));
  PGOC(dalloc(&minv, 6 * NL));
  PGOC(dalloc(&hdd, 3 * NL));
  PGOC(dalloc(&y, 3 * NL));
  PGOC(dalloc(&r, 3 * NL));
  PGOC(dalloc(&z, 3 * NL));
  PGOC(dalloc(&ap, 3 * NL));
  has_sw = (opt.method == 2);
  if (has_sw) {
    for (double** ptr : {&sw, &sw_cand, &sw_sigma, &sw_c, &sw_gamma, &sw_gs, &sw_den, &sw_hss}) PGOC(dalloc(ptr, EL));
    PGOC(dalloc(&sw_js, 3 * EL));
    PGOC(dalloc(&diag_full, 3 * NL));
    PGOC(dalloc(&gs_full, 3 * NL));
  }
  PGOC(dalloc(&st, 1));
  PGOC(dalloc(&scal, N_SCAL));
  PGOC(dalloc(&bad, 1));
  HIPC(hipHostMalloc((void**)&h_st, sizeof(dev::CgState)));
  HIPC(hipHostMalloc((void**)&h_scal, N_SCAL * sizeof(double)));

  for (int k = 0; k < N_PART; ++k) PGOC(dalloc(&part[k], O.part_cap));
  PGOC(dalloc(&fold_buf, 6 * 16));

  HIPC(hipMemcpyAsync(poses, poses_h, (size_t)3 * N * sizeof(double), hipMemcpyHostToDevice, stream));
  PGOC(sync());  // poses_p (reordered copy) dies with this call
  PGOC(upload(e_ia, S.ia));
  PGOC(upload(e_ib, S.ib));
  PGOC(upload(e_mx, S.mx));
  PGOC(upload(e_my, S.my));
  PGOC(upload(e_mt, S.mt));
  PGOC(upload(e_flags, S.flags));
  if (info6) {  // planes over the local edges
    std::vector<double> planes((size_t)6 * EL);
    for (int64_t k = 0; k < EL; ++k)
      for (int c = 0; c < 6; ++c) planes[(size_t)c * EL + k] = info6[6 * (size_t)S.orig_edge[k] + c];
    PGOC(upload(e_info, planes));
    PGOC(sync());  // `planes` dies with this scope
  }
  PGOC(upload(inc_ptr, S.inc_ptr));
  PGOC(upload(inc_edge, S.inc_edge));
  PGOC(upload(inc_col, S.inc_col));
  PGOC(upload(tile_row, S.tile_row));
  PGOC(upload(inc_rowoff, S.inc_rowoff));
  {  // one 16-byte descriptor per tile for K3: {first local row, rows, first incidence, incidences}
    // in row order: a breadth-first order of the tile graph cuts the gather traffic (FETCH_SIZE 992 -> 920-937 MB at 1M
    // poses) but the scattered 18-KB H chunks cost more than that saves (184 vs 179 us)
    std::vector<int4> desc((size_t)std::max(1, S.n_tiles()));
    for (int t = 0; t < S.n_tiles(); ++t) {
      const int32_t r0 = S.tile_row[t], r1 = S.tile_row[t + 1];
      desc[t] = make_int4(r0, r1 - r0, S.inc_ptr[r0], S.inc_ptr[r1] - S.inc_ptr[r0]);
    }
    PGOC(dalloc(&tile_desc, (int64_t)desc.size()));
    PGOC(upload(tile_desc, desc));
    PGOC(sync());  // `desc` dies with this scope
  }
  if (has_sw) {  // switches start at 1.0 (main.cpp:117,139)
    std::vector<double> ones((size_t)EL, 1.0);
    PGOC(upload(sw, ones));
    PGOC(upload(sw_cand, ones));
    PGOC(sync());  // `ones` dies with this scope
  }
  // halo lists for the point-to-point exchange of the search direction
  if (plan.all.use_halo) {
    PGOC(dalloc(&halo_send_rows, (int64_t)S.halo_send_row.size()));
    PGOC(dalloc(&halo_recv_rows, (int64_t)S.halo_recv_row.size()));
    PGOC(dalloc(&halo_send_buf, 3 * (int64_t)S.halo_send_row.size()));
    PGOC(dalloc(&halo_recv_buf, 3 * (int64_t)S.halo_recv_row.size()));
    PGOC(upload(halo_send_rows, S.halo_send_row));
    PGOC(upload(halo_recv_rows, S.halo_recv_row));
    halo_send_off3.resize(S.halo_send_off.size());
    halo_recv_off3.resize(S.halo_recv_off.size());
    for (size_t k = 0; k < S.halo_send_off.size(); ++k) {
      halo_send_off3[k] = 3 * S.halo_send_off[k];
      halo_recv_off3[k] = 3 * S.halo_recv_off[k];
    }
    if (O.overlap) {
      std::vector<int32_t> rows, ptr(1, 0), slots;
      for (int32_t r = 0; r < S.n_loc; ++r) {
        const size_t before = slots.size();
        for (int32_t q = S.inc_ptr[r]; q < S.inc_ptr[r + 1]; ++q)
          if (S.inc_col[q] < S.lo || S.inc_col[q] >= S.hi) slots.push_back(q);
        if (slots.size() > before) {
          rows.push_back(r);
          ptr.push_back((int32_t)slots.size());
        }
      }
      plan.own.n_rr = (int)rows.size();
      plan.own.g_rr = pgo::remote_rows_grid(O.n_rr);
      PGOC(dalloc(&rr_rows, std::max<int64_t>(1, O.n_rr)));
      PGOC(dalloc(&rr_ptr, (int64_t)ptr.size()));
      PGOC(dalloc(&rr_slots, std::max<int64_t>(1, (int64_t)slots.size())));
      PGOC(upload(rr_rows, rows));
      PGOC(upload(rr_ptr, ptr));
      PGOC(upload(rr_slots, slots));
      PGOC(sync());  // the lists die with this scope
      HIPC(hipStreamCreateWithFlags(&comm_stream, hipStreamNonBlocking));
      HIPC(hipEventCreateWithFlags(&ev_pack, hipEventDisableTiming));
      HIPC(hipEventCreateWithFlags(&ev_halo, hipEventDisableTiming));
    }
  }
  if (O.grp_B > 1) {   // block-Jacobi over groups of B poses: explicit dense inverses
    PGOC(dalloc(&ginv, (int64_t)O.n_groups * O.grp_nb * O.grp_nb));
    if (O.grp_lds > 48 * 1024)
      HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(dev::k_prepare_groups<>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)O.grp_lds));
  }
  if (chain_len) {   // (also on a rank that owns no rows: every rank must resolve to the same PCG loop and the same collectives)
    const int chain_pad = O.chain_pad;
    PGOC(dalloc(&chain_c, (int64_t)dev::CHAIN_REC * NL));   // zero-filled: rows without a block (i, i-1) keep C = 0
    {
      std::vector<int32_t> dup;
      for (int32_t r = 1; r < S.n_loc; ++r) {
        if ((r % chain_len) == 0) continue;
        int cnt = 0;
        for (int32_t q = S.inc_ptr[r]; q < S.inc_ptr[r + 1]; ++q) cnt += (S.inc_col[q] == S.lo + r - 1);
        if (cnt > 1) dup.push_back(r);
      }
      n_chain_dup = (int)dup.size();
      if (n_chain_dup) {
        PGOC(dalloc(&chain_dup_rows, n_chain_dup));
        PGOC(upload(chain_dup_rows, dup));
        PGOC(sync());  // `dup` dies with this scope
      }
    }
    PGOC(dalloc(&chain_w, 9 * (int64_t)chain_pad));
    PGOC(dalloc(&chain_s, 6 * (int64_t)chain_pad));
    // the padding rows of the factor planes are never written: they must read as 0
    HIPC(hipMemsetAsync(chain_w, 0, (size_t)9 * chain_pad * sizeof(double), stream));
    HIPC(hipMemsetAsync(chain_s, 0, (size_t)6 * chain_pad * sizeof(double), stream));
  }
  if (plan.all.fused_p_buffer) PGOC(dalloc(&p_full2, dev::PS * n_full));
  if (plan.all.sr_buffer) PGOC(dalloc(&sr_s, 3 * NL));
  if (!fixed_mask_h.empty()) {
    PGOC(dalloc(&fixed_mask, (int64_t)fixed_mask_h.size()));
    PGOC(upload(fixed_mask, fixed_mask_h));
  }
  if (batch_mode) PGOC(dalloc(&edge_cost, std::max<int64_t>(EL, 1)));
  {  // what pgo_handle_info reports while no active set is in force: every edge, opt.fixed_pose + the poses without an edge
     // (one numbering throughout: with the pose ordering on, ia / ib were replaced by their renumbered copies above, so they
     // index poses as fixed_internal and fixed_mask_h do)
    std::vector<uint8_t> used((size_t)N, 0);
    for (int32_t e = 0; e < E; ++e) used[ia[e]] = used[ib[e]] = 1;
    n_active_edges = E;
    n_constant_poses = 0;
    for (int32_t i = 0; i < N; ++i)
      n_constant_poses += (i == fixed_internal || (!fixed_mask_h.empty() && fixed_mask_h[i]) || !used[i]) ? 1 : 0;
  }
  if (plan.dl.direct) PGOC(direct_build());
  if (plan.co.on) PGOC(coarse_build(E, ia, ib));
  return sync();
}

// ---------------------------------------------------------------------------------------------------------------
// Second preconditioner level (coarse.hip.h): the block lists and buffers of the level the plan sized (CO(): the LM loop's, or
// the one covariance calls build for themselves -- plan_coarse, plan_coarse_for_covariance).
int pgo_handle::coarse_build(int32_t E, const int32_t* ia, const int32_t* ib) {
  const int world = comm ? comm->world : 1, rank = comm ? comm->rank : 0;
  const pgo::CoarsePlan& C = CO();
  const bool multi = C.co_multi;
  const int64_t NL = S.n_loc, N = S.n_poses;
  const int co_agg = C.co_agg, co_nagg = C.co_nagg, co_aoff = C.co_aoff, co_nown = C.co_nown, co_Kp = C.co_Kp, co_ndot = C.co_ndot;
  // coarse blocks of the own aggregates and their fine entries: incidences sorted by (aggregate of the row, aggregate of the
  // column, position); the column's aggregate may be a peer's (halo)
  std::vector<uint64_t> key((size_t)S.n_inc);
  {
    size_t k = 0;
    for (int32_t r = 0; r < S.n_loc; ++r)
      for (int32_t q = S.inc_ptr[r]; q < S.inc_ptr[r + 1]; ++q) {
        const uint64_t I = (uint64_t)((S.lo + r) / co_agg), J = (uint64_t)(S.inc_col[q] / co_agg);
        key[k++] = ((I * (uint64_t)co_nagg + J) << 32) | (uint32_t)q;
      }
  }
  std::sort(key.begin(), key.end());
  std::vector<int32_t> row_of((size_t)S.n_inc);
  for (int32_t r = 0; r < S.n_loc; ++r)
    for (int32_t q = S.inc_ptr[r]; q < S.inc_ptr[r + 1]; ++q) row_of[q] = S.lo + r;
  std::vector<int32_t> cbi, cbj, cbp, cbq((size_t)S.n_inc), cbr((size_t)S.n_inc);
  {
    size_t k = 0;
    int next_diag = co_aoff;   // every aggregate gets its (I, I) block, also without an off-diagonal fine entry inside
    const int end_diag = co_aoff + co_nown;
    auto open_block = [&](int I, int J) {
      cbi.push_back(I);
      cbj.push_back(J);
      cbp.push_back((int32_t)k);
    };
    while (k < key.size() || next_diag < end_diag) {
      const uint64_t blk = k < key.size() ? (key[k] >> 32) : ~0ull;
      const uint64_t dblk = next_diag < end_diag ? (uint64_t)next_diag * co_nagg + next_diag : ~0ull;
      if (dblk < blk) {   // a diagonal block without fine off-diagonal entries
        open_block(next_diag, next_diag);
        ++next_diag;
        continue;
      }
      if (dblk == blk) ++next_diag;
      open_block((int)(blk / co_nagg), (int)(blk % co_nagg));
      while (k < key.size() && (key[k] >> 32) == blk) {
        const int32_t q = (int32_t)(key[k] & 0xffffffffu);
        cbq[k] = q;
        cbr[k] = row_of[q];
        ++k;
      }
    }
    cbp.push_back((int32_t)k);
  }
  co_ncb = (int)cbi.size();
  // aggregates with no pose in the coarse space: every pose edge-less (no real incidence; k_coarse_basis tests the same through
  // H_ii = 0) or the constant pose.  Their block (I, I) is zero; k_coarse_dead puts identity there, as on the padding.
  std::vector<int32_t> dead;
  coarse_dead_list(&dead);
  if (multi) PGOC(coarse_setup_multi(E, ia, ib, world, rank, cbi, cbj, dead, &dead));   // (dead: every rank's, afterwards)
  co_ndead = (int)dead.size();
  if (co_ndead) {
    PGOC(dalloc(&co_dead, co_ndead));
    co_dead_cap = co_ndead;
    PGOC(upload(co_dead, dead));
  }
  PGOC(dalloc(&co_pb, 5 * (multi ? N : NL)));
  PGOC(dalloc(&co_cap, (int64_t)co_Kp * co_Kp));
  PGOC(dalloc(&co_nm, (int64_t)co_Kp * co_Kp));
  PGOC(dalloc(&co_dwork, (int64_t)(co_Kp / 32) * 1024));
  if (multi) {
    PGOC(dalloc(&co_red, co_Kp + 2));
    co_rc = co_red;
  } else {
    PGOC(dalloc(&co_rc, co_Kp));
  }
  PGOC(dalloc(&co_cy, co_Kp));
  PGOC(dalloc(&co_ec, co_Kp));
  PGOC(dalloc(&co_ok, 1));
  if (C.co_explicit) PGOC(dalloc(&co_ainv, (int64_t)co_Kp * co_Kp));
  if (multi) PGOC(dalloc(&co_dotp, co_ndot));
  PGOC(dalloc(&co_cb_i, co_ncb));
  PGOC(dalloc(&co_cb_j, co_ncb));
  PGOC(dalloc(&co_cb_ptr, co_ncb + 1));
  PGOC(dalloc(&co_cb_q, std::max<int64_t>(1, S.n_inc)));
  PGOC(dalloc(&co_cb_row, std::max<int64_t>(1, S.n_inc)));
  PGOC(upload(co_cb_i, cbi));
  PGOC(upload(co_cb_j, cbj));
  PGOC(upload(co_cb_ptr, cbp));
  PGOC(upload(co_cb_q, cbq));
  PGOC(upload(co_cb_row, cbr));
  PGOC(sync());   // the host lists die with this scope
  HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(dev::k_chol_panel<>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dev::CHOL_LDS_BYTES));
  return PGO_OK;
}

// The own aggregates with no pose in the coarse space.  With an active set in force (pgo_set_active) those are the aggregates
// whose poses are all resolved-constant: every other pose has an active edge.
void pgo_handle::coarse_dead_list(std::vector<int32_t>* dead) const {
  const int64_t NL = S.n_loc;
  dead->clear();
  const int co_agg = CO().co_agg, co_nown = CO().co_nown, co_aoff = CO().co_aoff;
  for (int Il = 0; Il < co_nown; ++Il) {
    bool any = false;
    for (int32_t r = Il * co_agg; r < std::min<int64_t>(NL, (int64_t)(Il + 1) * co_agg) && !any; ++r) {
      if (!act_const_h.empty()) {
        any = !act_const_h[(size_t)S.lo + r];
        continue;
      }
      if (S.lo + r == fixed_internal) continue;
      for (int32_t q = S.inc_ptr[r]; q < S.inc_ptr[r + 1] && !any; ++q) any = S.inc_edge[q] >= 0;
    }
    if (!any) dead->push_back(co_aoff + Il);
  }
}

// Several ranks: the edge mask of the basis planes, and the coarse coordinates of every rank's blocks and dead aggregates --
// all-gathered once, in lists padded to the longest rank's (the counts agreed by an all-reduce), so that every rank knows
// where each gathered block value lands in the dense matrix.  A rank that owns no rows contributes empty lists.
int pgo_handle::coarse_setup_multi(int32_t E, const int32_t* ia, const int32_t* ib, int world, int rank, const std::vector<int32_t>& cbi,
                                   const std::vector<int32_t>& cbj, const std::vector<int32_t>& dead, std::vector<int32_t>* gdead) {
  const int64_t N = S.n_poses;
  {
    std::vector<uint8_t> live((size_t)N, 0);
    for (int32_t e = 0; e < E; ++e) live[ia[e]] = live[ib[e]] = 1;
    PGOC(dalloc(&co_live, N));
    PGOC(upload(co_live, live));
    PGOC(sync());   // `live` dies with this scope
  }
  double* d_buf = nullptr;
  auto coll = [&](int64_t n, const std::function<int()>& body) -> int {   // body on a temporary device buffer of n doubles
    HIPC(hipMalloc((void**)&d_buf, (size_t)std::max<int64_t>(n, 1) * sizeof(double)));
    const int st_b = body();
    (void)hipFree(d_buf);
    d_buf = nullptr;
    return st_b;
  };
  double cnt[2] = {(double)cbi.size(), (double)dead.size()};
  PGOC(coll(2, [&]() -> int {
    HIPC(hipMemcpyAsync(d_buf, cnt, sizeof cnt, hipMemcpyHostToDevice, stream));
    if (comm->allreduce(d_buf, 2, true, stream) != 0) return fail(PGO_ERR_COMM, "coarse level: all-reduce of the block counts failed");
    HIPC(hipMemcpyAsync(cnt, d_buf, sizeof cnt, hipMemcpyDeviceToHost, stream));
    return sync();
  }));
  co_ncb_max = (int)cnt[0];
  const int64_t ndm = (int64_t)cnt[1], cpr = 2 * (int64_t)co_ncb_max + ndm;
  std::vector<double> all((size_t)(world * cpr), -1.0);
  for (size_t b = 0; b < cbi.size(); ++b) {
    all[(size_t)(rank * cpr + 2 * b)] = cbi[b];
    all[(size_t)(rank * cpr + 2 * b + 1)] = cbj[b];
  }
  for (size_t d = 0; d < dead.size(); ++d) all[(size_t)(rank * cpr + 2 * co_ncb_max + d)] = dead[d];
  PGOC(coll(world * cpr, [&]() -> int {
    HIPC(hipMemcpyAsync(d_buf, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    if (comm->allgather_inplace(d_buf, cpr, stream) != 0) return fail(PGO_ERR_COMM, "coarse level: all-gather of the block lists failed");
    HIPC(hipMemcpyAsync(all.data(), d_buf, all.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    return sync();
  }));
  const int64_t nblk = (int64_t)world * co_ncb_max;
  std::vector<int32_t> gi((size_t)std::max<int64_t>(nblk, 1), -1), gj((size_t)std::max<int64_t>(nblk, 1), -1);
  gdead->clear();
  for (int r = 0; r < world; ++r) {
    for (int b = 0; b < co_ncb_max; ++b) {
      gi[(size_t)r * co_ncb_max + b] = (int32_t)all[(size_t)(r * cpr + 2 * b)];
      gj[(size_t)r * co_ncb_max + b] = (int32_t)all[(size_t)(r * cpr + 2 * b + 1)];
    }
    for (int64_t d = 0; d < ndm; ++d) {
      const double v = all[(size_t)(r * cpr + 2 * co_ncb_max + d)];
      if (v >= 0.0) gdead->push_back((int32_t)v);
    }
  }
  PGOC(dalloc(&co_gi, nblk));
  PGOC(dalloc(&co_gj, nblk));
  PGOC(dalloc(&co_gvals, 9 * nblk));
  PGOC(upload(co_gi, gi));
  PGOC(upload(co_gj, gj));
  return sync();   // (the host lists die with this scope)
}

// ---------------------------------------------------------------------------------------------------------------
// Direct solve for small chain-like graphs (direct.hip.h): the lists and buffers of what plan_direct sized (plan.dl), at create() or
// when the direct solve takes over from PCG (lm_iteration).

// The odometry chain (the first local edge between every pair of consecutive poses) and the other edges with their endpoints;
// returns the first pose without a chain edge to its successor, or -1 (the lists are complete only then).
int32_t pgo_handle::direct_chain_lists(std::vector<int32_t>* chain, std::vector<int32_t>* lr, std::vector<int32_t>* va, std::vector<int32_t>* vb) const {
  const int64_t EL = S.n_edges_local;
  const int32_t gap = pgo::pick_chain_edges(S.n_poses, EL, S.ia.data(), S.ib.data(), chain);
  if (gap >= 0) return gap;
  for (int64_t e = 0; e < EL; ++e) {
    const int32_t lo_p = std::min(S.ia[e], S.ib[e]);
    if (std::max(S.ia[e], S.ib[e]) == lo_p + 1 && (*chain)[lo_p] == (int32_t)e) continue;
    lr->push_back((int32_t)e);
    va->push_back(S.ia[e]);
    vb->push_back(S.ib[e]);
  }
  return -1;
}

int pgo_handle::direct_build() {
  const pgo::DirectPlan& D = plan.dl;
  const int32_t N = S.n_poses;
  const int dl_m = D.dl_m, dl_Kp = D.dl_Kp, dl_ld = D.dl_ld, dl_nsep = D.dl_nsep, dl_nU = D.dl_nU, dl_nseg = D.dl_nseg;
  std::vector<int32_t> chain, lr, va, vb;
  (void)direct_chain_lists(&chain, &lr, &va, &vb);
  PGOC(dalloc(&dl_chain_edge, N));
  PGOC(dalloc(&dl_lr_edge, std::max(1, dl_m)));
  PGOC(dalloc(&dl_va, std::max(1, dl_m)));
  PGOC(dalloc(&dl_vb, std::max(1, dl_m)));
  PGOC(upload(dl_chain_edge, chain));
  PGOC(upload(dl_lr_edge, lr));
  PGOC(upload(dl_va, va));
  PGOC(upload(dl_vb, vb));
  if (knob("direct_setup_fail") > 0) return fail(PGO_ERR_NOMEM, "hipMalloc: out of memory (test hook direct_setup_fail)");
  PGOC(dalloc(&dl_trec, (int64_t)dev::DLR_REC * N));
  PGOC(dalloc(&dl_fac, (int64_t)dev::DLR_REC * (N + 1)));
  PGOC(dalloc(&dl_vrec, (int64_t)dev::DLR_V * std::max(1, dl_m)));
  PGOC(dalloc(&dl_Z, (int64_t)3 * N * dl_ld));
  PGOC(dalloc(&dl_x1, (int64_t)3 * N * 64));
  PGOC(dalloc(&dl_cap, (int64_t)dl_Kp * dl_Kp));
  PGOC(dalloc(&dl_dwork, (int64_t)(dl_Kp / 32) * 1024));
  PGOC(dalloc(&dl_nm, (int64_t)dl_Kp * dl_Kp));
  PGOC(dalloc(&dl_cy, dl_Kp));
  PGOC(dalloc(&dl_pre, (int64_t)dev::DLR_PRE * N));
  if (D.dl_fine) PGOC(dalloc(&dl_pre2, (int64_t)dev::DLR_PRE * N));
  PGOC(dalloc(&dl_E, (int64_t)dl_nseg * 3 * dl_ld));
  PGOC(dalloc(&dl_E2, (int64_t)dl_nseg * 3 * dl_ld));
  HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(dev::k_chol_panel<>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dev::CHOL_LDS_BYTES));
  PGOC(dalloc(&dl_cvec, dl_Kp));
  PGOC(dalloc(&dl_ksep, 18 * std::max(1, dl_nsep)));
  PGOC(dalloc(&dl_R, std::max(1, dl_nU * dl_nU)));
  PGOC(dalloc(&dl_Wm, (int64_t)std::max(1, dl_nU) * dl_ld));
  PGOC(sync());  // the host lists die with this scope
  dl_ready = true;
  return PGO_OK;
}

