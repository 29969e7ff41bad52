// pgo_window_solve (include/pgo.h, "window solves"): the host half.  Every list of the call is checked and resolved here --
// caller's pose -> row of the handle's pose array, caller's edge -> local edge, endpoints -> list positions, and the
// contribution list of every 3x3 block of the window's J'J -- before anything is launched; then ONE launch of
// k_window_solve (window.hip.h), one workgroup per window, and one copy-out.
#include "solver_handle.hip.h"
#include "window.hip.h"

int pgo_handle::window_solve(const char* who, int32_t nw, const int32_t* pose_ptr, const int32_t* pose_idx, const int32_t* edge_ptr,
                             const int32_t* edge_idx, const int32_t* anchor, int32_t max_iters, int32_t commit, double* poses_out,
                             pgo_window_result* results, pgo_iter_record* records) {
  const std::string W = std::string(who) + ": ";
  PGOC(requires(who, METHOD_01 | NO_INFO | ONE_RANK));   // (a batch is allowed: pgo_batch_window_solve)
  if (w_set)   // (k_window_solve evaluates the edges itself and does not read the plane)
    return fail(PGO_ERR_UNSUPPORTED, W + "not while edge weights are set (pgo_set_edge_weights(h, NULL) first)");
  if (pri_n > 0)   // (k_window_solve assembles its own system, which does not know the pose priors)
    return fail(PGO_ERR_UNSUPPORTED, W + "not while pose priors are set (pgo_set_priors(h, 0, ...) first)");
  if (nw < 0) return fail(PGO_ERR_INVALID_ARG, W + "n_windows < 0");
  if (nw == 0) return PGO_OK;
  if (!pose_ptr || !pose_idx || !edge_ptr || !edge_idx || !anchor || !results) return fail(PGO_ERR_INVALID_ARG, W + "null pointer");
  if (max_iters < 1 || max_iters > PGO_WINDOW_MAX_ITERS)
    return fail(PGO_ERR_INVALID_ARG, W + "max_iters must be 1.." + std::to_string(PGO_WINDOW_MAX_ITERS));
  if (pose_ptr[0] != 0 || edge_ptr[0] != 0) return fail(PGO_ERR_INVALID_ARG, W + "pose_ptr[0] and edge_ptr[0] must be 0");
  for (int32_t w = 0; w < nw; ++w)
    if (pose_ptr[w + 1] < pose_ptr[w] || edge_ptr[w + 1] < edge_ptr[w])
      return fail(PGO_ERR_INVALID_ARG, W + "window " + std::to_string(w) + ": pose_ptr / edge_ptr must not decrease");
  for (int32_t w = 0; w < nw; ++w) {
    const int32_t np = pose_ptr[w + 1] - pose_ptr[w], ne = edge_ptr[w + 1] - edge_ptr[w];
    if (np > PGO_WINDOW_MAX_POSES || ne > PGO_WINDOW_MAX_EDGES)
      return fail(PGO_ERR_UNSUPPORTED, W + "window " + std::to_string(w) + " has " + std::to_string(np) + " poses and " + std::to_string(ne) +
                                           " edges: above the cap of " + std::to_string(PGO_WINDOW_MAX_POSES) + " / " +
                                           std::to_string(PGO_WINDOW_MAX_EDGES) + " (use pgo_set_active)");
  }
  const int64_t N = S.n_poses, EL = S.n_edges_local, TP = pose_ptr[nw], TE = edge_ptr[nw];
  if (win_edge_local.empty() && EL > 0) {   // (one rank: every edge is local)
    win_edge_local.assign((size_t)n_edges_total, -1);
    for (int64_t k = 0; k < EL; ++k) win_edge_local[S.orig_edge[k]] = (int32_t)k;
  }
  if (win_pos.empty()) {
    win_pos.assign((size_t)N, -1);
    win_owner.assign((size_t)N, -1);
  }
  // ---- host image: desc | pidx | eloc | eab | blk | blk_ptr | ent  (blocks <= poses + edges, contributions <= 3 x edges)
  pgo::Layout LI;
  const auto s_desc = LI.add<dev::WinDesc>(nw);
  const auto s_pidx = LI.add<int32_t>(TP), s_eloc = LI.add<int32_t>(TE), s_eab = LI.add<int32_t>(TE), s_blk = LI.add<int32_t>(TP + TE),
             s_bptr = LI.add<int32_t>(TP + TE + 1), s_ent = LI.add<int32_t>(3 * TE);
  win_host.assign((size_t)LI.bytes(), 0);
  dev::WinDesc* const h_desc = s_desc.in(win_host.data());
  int32_t *const h_pidx = s_pidx.in(win_host.data()), *const h_eloc = s_eloc.in(win_host.data()), *const h_eab = s_eab.in(win_host.data()),
                *const h_blk = s_blk.in(win_host.data()), *const h_bptr = s_bptr.in(win_host.data()), *const h_ent = s_ent.in(win_host.data());
  int64_t n_blk = 0, n_ent = 0;
  int n3cap = 3;
  int status = PGO_OK;
  std::string msg;
  auto bad = [&](int32_t w, const std::string& what) {
    status = PGO_ERR_INVALID_ARG;
    msg = W + "window " + std::to_string(w) + ": " + what;
  };
  for (int32_t w = 0; w < nw && status == PGO_OK; ++w) {
    const int32_t p0 = pose_ptr[w], np = pose_ptr[w + 1] - p0, e0 = edge_ptr[w], ne = edge_ptr[w + 1] - e0;
    int32_t listed = 0;
    for (int32_t k = 0; k < np && status == PGO_OK; ++k) {
      const int32_t i = pose_idx[p0 + k];
      if (i < 0 || i >= N) {
        bad(w, "pose index " + std::to_string(i) + " out of range");
        break;
      }
      const int32_t row = perm.empty() ? i : perm[i];
      if (win_pos[row] >= 0) {
        bad(w, "pose " + std::to_string(i) + " is listed twice");
        break;
      }
      if (commit && win_owner[row] >= 0) {
        bad(w, "pose " + std::to_string(i) + " is also in window " + std::to_string(win_owner[row]) + " (commit needs disjoint lists)");
        break;
      }
      win_pos[row] = k;
      win_owner[row] = w;
      h_pidx[p0 + k] = row;
      listed = k + 1;
    }
    int32_t anchor_pos = -1;
    if (status == PGO_OK) {
      const int32_t a = anchor[w];
      if (a < 0 || a >= N || win_pos[perm.empty() ? a : perm[a]] < 0) bad(w, "the anchor " + std::to_string(a) + " is not in the pose list");
      else anchor_pos = win_pos[perm.empty() ? a : perm[a]];
    }
    win_sort.clear();
    for (int32_t k = 0; k < ne && status == PGO_OK; ++k) {
      const int32_t e = edge_idx[e0 + k];
      if (e < 0 || e >= n_edges_total || win_edge_local[e] < 0) {
        bad(w, "edge index " + std::to_string(e) + " out of range");
        break;
      }
      const int32_t l = win_edge_local[e], pa = win_pos[S.ia[l]], pb = win_pos[S.ib[l]];
      if (pa < 0 || pb < 0) {
        bad(w, "an endpoint of edge " + std::to_string(e) + " is not in the pose list");
        break;
      }
      h_eloc[e0 + k] = l;
      h_eab[e0 + k] = pa | (pb << 8);
      // contributions, keyed (block, listed edge): sorting keeps every block's contributions in list order
      const uint32_t hi = (uint32_t)std::max(pa, pb), lo = (uint32_t)std::min(pa, pb), side_hi = pa > pb ? 0u : 1u;
      win_sort.push_back((uint32_t)pa << 17 | (uint32_t)pa << 9 | (uint32_t)k << 1 | 0u);
      win_sort.push_back((uint32_t)pb << 17 | (uint32_t)pb << 9 | (uint32_t)k << 1 | 1u);
      win_sort.push_back(1u << 25 | hi << 17 | lo << 9 | (uint32_t)k << 1 | side_hi);
    }
    for (int32_t k = 0; k < listed; ++k) win_pos[h_pidx[p0 + k]] = -1;   // idle again, whatever happened
    if (status != PGO_OK) break;
    std::sort(win_sort.begin(), win_sort.end());
    dev::WinDesc& D = h_desc[w];
    D.pose0 = p0;
    D.np = np;
    D.edge0 = e0;
    D.ne = ne;
    D.anchor = anchor_pos;
    D.blk0 = (int32_t)n_blk;
    size_t c = 0;
    for (int32_t p = 0; p < np; ++p) {   // the diagonal blocks first, one per listed pose (empty: a pose without an edge)
      h_blk[n_blk] = p | (p << 8);
      h_bptr[n_blk] = (int32_t)n_ent;
      ++n_blk;
      for (; c < win_sort.size() && (win_sort[c] >> 17) == (uint32_t)p; ++c) h_ent[n_ent++] = (int32_t)(win_sort[c] & 511u);
    }
    while (c < win_sort.size()) {        // then the blocks (p, q), p > q, that an edge joins
      const uint32_t key = win_sort[c] >> 9;
      h_blk[n_blk] = (int32_t)((key >> 8) & 255u) | (int32_t)((key & 255u) << 8);
      h_bptr[n_blk] = (int32_t)n_ent;
      ++n_blk;
      for (; c < win_sort.size() && (win_sort[c] >> 9) == key; ++c) h_ent[n_ent++] = (int32_t)(win_sort[c] & 511u);
    }
    D.nblk = (int32_t)n_blk - D.blk0;
    n3cap = std::max(n3cap, 3 * np);
  }
  h_bptr[n_blk] = (int32_t)n_ent;
  for (int64_t k = 0; k < TP; ++k) {   // (rows recorded so far; on an error the tail of the image is still 0)
    const int32_t row = h_pidx[k];
    if (row >= 0 && row < N) win_owner[row] = -1;
  }
  if (status != PGO_OK) return fail(status, msg);

  // ---- device
  HIPC(hipSetDevice(device));
  const int64_t rec_rows = (int64_t)max_iters + 1;
  pgo::Layout LW;   // work = per-edge records | poses out | results | iteration records
  const auto s_rec = LW.add<double>(TE * dev::WIN_REC), s_out = LW.add<double>(TP * 3);
  const auto s_res = LW.add<pgo_window_result>(nw);
  const auto s_its = LW.add<pgo_iter_record>(records ? nw * rec_rows : 0);
  PGOC(reserve(win_in, LI.bytes()));
  PGOC(reserve(win_work, LW.bytes()));
  const size_t lds_max = (size_t)dev::win_lds_doubles(3 * PGO_WINDOW_MAX_POSES) * sizeof(double);
  if (!win_lds_set) {   // more than 64 KiB of LDS needs the kernel's dynamic-LDS attribute
    HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(&dev::k_window_solve<>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    win_lds_set = true;
  }
  HIPC(hipMemcpyAsync(win_in.p, win_host.data(), win_host.size(), hipMemcpyHostToDevice, stream));
  if (records) HIPC(hipMemsetAsync(s_its.in(win_work.p), 0, (size_t)s_its.bytes(), stream));
  dev::WinArgs A;
  A.win = s_desc.in(win_in.p);
  A.pidx = s_pidx.in(win_in.p);
  A.eloc = s_eloc.in(win_in.p);
  A.eab = s_eab.in(win_in.p);
  A.blk = s_blk.in(win_in.p);
  A.blk_ptr = s_bptr.in(win_in.p);
  A.ent = s_ent.in(win_in.p);
  A.poses = poses;
  A.mx = e_mx;
  A.my = e_my;
  A.mt = e_mt;
  A.flags = e_flags;
  A.phi = opt.phi;
  A.loss0 = loss_cls[0];
  A.loss1 = loss_cls[1];
  A.loss2 = loss_cls[2];
  A.loss3 = loss_cls[3];
  A.max_iters = max_iters;
  A.jacobi_scaling = opt.jacobi_scaling;
  A.commit = commit ? 1 : 0;
  A.n3cap = n3cap;
  A.ftol = opt.ftol;
  A.gtol = opt.gtol;
  A.ptol = opt.ptol;
  A.radius0 = opt.radius0;
  A.max_radius = opt.max_radius;
  A.min_radius = opt.min_radius;
  A.min_relative_decrease = opt.min_relative_decrease;
  A.min_lm_diagonal = opt.min_lm_diagonal;
  A.max_lm_diagonal = opt.max_lm_diagonal;
  A.rec = s_rec.in(win_work.p);
  A.poses_out = s_out.in(win_work.p);
  A.results = s_res.in(win_work.p);
  A.records = records ? s_its.in(win_work.p) : nullptr;
  const size_t lds = (size_t)dev::win_lds_doubles(n3cap) * sizeof(double);
  hipLaunchKernelGGL(dev::k_window_solve<>, dim3(nw), dim3(dev::WIN_WG), lds, stream, A);
  PGOC(check_launch("k_window_solve"));
  if (poses_out && TP > 0) HIPC(hipMemcpyAsync(poses_out, A.poses_out, (size_t)s_out.bytes(), hipMemcpyDeviceToHost, stream));
  HIPC(hipMemcpyAsync(results, A.results, (size_t)s_res.bytes(), hipMemcpyDeviceToHost, stream));
  if (records) HIPC(hipMemcpyAsync(records, A.records, (size_t)s_its.bytes(), hipMemcpyDeviceToHost, stream));
  if (commit) solve_is_stale();   // as pgo_set_poses
  return sync();
}

extern "C" int pgo_window_solve(pgo_t* h, int32_t n_windows, const int32_t* pose_ptr, const int32_t* pose_idx, const int32_t* edge_ptr,
                                const int32_t* edge_idx, const int32_t* anchor, int32_t max_iters, int32_t commit, double* poses_out,
                                pgo_window_result* results, pgo_iter_record* records) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_window_solve: null handle");
  if (h->batch_mode) return fail(PGO_ERR_INVALID_ARG, "pgo_window_solve: a batched handle takes pgo_batch_window_solve");
  return h->window_solve("pgo_window_solve", n_windows, pose_ptr, pose_idx, edge_ptr, edge_idx, anchor, max_iters, commit, poses_out,
                         results, records);
}
